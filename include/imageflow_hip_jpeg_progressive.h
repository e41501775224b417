/* imageflow_hip_jpeg_progressive.h -- the device entropy decoder of progressive (SOF2) Huffman JPEG files
 * (csrc/jpeg_progressive_read.cpp, csrc/jpeg_progressive_core.hpp, csrc/jpeg_progressive_decode.hip).
 *
 * Why a header of its own: tests/test_gpu_stream_order.py compares every declaration of imageflow_hip.h that takes a
 * `void* hip_stream` with the rows of its table, and the batch entry's proof of stream order lives in a file of its own
 * (tests/test_gpu_jpeg_progressive_stream_order.py, built on the same tests/stream_order.py).  The declarations are folded
 * into imageflow_hip.h when that table gains its row.  Plain C99; includes imageflow_hip.h and is included by nothing.
 *
 * The contract is ifhip_jpeg_read_coefficients_host's: the quantised coefficient planes [blocks_h][blocks_w][64] int16, natural
 * order, MCU-padded, byte for byte what the host reader gives -- padding blocks included -- for every file that is prepared
 * and decodes with status 0. */
#ifndef IMAGEFLOW_HIP_JPEG_PROGRESSIVE_H
#define IMAGEFLOW_HIP_JPEG_PROGRESSIVE_H

#include "imageflow_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* A file's status word: 0 = decoded; else the OR of what its streams met.  A file with a nonzero word leaves its planes
 * undefined (but nothing outside them is touched) and its neighbours in the batch decode exactly; the caller asks the host
 * reader, whose verdict on the file stands. */
#define IFHIP_JPEG_PROG_NO_SUCH_CODE 1u  /* a bit pattern no code of the table starts with, or a DC size above 15       */
#define IFHIP_JPEG_PROG_PAST_SE 2u       /* a run carried the coefficient index past the end of the scan's band         */
#define IFHIP_JPEG_PROG_REFINE_SIZE 4u   /* a refinement symbol whose size is not 1                                     */
#define IFHIP_JPEG_PROG_OUT_OF_BITS 8u   /* a stream ended before its MCU count                                         */
#define IFHIP_JPEG_PROG_BOUNDS 16u       /* a block outside the plane (never, for records the front end wrote)          */

typedef struct ifhip_jpeg_progressive_prepared ifhip_jpeg_progressive_prepared;

/* The host front end (no device): walks the markers, un-stuffs every scan and cuts it at its restart markers into streams,
 * snapshots the Huffman tables and the restart interval in force at every SOS, latches the quantisation tables and gives
 * every scan its dependency level.  IFHIP_METHOD_NOT_IMPLEMENTED for every file the device path does not take: sequential
 * files (multi-scan ones included), progressions libjpeg would decode with JWRN_BOGUS_PROGRESSION (a refinement before its
 * first scan, two first scans of one band, a band over indices at different Al, AC before DC), Huffman tables that are no
 * prefix code, and whatever ifhip_jpeg_read_coefficients_host itself refuses -- its verdict on those stands. */
IFHIP_API int ifhip_jpeg_progressive_prepare(ifhip_jpeg_progressive_prepared** prepared, const uint8_t* jpeg, size_t len);
/* Null pointers are skipped.  qt3x64: the tables as latched at each component's first scan, natural order. */
IFHIP_API int ifhip_jpeg_progressive_prepared_info(const ifhip_jpeg_progressive_prepared* prepared, uint32_t* width, uint32_t* height,
                                                   int* n_components, uint8_t* h_samp3, uint8_t* v_samp3, uint32_t* blocks_w3,
                                                   uint32_t* blocks_h3, uint16_t* qt3x64, uint32_t* n_scans, uint32_t* n_streams,
                                                   uint32_t* n_levels);
IFHIP_API void ifhip_jpeg_progressive_prepared_destroy(ifhip_jpeg_progressive_prepared* prepared);

/* n prepared files of any mix of sizes, samplings and scan scripts into their planes: d_coef{0,1,2}[i] is plane 0, 1, 2 of file i
 * (device memory, 8-byte aligned; planes a file does not have may be null), plane_bytes[3 * i + c] the size of plane c of file
 * i, at least blocks_w * blocks_h * 128.  d_status[i] (device) receives the file's status word.  One clear of the planes, then
 * one launch per dependency level with every stream of that level of every file: the number of launches depends on the deepest
 * level in the batch alone.  The records are uploaded on hip_stream and the call waits for that copy before its first launch;
 * the kernels are asynchronous on hip_stream.  Argument checks come before the device check. */
IFHIP_API int ifhip_jpeg_progressive_decode_batch_device(const ifhip_jpeg_progressive_prepared* const* prepared, uint32_t n_files,
                                                         int16_t* const* d_coef0, int16_t* const* d_coef1, int16_t* const* d_coef2,
                                                         const size_t* plane_bytes, uint32_t* d_status, void* hip_stream);

/* One file, host buffers, synchronous on the null stream: planes sized by ifhip_jpeg_frame_info's facts, the latched tables in
 * qt3x64 (may be null).  *status receives the status word; with status == NULL a nonzero word fails the call. */
IFHIP_API int ifhip_jpeg_progressive_decode(const uint8_t* jpeg, size_t len, int16_t* coef0, int16_t* coef1, int16_t* coef2,
                                            uint16_t* qt3x64, uint32_t* status);

#ifdef __cplusplus
}
#endif

#endif
