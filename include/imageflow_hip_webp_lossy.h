/* imageflow_hip_webp_lossy.h -- the batch entry of the device lossy WebP decoder (csrc/vp8_decode.hip).
 *
 * Why a header of its own: tests/test_gpu_stream_order.py compares every declaration of imageflow_hip.h that takes a
 * `void* hip_stream` with the rows of its table, and this entry point's proof of stream order lives in a file of its own
 * (tests/test_gpu_webp_lossy_stream_order.py, built on the same tests/stream_order.py).  The declaration is folded into
 * imageflow_hip.h when that table gains its row.  Plain C99; includes imageflow_hip.h and is included by nothing.
 * The status words (IFHIP_VP8_DEC_*) and the host-buffer drop-in ifhip_webp_lossy_decode are in imageflow_hip.h. */
#ifndef IMAGEFLOW_HIP_WEBP_LOSSY_H
#define IMAGEFLOW_HIP_WEBP_LOSSY_H

#include "imageflow_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* n files (host memory), each with its own size, partitions and alpha coding, into n device frames: d_frames[i] holds height_i
 * rows of strides[i] bytes inside frame_bytes[i]; only the 4 * width_i bytes of a row are written.  d_status[i] (device)
 * receives the file's status word; a damaged file leaves its frame untouched and never disturbs its neighbours; a lossless
 * file (IFHIP_VP8_DEC_NOT_LOSSY) and one whose container does not parse need no frame.  A fixed number of launches per batch,
 * every file in each: residuals, prediction, loop filter, alpha plane, conversion -- and the VP8L reader's for the files
 * whose ALPH plane is VP8L-coded.  The records are uploaded before the call returns; the kernels are asynchronous on
 * hip_stream.  ICCP chunks are NOT acted on here (see ifhip_webp_info's color_kind).  Argument and frame checks come before
 * the device check. */
IFHIP_API int ifhip_webp_lossy_decode_batch_device(const uint8_t* const* files, const size_t* lens, uint32_t n_files,
                                                   uint8_t* const* d_frames, const size_t* frame_bytes, const uint32_t* strides,
                                                   uint32_t* d_status, void* hip_stream);

#ifdef __cplusplus
}
#endif

#endif
