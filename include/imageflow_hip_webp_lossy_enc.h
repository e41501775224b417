/* imageflow_hip_webp_lossy_enc.h -- the device lossy WebP coder (csrc/vp8_encode.hip): BGRA / BGRX frames in HBM -> complete
 * lossy WebP files in HBM, for EncoderPreset::WebPLossy (codecs/webp.rs: WebPEncodeBGRA / WebPEncodeBGR).
 *
 * Why a header of its own: tests/test_gpu_stream_order.py compares every declaration of imageflow_hip.h that takes a
 * `void* hip_stream` with the rows of its table, and this entry point's proof of stream order lives in a file of its own
 * (tests/test_gpu_webp_lossy_stream_order_encode.py, built on the same tests/stream_order.py).  Plain C99; includes
 * imageflow_hip.h and is included by nothing.
 *
 * The contract is not libwebp's bytes: a file equals the CPU emulation's byte for byte (tests/vp8_encode_emulate.cpp, built
 * from the same csrc/vp8_encode_core.hpp), and libwebp decodes it to exactly the pixels the coder reconstructed.  One VP8 key
 * frame: profile 0, no segments, 16x16 luma modes (and the sixteen 4x4 modes of a macroblock where a stage is created with
 * IFHIP_VP8_ENC_INTRA4; csrc/vp8_encode_intra4.hip), the normal loop filter, the largest power of two <= min(8, macroblock
 * rows) token partitions; the quantiser index follows `quality` (clamped to 0..100) by libwebp's QualityToCompression curve.
 * A frame whose alpha is meaningful and somewhere below 255 gets `VP8X` + `ALPH` (the plane coded by the lossless coder,
 * header byte 0x01); every other frame is a simple `RIFF` / `VP8 ` file. */
#ifndef IMAGEFLOW_HIP_WEBP_LOSSY_ENC_H
#define IMAGEFLOW_HIP_WEBP_LOSSY_ENC_H

#include "imageflow_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define IFHIP_VP8_ENC_FILE_OVERFLOW 1
typedef struct ifhip_webp_lossy_enc_stage ifhip_webp_lossy_enc_stage;
/* refused: zero dimensions, a width or a height above 16383 (the frame header's 14 bits), max_images outside 1..65535.
 * The stage owns an ifhip_webp_enc_stage for the alpha planes when alpha_meaningful, and its scratch (allocated by the first
 * batch); it is bound to ONE stream at a time. */
IFHIP_API int ifhip_webp_lossy_enc_stage_create(ifhip_webp_lossy_enc_stage** stage, uint32_t width, uint32_t height,
                                                int alpha_meaningful, uint32_t max_images);
/* The same with flags.  IFHIP_VP8_ENC_INTRA4: per macroblock the coder also tries the sixteen 4x4 luma sub-blocks with the ten
 * modes each and codes the macroblock as B_PRED where that is cheaper than the best 16x16 mode; everything else of the file is
 * as without the flag, and flags 0 is ifhip_webp_lossy_enc_stage_create to the byte.  Any other flag bit is refused
 * (InvalidArgument).  The stage carries its flags: the batch call's signature is the same, and
 * ifhip_webp_lossy_enc_stage_max_file_bytes answers for them. */
#define IFHIP_VP8_ENC_INTRA4 1u
IFHIP_API int ifhip_webp_lossy_enc_stage_create_flags(ifhip_webp_lossy_enc_stage** stage, uint32_t width, uint32_t height,
                                                      int alpha_meaningful, uint32_t max_images, uint32_t flags);
IFHIP_API void ifhip_webp_lossy_enc_stage_destroy(ifhip_webp_lossy_enc_stage* stage);
/* a file_pitch with which no file overflows, by arithmetic over the coder's choices (csrc/vp8_encode_core.hpp
 * vp8e_max_file_bytes).  One limit is the format's own: the frame tag holds the first partition's size in 19 bits, which the
 * modes of more than about 230 000 macroblocks can outgrow; such a file gets IFHIP_VP8_ENC_FILE_OVERFLOW.  With
 * IFHIP_VP8_ENC_INTRA4 a B_PRED macroblock carries sixteen sub-modes: the bound allows 32 bytes of modes a macroblock and is
 * capped at the limit from 16 313 macroblocks on (2 040 x 2 040 pixels); files of photo-like content (4.4 bytes a B_PRED
 * macroblock) reach the limit itself at about 120 000 macroblocks. */
IFHIP_API size_t ifhip_webp_lossy_enc_stage_max_file_bytes(const ifhip_webp_lossy_enc_stage* stage);
/* n_images frames of the stage's geometry at d_images + i * image_bytes (rows of `stride` bytes; the frame checks of every
 * batch entry, made before the device is asked for).  Image i's file goes to d_files + i * file_pitch, its length to
 * d_lengths[i] -- 0 when the file is longer than file_pitch, with IFHIP_VP8_ENC_FILE_OVERFLOW in d_status[i] (nullable) and
 * nothing of that file written; its neighbours are untouched.  Otherwise all of the image's file_pitch bytes are written
 * (zeros behind the file) and none beyond them; file_pitch may be any size from 32 bytes on.
 * Asynchronous on hip_stream, no host round trip.  The same pixels give the same bytes on every run and in every batch position. */
IFHIP_API int ifhip_webp_lossy_encode_batch_device(ifhip_webp_lossy_enc_stage* stage, const uint8_t* d_images, size_t image_bytes,
                                                   uint32_t stride, uint32_t n_images, float quality, uint8_t* d_files,
                                                   size_t file_pitch, uint32_t* d_lengths, uint32_t* d_status, void* hip_stream);
/* The synchronous host-buffer drop-in for WebPEncodeBGRA / WebPEncodeBGR: one frame.  out == NULL: only *len (the size needed)
 * is written. */
IFHIP_API int ifhip_webp_lossy_encode(const uint8_t* bgra, uint32_t width, uint32_t height, uint32_t stride, int alpha_meaningful,
                                      float quality, uint8_t* out, size_t capacity, size_t* len);
/* the drop-in with the stage's flags (IFHIP_VP8_ENC_INTRA4) */
IFHIP_API int ifhip_webp_lossy_encode_flags(const uint8_t* bgra, uint32_t width, uint32_t height, uint32_t stride, int alpha_meaningful,
                                            float quality, uint32_t flags, uint8_t* out, size_t capacity, size_t* len);

#ifdef __cplusplus
}
#endif

#endif
