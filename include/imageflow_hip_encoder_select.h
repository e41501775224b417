/* imageflow_hip_encoder_select.h -- which coder an `encode` node's presets `auto` and `format` come to, callable on its own
 * (csrc/encoder_select.cpp: no GPU, no context): the reference's encoder selection (imageflow_core/src/codecs/auto.rs:368-1242,
 * built with `c-codecs` and without `zen-codecs`: no jxl, avif, animated webp or jpegli) and the preset its querystring layer
 * makes of the output keys (imageflow_riapi/src/ir4/encoder.rs:5-98).  Jobs run the same code where the context's switch is on
 * (ifhip_shim_context_set_encoder_selection, imageflow_abi_subset.h).
 *
 * Why a header of its own: tests count the declarations of imageflow_hip.h against bindings/hip_interop.rs and against the
 * stream-order table; these two entry points take no stream and have their own bindings file
 * (bindings/hip_interop_encoder_select.rs).  Plain C99; includes imageflow_abi_subset.h and is included by nothing.
 *
 * One deliberate difference from the reference: its interpolate_value (auto.rs:696-702) panics when b - a <= 0, which is the
 * case for every interpolated quality profile outside 55 < percent < 73 and for most quality_profile_dpr values; this library
 * evaluates a + ratio * (b - a) without the guard.  On the table's own rows, inside (55, 73) and inside its counterpart on the
 * ssim2 axis (60, 70) the values are the reference's. */
#ifndef IMAGEFLOW_HIP_ENCODER_SELECT_H
#define IMAGEFLOW_HIP_ENCODER_SELECT_H

#include "imageflow_abi_subset.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Both return 0; 2 for a querystring key or value this library refuses (ActionNotSupported); 3 for an argument that means
 * nothing (InvalidArgument -- "No formats enabled; try 'allow': { 'web_safe':true}" is one); 4 for a preset serde would not
 * read (InvalidJson: a missing required field, a wrong type, an unknown variant).  The text is where
 * ifhip_last_error_message() finds it.  The JSON and its length with the terminating 0 go to out / *needed; the text is copied
 * only when cap is large enough (out may be NULL with cap 0). */
#define IFHIP_SELECT_OK 0
#define IFHIP_SELECT_REFUSED 2
#define IFHIP_SELECT_INVALID 3
#define IFHIP_SELECT_INVALID_JSON 4

/* The job's source (in a job: its first decode node), as get_unscaled_unrotated_image_info describes it to build_auto_encoder_details
 * (auto.rs:1059-1079).  NONE: no decoder, or this library's raw BGRA container -- `keep` then falls through to auto-selection. */
#define IFHIP_SELECT_SOURCE_NONE 0
#define IFHIP_SELECT_SOURCE_JPEG 1
#define IFHIP_SELECT_SOURCE_PNG 2   /* source_lossless: the file is not a palette PNG (libpng_decoder.rs:49) */
#define IFHIP_SELECT_SOURCE_GIF 3   /* source_frames above 1: animated */
#define IFHIP_SELECT_SOURCE_WEBP 4  /* source_lossless: the file has a VP8L image chunk */

/* The EncoderPreset a querystring comes to (calculate_encoder_preset with read_allowed_formats and read_encoder_hints):
 * {"auto": {quality_profile, quality_profile_dpr, matte, lossless, allow}} for format=auto (and for a `qp` without a format), else
 * {"format": {format, quality_profile, quality_profile_dpr, matte, lossless, allow, encoder_hints}}; serde's field names and order,
 * None as null.  `quality` without `qp` becomes the profile {"percent": quality} only under format=auto.  The whole string is
 * parsed as command_string parses it with the switch on: a key that stays refused there is refused here. */
IMAGEFLOW_SHIM_API int ifhip_shim_querystring_encoder_preset(const char *value, char *out, size_t cap, size_t *needed);

/* The resolution of {"auto": ..} / {"format": ..} (len bytes of JSON) for a source and a final frame of w x h:
 * {"format": "jpeg" | "png" | "webp" | "gif", "coder": "mozjpeg" | "libjpeg_turbo" | "lodepng" | "pngquant" | "libpng" | "webp_lossy" |
 * "webp_lossless" | "gif", "params": {..}, "matte": colour | null}.  params holds the fields of the named preset of that coder:
 * mozjpeg {quality, progressive, matte}; libjpeg_turbo {quality, progressive, optimize_huffman_coding, matte}; lodepng
 * {maximum_deflate}; pngquant {quality, minimum_quality, speed, maximum_deflate}; libpng {depth, matte, zlib_compression};
 * webp_lossy {quality}; webp_lossless and gif {}. */
IMAGEFLOW_SHIM_API int ifhip_shim_resolve_encoder_preset(const char *preset_json, size_t len, int source_kind, int source_lossless,
                                                         uint32_t source_frames, int alpha_meaningful, uint32_t w, uint32_t h, char *out,
                                                         size_t cap, size_t *needed);

#ifdef __cplusplus
}
#endif

#endif
