/* imageflow_hip_color_link.h -- GRAY and LUT-based ICC profiles converted to sRGB on the device (csrc/color_link.cpp,
 * csrc/color_link_core.hpp, csrc/color_link.hip): what codecs/lcms2_transform.rs does for SourceProfile::IccProfileGray
 * (:132-186) and for an IccProfile that carries A2B0 (:82-84, :117-130), pinned to lcms2's 8-bit transform.
 *
 * Why a header of its own: tests/test_gpu_stream_order.py compares every declaration of imageflow_hip.h that takes a
 * `void* hip_stream` with the rows of its table, and the batch entry's proof of stream order lives in
 * tests/test_gpu_color_link.py (built on the same tests/stream_order.py).  Plain C99; includes imageflow_hip.h and is
 * included by nothing.
 *
 * A link is built on the host from the profile's bytes and is one of
 *   a grey table   256 bytes: a grey frame's sample -> the sRGB byte written to B, G and R (GRAY space, kTRC, XYZ PCS)
 *   an RGB link    33 x 33 x 33 nodes of 3 x 16 bits: the profile's A2B0 (mft1, mft2 or mAB; XYZ or Lab PCS) -> PCS ->
 *                  lcms2's built-in sRGB, perceptual intent with lcms2's black point compensation, sampled at the uniform
 *                  grid and interpolated tetrahedrally per pixel in integers, as lcms2's optimiser does for 8-bit pixels
 * ifhip_color_plan_from_icc keeps answering NOT_CONVERTIBLE for these profiles; a matrix/TRC profile is not a link. */
#ifndef IMAGEFLOW_HIP_COLOR_LINK_H
#define IMAGEFLOW_HIP_COLOR_LINK_H

#include "imageflow_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ifhip_color_link ifhip_color_link;

#define IFHIP_COLOR_LINK_GRAY 1 /* 256 bytes                                   */
#define IFHIP_COLOR_LINK_RGB 2  /* 33 * 33 * 33 nodes of R, G, B as uint16     */
#define IFHIP_COLOR_LINK_GRID 33u

/* Host only, every read bounds-checked against `len`.  frame_is_gray: the decoded frame came from one grey channel (a
 * one-component JPEG, PNG colour types 0 and 4); a GRAY profile is convertible only then, an RGB profile either way.
 * Returns an ifhip_color_plan_status; PLANNED: *link owns a new link (ifhip_color_link_free).  Otherwise *link is NULL and
 * ifhip_last_error_message() names the case. */
IFHIP_API int ifhip_color_link_from_icc(const uint8_t* icc, size_t len, int frame_is_gray, ifhip_color_link** link);
/* Waits for the device if the link was ever used there.  NULL is accepted. */
IFHIP_API void ifhip_color_link_free(ifhip_color_link* link);
IFHIP_API int ifhip_color_link_kind(const ifhip_color_link* link);
/* The link's contents for tests: 256 bytes, or 33 * 33 * 33 * 3 uint16 (node (r * 33 + g) * 33 + b; R, G, B).  `capacity` in
 * bytes; *written receives the bytes copied. */
IFHIP_API int ifhip_color_link_copy_nodes(const ifhip_color_link* link, void* out, size_t capacity, size_t* written);

/* Host frame, in place, synchronous on the null stream. */
IFHIP_API int ifhip_color_link_transform(uint8_t* bgra, uint32_t w, uint32_t h, uint32_t stride, ifhip_color_link* link);
/* n_images frames of one shape in device memory, in place: one launch, asynchronous and ordered on hip_stream, no host wait.
 * The contract of ifhip_color_transform_batch_device: 4-byte aligned rows, row padding neither read as pixels nor written,
 * the fourth byte of every pixel keeps its value, at most 65535 images.  A grey table reads the B byte alone.  The link's
 * device copy is uploaded once, ordered on the stream of the first call that needs it (later calls on other streams wait
 * for that copy on the device, not on the host), and lives as long as the link. */
IFHIP_API int ifhip_color_link_transform_batch_device(uint8_t* d_bgra, size_t image_bytes, uint32_t n_images, uint32_t w,
                                                      uint32_t h, uint32_t stride, ifhip_color_link* link, void* hip_stream);

#ifdef __cplusplus
}
#endif

#endif
