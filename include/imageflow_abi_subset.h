/*
 * imageflow_abi_subset.h -- libimageflow's C ABI v3.2 as libimageflow_hip.so re-exports it: all 25 functions of
 * bindings/headers/imageflow_default.h, so that a C caller (or any language binding generated from that header) can run
 * resize jobs on the MI355X path without the Rust host.  Same names, argument order and ownership rules as the
 * reference: imageflow_abi/src/lib.rs (line numbers per function below), ABI version imageflow_abi/src/abi_version.rs:4,7.
 * "Subset" is what a JOB may contain, not the function list.
 *
 * Endpoints of imageflow_context_send_json: v1/build, v1/execute, v1/get_image_info, v1/tell_decoder (+ v0.1/ aliases),
 * v1/get_scaled_image_info, v1/get_version_info; everything else answers 404 as json/mod.rs:158-168.
 *
 * What a job may contain (anything else answers ActionNotSupported, HTTP 400): decode (baseline JPEG, or the raw
 * BGRA container EXTENSION), create_canvas, fill_rect, expand_canvas, crop, flip_h/flip_v, transpose, rotate_90/180/270,
 * apply_orientation, color_matrix_srgb, color_filter_srgb, resample_2d, draw_image_exact and copy_rect_to_canvas (graph
 * form, with a `canvas` edge), watermark (all five fit modes), constrain (all nine modes, gravity, canvas_color),
 * command_string (ir4: width/height, mode=max), encode.
 * `encode` with the libjpeg_turbo preset writes a real JPEG (quality, matte, progressive, optimize_huffman_coding:
 * byte-identical to libjpeg-turbo's file for the same pixels at 4:2:0); every other preset writes the raw BGRA container
 * EXTENSION (this library has no deflate / GIF / WebP coder): 8 bytes "IFBGRA1\0", u32le w, h, stride,
 * alpha_meaningful, then h rows of `stride` bytes.
 * Implementation: imageflow_amd/csrc/abi_shim.cpp (these entry points) and, for the jobs, shim_job.hpp with
 * shim_interp.cpp, shim_decode.cpp, shim_nodes.cpp and shim_encode.cpp beside it.
 */
#ifndef IMAGEFLOW_ABI_SUBSET_H
#define IMAGEFLOW_ABI_SUBSET_H

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#define IMAGEFLOW_ABI_VER_MAJOR 3
#define IMAGEFLOW_ABI_VER_MINOR 2
#define IMAGEFLOW_SHIM_API __attribute__((visibility("default")))

struct imageflow_context;
struct imageflow_json_response;

/* imageflow_abi/src/lib.rs:281-288 */
typedef enum imageflow_lifetime {
  imageflow_lifetime_lifetime_outlives_function_call = 0,
  imageflow_lifetime_lifetime_outlives_context = 1,
} imageflow_lifetime;

#ifdef __cplusplus
extern "C" {
#endif

IMAGEFLOW_SHIM_API bool imageflow_abi_compatible(uint32_t imageflow_abi_ver_major, uint32_t imageflow_abi_ver_minor);  /* :389 */
IMAGEFLOW_SHIM_API uint32_t imageflow_abi_version_major(void);                                                         /* :398 */
IMAGEFLOW_SHIM_API uint32_t imageflow_abi_version_minor(void);                                                         /* :403 */

IMAGEFLOW_SHIM_API struct imageflow_context *imageflow_context_create(uint32_t imageflow_abi_ver_major,
                                                                      uint32_t imageflow_abi_ver_minor);                /* :430 */
IMAGEFLOW_SHIM_API bool imageflow_context_begin_terminate(struct imageflow_context *context);                          /* :459 */
IMAGEFLOW_SHIM_API void imageflow_context_destroy(struct imageflow_context *context);                                  /* :492 */

IMAGEFLOW_SHIM_API bool imageflow_context_has_error(struct imageflow_context *context);                                /* :530 */
IMAGEFLOW_SHIM_API bool imageflow_context_error_recoverable(struct imageflow_context *context);                        /* :549 */
IMAGEFLOW_SHIM_API bool imageflow_context_error_try_clear(struct imageflow_context *context);                          /* :572 */
IMAGEFLOW_SHIM_API int32_t imageflow_context_error_code(struct imageflow_context *context);                            /* :600 */
IMAGEFLOW_SHIM_API int32_t imageflow_context_error_as_exit_code(struct imageflow_context *context);                    /* :620 */
IMAGEFLOW_SHIM_API int32_t imageflow_context_error_as_http_code(struct imageflow_context *context);                    /* :645 */
IMAGEFLOW_SHIM_API bool imageflow_context_error_write_to_buffer(struct imageflow_context *context, char *buffer,
                                                                size_t buffer_length, size_t *bytes_written);          /* :684 */
/* prints the error and calls exit(imageflow_context_error_as_exit_code) -- does not return when there is one */
IMAGEFLOW_SHIM_API bool imageflow_context_print_and_exit_if_error(struct imageflow_context *context);                  /* :744 */
/* the one call made from another thread while a job runs: sets the flag the job polls before every node, at every frame
 * allocation and inside decode / encode; the job then fails with category 21 (HTTP 499, exit 130) */
IMAGEFLOW_SHIM_API void imageflow_context_request_cancellation(struct imageflow_context *context);                     /* :878 */

IMAGEFLOW_SHIM_API const struct imageflow_json_response *imageflow_context_send_json(struct imageflow_context *context,
                                                                                     const char *method,
                                                                                     const uint8_t *json_buffer,
                                                                                     size_t json_buffer_size);         /* :944 */
IMAGEFLOW_SHIM_API bool imageflow_json_response_read(struct imageflow_context *context,
                                                     const struct imageflow_json_response *response_in,
                                                     int64_t *status_as_http_code_out,
                                                     const uint8_t **buffer_utf8_no_nulls_out,
                                                     size_t *buffer_size_out);                                         /* :783 */
IMAGEFLOW_SHIM_API bool imageflow_json_response_destroy(struct imageflow_context *context,
                                                        struct imageflow_json_response *response);                     /* :842 */

IMAGEFLOW_SHIM_API bool imageflow_context_add_input_buffer(struct imageflow_context *context, int32_t io_id,
                                                           const uint8_t *buffer, size_t buffer_byte_count,
                                                           imageflow_lifetime lifetime);                               /* :1137 */
IMAGEFLOW_SHIM_API bool imageflow_context_add_output_buffer(struct imageflow_context *context, int32_t io_id);         /* :1224 */
IMAGEFLOW_SHIM_API bool imageflow_context_get_output_buffer_by_id(struct imageflow_context *context, int32_t io_id,
                                                                  const uint8_t **result_buffer,
                                                                  size_t *result_buffer_length);                       /* :1272 */

/* ownership of the output bytes moves to the caller; refused once get_output_buffer_by_id lent a pointer, or twice */
IMAGEFLOW_SHIM_API bool imageflow_context_take_output_buffer(struct imageflow_context *context, int32_t io_id,
                                                             uint8_t **result_buffer, size_t *result_buffer_length);   /* :1335 */
IMAGEFLOW_SHIM_API bool imageflow_buffer_free(uint8_t *buffer, size_t length);                                         /* :1385 */

IMAGEFLOW_SHIM_API void *imageflow_context_memory_allocate(struct imageflow_context *context, size_t bytes,
                                                           const char *filename, int32_t line);                        /* :1424 */
IMAGEFLOW_SHIM_API bool imageflow_context_memory_free(struct imageflow_context *context, void *pointer,
                                                      const char *filename, int32_t line);                             /* :1484 */

/* Not part of libimageflow's header: the poll countdown debug builds of the reference carry for their own cancellation
 * test (Context::request_cancellation_after_n_polls, imageflow_core/src/context.rs:96-104,167-172). */
IMAGEFLOW_SHIM_API void ifhip_shim_request_cancellation_after_n_polls(struct imageflow_context *context, int64_t polls);
IMAGEFLOW_SHIM_API int64_t ifhip_shim_cancellation_polls_remaining(struct imageflow_context *context);
/* Diagnostic: how many decode -> resample pairs of this context's jobs ran as ONE device call without a decoded bitmap in
 * HBM (ifhip_jpeg_decode_resample_batch_device reporting fused = 1). */
IMAGEFLOW_SHIM_API int64_t ifhip_shim_fused_decode_resamples(struct imageflow_context *context);
/* Diagnostic: how many JPEG outputs of this context's jobs were entropy-coded on the device (libjpeg_turbo preset without
 * progressive / optimize_huffman_coding: ifhip_jpeg_encode_batch_device; with them only after
 * ifhip_shim_context_set_device_jpeg_options; only the file is downloaded). */
IMAGEFLOW_SHIM_API int64_t ifhip_shim_device_coded_files(struct imageflow_context *context);
/* Diagnostic: how many decodes of this context's jobs shared their entropy-decode device call with the job of another
 * thread (concurrent decodes of one geometry are coalesced into one batch; one context per thread, lib.rs:20-27). */
IMAGEFLOW_SHIM_API int64_t ifhip_shim_coalesced_decodes(struct imageflow_context *context);
/* Independent jobs over the GPUs of one node, without a process per GPU: a context may be bound to a device ordinal and
 * every job it runs (whichever thread calls) runs there -- the reference's "one Context per thread"
 * (imageflow_abi/src/lib.rs:20-27) then shards a batch of jobs by construction, with no collective (outputs are host
 * buffers).  ifhip_shim_spread_contexts(1): contexts created from now on take the usable devices round-robin;
 * _context_set_device binds one context (-1: follow the calling thread's current device, the default). */
IMAGEFLOW_SHIM_API void ifhip_shim_spread_contexts(int enable);
IMAGEFLOW_SHIM_API bool ifhip_shim_context_set_device(struct imageflow_context *context, int ordinal);
IMAGEFLOW_SHIM_API int ifhip_shim_context_device(struct imageflow_context *context);
/* EXTENSION.  Colour management, off by default: with on != 0 every input of the context's jobs whose ICC profile (JPEG
 * APP2, PNG iCCP, WebP ICCP) or PNG gAMA + cHRM is not sRGB is converted to sRGB on the device right behind its decode, as
 * the reference does in codecs/cms.rs::transform_to_srgb (mozjpeg_decoder.rs:409, libpng_decoder.rs:376, webp.rs), pinned
 * to its lcms2 back end -- instead of the ActionNotSupported refusal such inputs get otherwise.  Jobs written for the
 * reference run unmodified.  The decoder command "convert_color_profile" (decode.commands, v1/tell_decoder) does the same
 * for one input; "discard_color_profile" wins over both.  Converted: RGB matrix/TRC profiles (v2 / v4, XYZ PCS) and gAMA +
 * cHRM.  Still refused, naming the case: GRAY / CMYK spaces, a Lab PCS, LUT-based profiles.  A malformed profile is a
 * ColorProfileError (ImageMalformed) unless the decoder was told "ignore_color_profile_errors".  Returns true. */
IMAGEFLOW_SHIM_API bool ifhip_shim_context_set_color_management(struct imageflow_context *context, int on);
/* EXTENSION.  The profile kinds colour management converts beyond the above, 0 by default: IFHIP_COLOR_KIND_GRAY -- a GRAY
 * profile (kTRC, XYZ PCS) on a grey frame (a one-component JPEG, PNG colour types 0 and 4), the reference's
 * SourceProfile::IccProfileGray; IFHIP_COLOR_KIND_LUT -- an RGB profile that carries A2B0 (lut8 / lut16 with an XYZ PCS, lutAToB
 * with an XYZ or Lab PCS).  Both go through a colour link (include/imageflow_hip_color_link.h), built once per profile and
 * context.  The flags act only where colour management already acts for that input (the switch above, or the decoder command
 * "convert_color_profile"); "discard_color_profile" wins as before.  With a flag set, a profile of that kind that is still not
 * converted keeps the ActionNotSupported refusal, which names the case (perceptual intent and A2B0 only; no grey LUTs; lut8 /
 * lut16 with a Lab PCS; CMYK); a malformed one is a ColorProfileError unless the decoder was told
 * "ignore_color_profile_errors".  Returns false for an unknown bit.
 * ifhip_shim_color_links_built: how many links this context's jobs built from profile bytes (diagnostic: a profile met again
 * is served from the context's cache of a handful of links). */
#define IFHIP_COLOR_KIND_GRAY 1u
#define IFHIP_COLOR_KIND_LUT 2u
IMAGEFLOW_SHIM_API bool ifhip_shim_context_set_color_profile_kinds(struct imageflow_context *context, uint32_t flags);
IMAGEFLOW_SHIM_API int64_t ifhip_shim_color_links_built(struct imageflow_context *context);
/* EXTENSION: lossy WebP inputs -- a still `VP8 ` chunk, with or without an `ALPH` chunk -- are decoded on the device, to
 * exactly what WebPDecode(MODE_BGRA) gives with libwebp's default options (csrc/vp8_read.cpp, csrc/vp8_decode.hip): `decode`,
 * `watermark`, `command_string` and v1/get_image_info then take such a file (bgra_32 where it has alpha, else bgr_32).  Off by
 * default, where a lossy file stays ImageTypeNotSupported.  max_decode_size, the ICCP policy, webp_decoder_hints and EXIF
 * are treated as for a lossless file; animated WebP and libwebp's decode-time rescaler stay refused.  Returns true. */
IMAGEFLOW_SHIM_API bool ifhip_shim_context_set_webp_lossy_decoder(struct imageflow_context *context, int on);
/* EXTENSION: progressive (SOF2) JPEG inputs are entropy-decoded on the device (include/imageflow_hip_jpeg_progressive.h: the
 * file is prepared on the job's thread, uploaded once, and its coefficient planes never leave HBM) in `decode`, `watermark` and
 * `command_string`.  Off by default, where such files are decoded by the host reader and every job is byte for byte what it
 * was.  With it on a job's outputs are the same bytes: a file the front end refuses (a sequential multi-scan file, a
 * progression libjpeg decodes with a warning) or whose status word is not 0 (damaged entropy data) goes to the host reader
 * exactly as with the switch off, and that reader's answer -- planes or error -- stands.  Downscale hints, EXIF, the ICC
 * policy, cancellation and the `performance` block are unchanged.  Returns true.
 * ifhip_shim_device_progressive_decodes: how many decodes of this context's jobs took the device path; *fell_back (may be
 * NULL): how many were sent back to the host reader.  Both stay 0 with the switch off. */
IMAGEFLOW_SHIM_API bool ifhip_shim_context_set_device_progressive_decoder(struct imageflow_context *context, int on);
IMAGEFLOW_SHIM_API int64_t ifhip_shim_device_progressive_decodes(struct imageflow_context *context, int64_t *fell_back);
/* EXTENSION: `encode` with the preset {"webplossy": {"quality": q}} writes a lossy WebP file on the device
 * (ifhip_webp_lossy_encode_batch_device: WebPEncoder::write_frame over WebPEncodeBGRA / WebPEncodeBGR, codecs/webp.rs) and reports
 * image/webp; off by default, where the preset writes the raw BGRA container as ever.  With it on, the bare string "webplossy" and a
 * missing or non-numeric quality are InvalidJson before any node runs (the reference's variant is a struct with a required f32), and
 * a side above 16383 is "ImageEncodingError: libwebp encoding error".  `on`: 0 off; 2 on with the sixteen 4x4 luma modes
 * (IFHIP_VP8_ENC_INTRA4 of imageflow_hip_webp_lossy_enc.h: smaller files of textured frames, a longer serial chain); any other
 * value on as ever.  Returns true. */
IMAGEFLOW_SHIM_API bool ifhip_shim_context_set_webp_lossy_encoder(struct imageflow_context *context, int on);
/* EXTENSION: the stage flags of the "webplossless" preset's device coder (ifhip_webp_enc_stage_create_flags of imageflow_hip.h), in
 * steps and graphs alike; 0 by default.  IFHIP_WEBP_ENC_COLOR_INDEXING: a frame of at most 256 colours is written with a colour
 * table where that is the smaller file; no file grows, and the pixels are the same.  Returns false, and changes nothing, for
 * a bit the coder does not know.  The lossy coder's alpha planes are not concerned. */
IMAGEFLOW_SHIM_API bool ifhip_shim_context_set_webp_lossless_flags(struct imageflow_context *context, uint32_t flags);
/* EXTENSION: `encode` with the preset "gif" writes a GIF89a file on the device (ifhip_gif_encode_batch_device: GifEncoder::write_frame,
 * codecs/gif/mod.rs:385-592) and reports image/gif; off by default, where the preset writes the raw BGRA container as ever.  A
 * GIF input of the job hands its loop count and the selected frame's delay and user-input flag to the file. */
IMAGEFLOW_SHIM_API bool ifhip_shim_context_set_gif_encoder(struct imageflow_context *context, int on);
/* EXTENSION: animated GIFs pass through jobs, as the reference re-runs a job for every frame (GifDecoder::has_more_frames /
 * ctx.set_more_frames, codecs/gif/mod.rs:207-305; GifEncoder::write_frame with its frame_ix, :429-521).  Off by default.  The
 * path applies only where this switch AND the GIF encoder are on, a `decode` node reads a GIF of more than one frame with
 * no select_frame told to it, and an `encode` node with the "gif" preset lies downstream of it: the source's screens are
 * decoded once (ifhip_gif_decode_frames_device), the framewise job runs once per frame, every "gif" encode node collects
 * its frames on the device and codes them in ONE call behind the last (ifhip_gif_encode_animation_device: frame k's delay
 * and user-input flag are the source frame's).  Every other encoder takes frame 0 and writes once; watermarks and a
 * command_string's own decode do not animate.  Several animated decodes must agree on the frame count (InvalidOperation);
 * the decoded screens and the collected frames together may hold security.max_total_file_pixels pixels at the most (the
 * reference's check_total_pixels, codecs/gif/mod.rs:103-118; default 400 000 000, imageflow_types/src/lib.rs:1212-1235): a job
 * over it is refused as SizeLimitExceeded before anything is allocated.  Every other job is byte for byte what it is with
 * the switch off.  (With ifhip_shim_context_set_encoder_selection on, an `auto` / `format` encode that comes to GIF counts as
 * a "gif" node, with or without the GIF encoder's switch.) */
IMAGEFLOW_SHIM_API bool ifhip_shim_context_set_gif_animation(struct imageflow_context *context, int on);
/* EXTENSION.  Device coding of the libjpeg_turbo preset's options, off by default: with on != 0 an encode with
 * "progressive" and / or "optimize_huffman_coding" is entropy-coded on the device (ifhip_jpeg_encode_flags_batch_device:
 * only the file is downloaded, not the coefficient planes) -- first with room for streams half the size of the
 * coefficients, then with the geometry's worst case; the host writer codes the file when a stage cannot be made or the
 * geometry is refused.  The files are byte-identical either way; ifhip_shim_device_coded_files counts those coded on the
 * device.  Off, such encodes go to the host writer as before.  Returns true. */
IMAGEFLOW_SHIM_API bool ifhip_shim_context_set_device_jpeg_options(struct imageflow_context *context, int on);
/* EXTENSION.  Encoder selection, off by default: with on != 0 an `encode` whose preset is {"auto": ..} or {"format": ..} is
 * resolved as the reference resolves it (codecs/auto.rs: build_auto_encoder_details, format_auto_select, create_encoder_auto,
 * with its quality tables) against the job's source (the first decode of its steps, or the decode node of the lowest id) and the final frame, and written as a real file by the
 * coder that comes out: mozjpeg, libjpeg_turbo, libpng, pngquant, lodepng (a truecolour PNG of the device PNG coder, RGBA
 * where the frame's alpha is meaningful), webp_lossless, webp_lossy (with the 4x4 modes where the lossy WebP encoder's switch
 * has the value 2) or gif -- whatever the GIF and lossy WebP encoder switches say, whose named presets keep their meaning.
 * The preset's matte is applied before every coder (on a private copy of a shared frame); the record carries the resolved
 * format's mime type and extension.  A preset serde would not read is InvalidJson before the first node runs.
 * `command_string` then reads the output keys of its querystring (format / thumbnail, qp, qp.dpr / qp.dppx, lossless, accept.*,
 * quality, jpeg.*, webp.*, png.*) with the reference's parsers and encodes through the preset they make
 * (ifhip_shim_querystring_encoder_preset, imageflow_hip_encoder_select.h); a string without an output key keeps the source's
 * format.  With ifhip_shim_context_set_gif_animation on as well, an auto / format encode that comes to GIF collects the frames
 * of an animated source as a "gif" encode node does.  Differences from the reference: imageflow_hip_encoder_select.h and
 * DESIGN "Encoder selection".  Off, every job is byte for byte what it was.  Returns true. */
IMAGEFLOW_SHIM_API bool ifhip_shim_context_set_encoder_selection(struct imageflow_context *context, int on);

/* The layout arithmetic behind the `constrain` and `watermark` nodes, callable on its own (no GPU, no context):
 * imageflow_riapi::ir4::process_constraint (imageflow_riapi/src/ir4/layout.rs:334-412) for a source of source_w x source_h
 * and a Constraint {mode, w, h, gravity}.  mode: "distort" | "within" | "fit" | "larger_than" | "within_crop" | "fit_crop" |
 * "aspect_crop" | "within_pad" | "fit_pad"; w / h < 0: not given; has_gravity 0: centre.  Out: crop_x1y1x2y2[4] (valid when
 * bit 0 of *flags), scale_to_wh[2], pad_ltrb[4] (valid when bit 1 of *flags), canvas_wh[2].  Returns 0, 1 for a LayoutError
 * (the reference's Err), 2 for an unknown mode or a null pointer. */
IMAGEFLOW_SHIM_API int ifhip_shim_process_constraint(const char *mode, int32_t source_w, int32_t source_h, int64_t w, int64_t h,
                                                     int has_gravity, float gravity_x, float gravity_y,
                                                     uint32_t *crop_x1y1x2y2, int32_t *scale_to_wh, uint32_t *pad_ltrb,
                                                     int32_t *canvas_wh, int *flags);

/* What `command_string` {kind: "ir4", value} expands to, callable on its own (no GPU, no context): the querystring is parsed
 * (imageflow_riapi Instructions) and laid out for a frame of source_w x source_h decoded from an image of reference_w x
 * reference_h (the two differ after a reduced JPEG decode), as Ir4Layout::add_steps and Ir4Expand::get_decode_commands do.
 * watermarks_json: the JSON text of command_string.watermarks (an array), or NULL.  Writes
 * {"decoder_commands": [...], "steps": [...], "canvas": [w, h]} -- the steps in the JSON form v1/execute takes, without decode
 * and encode -- and its length with the terminating 0 to *needed; the text is copied only when cap is large enough (out may be
 * NULL with cap 0).  Returns 0; 1 for a layout error (the reference's Err); 2 for a key or value this library refuses
 * (ActionNotSupported); 3 for an argument no querystring of the reference's could mean.  For 1, 2 and 3 the text is where
 * ifhip_last_error_message() finds it.  command_string itself runs this expansion. */
IMAGEFLOW_SHIM_API int ifhip_shim_expand_command_string(const char *value, int32_t source_w, int32_t source_h, int32_t reference_w,
                                                        int32_t reference_h, const char *watermarks_json, char *out, size_t cap,
                                                        size_t *needed);

#ifdef __cplusplus
}
#endif
#endif /* IMAGEFLOW_ABI_SUBSET_H */
