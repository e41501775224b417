/*
 * imageflow_hip.h -- C ABI of libimageflow_hip.so: the MI355X (gfx950) implementation of imageflow's
 * pixel hot path.  Plain pointers and sizes only; no C++/torch types cross this boundary.
 *
 * Every entry point names the reference interface it replaces (paths relative to the imageflow tree).
 * The Rust side binds these with an `extern "C"` block exactly like imageflow_core/src/ffi/c_interop.rs:115-213
 * binds c_components today (binding source: bindings/hip_interop.rs, generated from this file; call sites: INTEGRATION.md).
 *
 * Conventions (mirroring wrap_jpeg_* in c_components/lib/codec_jpeg_wrapper.c:187-233 and FlowError):
 *   - functions return an ifhip_status (0 = ok); the message of the last failure on the calling thread is
 *     available from ifhip_last_error_message();
 *   - a bitmap is (pointer, w, h, stride-in-bytes), BGRA8, rows padded as graphics/bitmaps.rs:712-740;
 *   - colours are Color32 0xAARRGGBB whose little-endian bytes are B,G,R,A (imageflow_helpers/src/colors.rs:77-117);
 *   - `*_device` variants take pointers into HBM and a hipStream_t (as void*).  Every read and write of such a call is
 *     ordered on that stream: the producer of its inputs may be queued in front of it and the consumer of its outputs behind
 *     it on the same stream, with no host wait in between (tests/test_gpu_stream_order.py holds every entry point to this
 *     with inputs that arrive late).  Most calls enqueue and return.  These wait on the host for what is already queued on
 *     hip_stream: the file decoders ifhip_{png,webp,gif}_decode_batch_device and ifhip_gif_decode_frames_device (the files go
 *     up on hip_stream and the call waits for that copy before its first launch), ifhip_gif_encode_animation_device (its two
 *     host arrays likewise), ifhip_jpeg_entropy_decode_device (it synchronises the stream) and the first call of a JPEG
 *     encode stage at a quality it has not coded yet (the marker segments go up from the stage's one pinned copy, which the
 *     call before may still be sending); DESIGN.md, "Stream contract".
 *     The non-device variants take host memory, are synchronous, and are the drop-in for the Rust callers.
 *   - there is NO CPU fallback: without a usable gfx950 device every compute entry point fails with
 *     IFHIP_GPU_UNAVAILABLE.
 */
#ifndef IMAGEFLOW_HIP_H
#define IMAGEFLOW_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IFHIP_API __attribute__((visibility("default")))

/* Subset of imageflow_core::ErrorKind (errors.rs:158-248) that this path can raise. */
typedef enum ifhip_status {
    IFHIP_OK = 0,
    IFHIP_INVALID_ARGUMENT = 1,        /* ErrorKind::InvalidArgument   (scaling.rs:24-29,40)   */
    IFHIP_METHOD_NOT_IMPLEMENTED = 2,  /* ErrorKind::MethodNotImplemented (scaling.rs:43-48)   */
    IFHIP_INVALID_STATE = 3,           /* ErrorKind::InvalidState      (scaling.rs:145,192)    */
    IFHIP_ALLOCATION_FAILED = 4,       /* ErrorKind::AllocationFailed                           */
    IFHIP_GPU_UNAVAILABLE = 5,         /* no gfx950 device / HIP runtime error                  */
    IFHIP_GPU_ERROR = 6
} ifhip_status;

/* graphics/weights.rs:43-78 -- same discriminants. */
typedef enum ifhip_filter {
    IFHIP_FILTER_ROBIDOUX_FAST = 1, IFHIP_FILTER_ROBIDOUX = 2, IFHIP_FILTER_ROBIDOUX_SHARP = 3,
    IFHIP_FILTER_GINSENG = 4, IFHIP_FILTER_GINSENG_SHARP = 5, IFHIP_FILTER_LANCZOS = 6,
    IFHIP_FILTER_LANCZOS_SHARP = 7, IFHIP_FILTER_LANCZOS2 = 8, IFHIP_FILTER_LANCZOS2_SHARP = 9,
    IFHIP_FILTER_CUBIC_FAST = 10, IFHIP_FILTER_CUBIC = 11, IFHIP_FILTER_CUBIC_SHARP = 12,
    IFHIP_FILTER_CATMULL_ROM = 13, IFHIP_FILTER_MITCHELL = 14, IFHIP_FILTER_CUBIC_B_SPLINE = 15,
    IFHIP_FILTER_HERMITE = 16, IFHIP_FILTER_JINC = 17, IFHIP_FILTER_RAW_LANCZOS3 = 18,
    IFHIP_FILTER_RAW_LANCZOS3_SHARP = 19, IFHIP_FILTER_RAW_LANCZOS2 = 20, IFHIP_FILTER_RAW_LANCZOS2_SHARP = 21,
    IFHIP_FILTER_TRIANGLE = 22, IFHIP_FILTER_LINEAR = 23, IFHIP_FILTER_BOX = 24,
    IFHIP_FILTER_CATMULL_ROM_FAST = 25, IFHIP_FILTER_CATMULL_ROM_FAST_SHARP = 26, IFHIP_FILTER_FASTEST = 27,
    IFHIP_FILTER_MITCHELL_FAST = 28, IFHIP_FILTER_N_CUBIC = 29, IFHIP_FILTER_N_CUBIC_SHARP = 30,
    IFHIP_FILTER_LEGACY_IDCT = 31
} ifhip_filter;

/* graphics/color.rs:4-9 WorkingFloatspace (Gamma is not reachable from scale_render.rs:293-296). */
typedef enum ifhip_working_space { IFHIP_SPACE_SRGB = 0, IFHIP_SPACE_LINEAR = 1 } ifhip_working_space;

/* ffi/mod.rs:41-47 BitmapCompositingMode. */
typedef enum ifhip_compositing {
    IFHIP_REPLACE_SELF = 0, IFHIP_BLEND_WITH_SELF = 1, IFHIP_BLEND_WITH_MATTE = 2
} ifhip_compositing;

/* weights.rs:14-40 LobeRatio. */
typedef enum ifhip_lobe_mode { IFHIP_LOBE_NATURAL = 0, IFHIP_LOBE_EXACT = 1, IFHIP_LOBE_SHARPEN_PERCENT = 2 } ifhip_lobe_mode;

/* ---- library / device -------------------------------------------------------------------------------- */
IFHIP_API const char* ifhip_last_error_message(void);
IFHIP_API const char* ifhip_version(void);
/* Development switches of tests and tools/ (kernel choice for A/B runs, rarely taken paths forced): the library reads NO
 * environment variable -- what a call launches depends on its arguments only -- and a switch exists only after this call
 * (value NULL: unset).  Not part of the drop-in surface. */
IFHIP_API int ifhip_debug_set(const char* key, const char* value);
IFHIP_API int ifhip_device_count(void);            /* number of usable gfx950 devices (0 if none)          */
/* Compute units the resample launches of this PROCESS plan for (default and 0: all 256).  The fused kernel occupies a CU per
 * workgroup (its tables fill the LDS) and cuts frames into bands so that a launch fills the chip in whole rounds; a host that
 * runs something else beside it -- the batch harness overlaps the RCCL gather of batch k, a few workgroups, with the kernel
 * of batch k + 1 -- says how many CUs that leaves, and the band count is chosen for THAT number (finer bands, a short last
 * round) instead of a grid of exactly 256 workgroups whose last few wait a whole round for a CU.  Pixels do not depend on it. */
IFHIP_API int ifhip_set_cu_budget(uint32_t compute_units);
IFHIP_API int ifhip_set_device(int ordinal);       /* one process per GPU: call once with LOCAL_RANK       */
/* The HIP stream on which THIS THREAD's create calls (plans, stages, entropy handles) upload and clear what they need;
 * default: the null stream.  A host that runs one job per thread (one imageflow Context per thread, lib.rs:20-27) sets its
 * own stream here and passes the same stream to the *_device calls, so that jobs of different threads overlap. */
IFHIP_API void ifhip_set_thread_stream(void* hip_stream);
/* The library's block cache (csrc/devmem.cpp): plans, stages, entropy handles and the frames of ABI jobs are created and
 * destroyed once per JOB, so their device and pinned blocks are recycled through size-class free lists instead of hipMalloc /
 * hipFree (whose device-wide wait would serialise every thread's jobs).  What sits in the lists is invisible to every other
 * allocator on the device (torch's caching allocator, other processes):
 *   ifhip_cache_set_limits  bytes the lists may hold, per device / pinned (defaults 8 GiB / 1 GiB; 0 = recycle nothing);
 *   ifhip_cache_trim        give listed blocks back to the driver until at most the given bytes stay (0, 0: everything) --
 *                           what a torch user calls next to torch.cuda.empty_cache() or after an out-of-memory error;
 *   ifhip_cache_stats       hits / driver calls / bytes cached and handed out, for capacity planning and the jobs bench.
 * Blocks handed out are never touched.  Scratch of the device calls is released BEHIND the launch stream (an event marks the
 * point; no host wait): such blocks count as cached from that moment, are handed out again at once for work on the same
 * stream, to anybody once the event has completed, and a trim waits for them.  Thread safe. */
typedef struct ifhip_cache_stats_t {
    uint64_t device_hits, device_driver_allocs, device_driver_frees, device_oom_flushes, device_wide_syncs;
    uint64_t device_bytes_cached, device_bytes_live, device_blocks_live, device_limit_bytes;
    uint64_t host_hits, host_driver_allocs, host_driver_frees;
    uint64_t host_bytes_cached, host_bytes_live, host_blocks_live, host_limit_bytes;
} ifhip_cache_stats_t;
IFHIP_API int ifhip_cache_set_limits(size_t device_bytes, size_t host_bytes);
IFHIP_API int ifhip_cache_trim(size_t keep_device_bytes, size_t keep_host_bytes, size_t* released_device_bytes, size_t* released_host_bytes);
IFHIP_API int ifhip_cache_stats(ifhip_cache_stats_t* out);

/* ---- host-side tables (no GPU needed) ---------------------------------------------------------------- */
/* graphics/bitmaps.rs:712-740 Bitmap::get_stride::<u8>(w, h, 4, 64); 0 when the row does not fit 32 bits. */
IFHIP_API uint32_t ifhip_stride_for_width(uint32_t w);
/* graphics/weights.rs:681-788 populate_weights + PixelWeightIndexes (:555-571).  left[u]/count[u] give the first
 * source pixel and tap count of output pixel u; weights are concatenated in output order.  Pass
 * weights_capacity = 0 to query *n_weights.  kernel_width_scale = 1.0 unless set_kernel_width_scale is wanted. */
IFHIP_API int ifhip_populate_weights(int filter, int lobe_mode, float lobe_value, double kernel_width_scale,
                                     uint32_t output_line_size, uint32_t input_line_size,
                                     uint32_t* left_pixel, uint32_t* tap_count,
                                     float* weights, uint32_t weights_capacity, uint32_t* n_weights);
/* graphics/color.rs:22-45 ColorContext::byte_to_float (space = working space), 256 floats. */
IFHIP_API int ifhip_table_srgb_to_floatspace(int working_space, float* out256);
/* graphics/lut.rs:14-271 LINEAR_TO_SRGB_LUT, 16384 bytes. */
IFHIP_API int ifhip_table_linear_to_srgb(uint8_t* out16384);
/* The same table in the form the fused kernel keeps in LDS: thr[k] = first index whose value is >= k+1
 * (65535 if none), so table[i] == number of k with thr[k] <= i. */
IFHIP_API int ifhip_table_linear_to_srgb_thresholds(uint16_t* out256);

/* ---- Inner A: resample + render ---------------------------------------------------------------------- */
/*
 * Replaces imageflow_core::graphics::scaling::scale_and_render (graphics/scaling.rs:19-90) with
 * ScaleAndRenderParams (:8-17).  Host buffers, synchronous: upload -> kernels -> download of the touched
 * canvas rect.  in_alpha_meaningful = input.info().alpha_meaningful(); `compositing`/`matte_bgra` =
 * canvas.info().compose().  Errors as the reference: rect outside the canvas -> IFHIP_INVALID_ARGUMENT.
 */
IFHIP_API int ifhip_scale_and_render(const uint8_t* in, uint32_t in_w, uint32_t in_h, uint32_t in_stride,
                                     int in_alpha_meaningful,
                                     uint8_t* canvas, uint32_t canvas_w, uint32_t canvas_h, uint32_t canvas_stride,
                                     int canvas_alpha_meaningful,
                                     uint32_t x, uint32_t y, uint32_t w, uint32_t h,
                                     int filter, float sharpen_percent_goal, int working_space,
                                     int compositing, uint32_t matte_bgra);

/*
 * Device-resident batch form: what a job that keeps frames in HBM calls.  A plan owns the per-shape tables
 * (PixelRowWeights for both axes, the vertical schedule) for (in_w, in_h) -> (w, h); its tables are immutable and it
 * may be shared by any number of launches on the device it was created on (internal lazily built caches are locked).
 * The generic two-pass kernels (up-scaling, > 8 live rows, unaligned rows) stage through stream-ordered scratch
 * (a block of the library's cache, released behind the launch stream: ifhip_cache_stats counts it), so launches of one plan
 * may run on any number of streams.
 */
typedef struct ifhip_resample_plan ifhip_resample_plan;
IFHIP_API int ifhip_resample_plan_create(ifhip_resample_plan** plan, uint32_t in_w, uint32_t in_h,
                                         uint32_t w, uint32_t h, int filter, float sharpen_percent_goal);
IFHIP_API void ifhip_resample_plan_destroy(ifhip_resample_plan* plan);
/* introspection for tests/bench: 0 = fused single-pass kernel, 1 = generic two-pass kernels */
IFHIP_API int ifhip_resample_plan_kernel_kind(const ifhip_resample_plan* plan, int in_alpha_meaningful);
/* Diagnostic: the fused kernel's fast horizontal pass for this plan -- groups of four source columns per output (0: some
 * output needs more than four groups, the general pass runs) and groups of two (0: not available, or more than two thirds
 * of the taps; used for BGRA sources without meaningful alpha). */
IFHIP_API int ifhip_resample_plan_horizontal_groups(const ifhip_resample_plan* plan, uint32_t* four_column_groups,
                                                    uint32_t* two_column_groups);

/*
 * n_images independent frames, image i at d_in + i*in_image_bytes / d_canvas + i*canvas_image_bytes.
 * d_f32_dump (nullable): [n_images][h][w][4] premultiplied working-space floats (the f32 working buffer,
 * what StreamingResize::next_output_row_f32 yields at scaling.rs:195).
 * force_kernel: -1 auto, 0 fused, 1 generic, 2 banded (the generic pair fused through LDS: up-scales and small frames);
 * tests cross-check them.
 */
IFHIP_API int ifhip_scale_and_render_batch_device(const ifhip_resample_plan* plan,
                                                  const uint8_t* d_in, size_t in_image_bytes, uint32_t in_stride,
                                                  int in_alpha_meaningful, uint32_t n_images,
                                                  uint8_t* d_canvas, size_t canvas_image_bytes,
                                                  uint32_t canvas_w, uint32_t canvas_h, uint32_t canvas_stride,
                                                  uint32_t x, uint32_t y,
                                                  int working_space, int compositing, uint32_t matte_bgra,
                                                  float* d_f32_dump, int force_kernel, void* hip_stream);

/* Describes a launch and performs none (host only, for tests and tools: no device is asked for and no pixel is computed).
 * What ifhip_scale_and_render_batch_device would launch for a plan of (in_w, in_h, w, h, filter, sharpen_percent_goal) and
 * these frames -- planar_ycc_source: the component planes of the JPEG stage (in_stride = sample pitch, in_image_bytes =
 * plane size); source_alignment: the largest power of two, in bytes, the source pointers are aligned to -- as one line of
 * text in `line`: which kernel, and every number of its geometry.  It is the line the `trace_launch` debug switch prints
 * for the real launch, and it honours ifhip_set_cu_budget and the debug switches alike.  A launch that would fail returns
 * that status (message: ifhip_last_error_message). */
IFHIP_API int ifhip_describe_launch(uint32_t in_w, uint32_t in_h, uint32_t w, uint32_t h, int filter,
                                    float sharpen_percent_goal, int in_alpha_meaningful, int planar_ycc_source,
                                    uint32_t n_images, uint32_t in_stride, size_t in_image_bytes, uint32_t source_alignment,
                                    int working_space, int force_kernel, char* line, size_t line_capacity);

/* ---- Inner B: flatten --------------------------------------------------------------------------------- */
/* Replaces graphics::blend::apply_matte (graphics/blend.rs:6-59) / Bitmap::apply_matte (bitmaps.rs:528-541).
 * In place; no-op when !alpha_meaningful (blend.rs:11-13). */
IFHIP_API int ifhip_apply_matte(uint8_t* bgra, uint32_t w, uint32_t h, uint32_t stride, int alpha_meaningful,
                                uint32_t matte_bgra);
IFHIP_API int ifhip_apply_matte_batch_device(uint8_t* d_bgra, size_t image_bytes, uint32_t n_images,
                                             uint32_t w, uint32_t h, uint32_t stride, int alpha_meaningful,
                                             uint32_t matte_bgra, void* hip_stream);

/* ---- Inner C: JPEG pixel stage ------------------------------------------------------------------------- */
/*
 * Replaces what libjpeg does between entropy decoding and the scanline hand-over inside MzDec::read_frame
 * (codecs/mozjpeg_decoder.rs:295-420, wrap_jpeg_read_scan_lines codec_jpeg_wrapper.c:203-212): de-quantisation,
 * the islow 8x8 IDCT, "fancy" chroma up-sampling (h2v1 / h2v2) and YCbCr -> BGRA (out_color_space = JCS_EXT_BGRA,
 * :320; alpha bytes 255).  A GPU stage cannot be libjpeg's per-block IDCT callback, so the boundary is
 * "coefficient planes in, BGRA8 64-byte-stride bitmap out": the host keeps mozjpeg for the (serial) Huffman pass and
 * hands over what jpeg_read_coefficients() returns.
 *   coef[c]   int16 [blocks_h_c][blocks_w_c][64], natural (de-zigzagged) order, quantised;
 *             blocks_w_c = ceil(width / (8*hmax)) * h_samp[c], blocks_h_c likewise (MCU padded, as libjpeg's arrays)
 *   qt        uint16 [n_components][64], natural order (JQUANT_TBL.quantval)
 * scale_num / luma_spatial / luma_srgb are what MzDec::apply_downscaling (:588-618) and DecoderDownscaleHints
 * (ffi/c_interop.rs:6-15) set: libjpeg's scale_num/8 and whether the luma component goes through imageflow's
 * flow_scale_spatial[_srgb]_NxN block scalers (codec_jpeg_wrapper.c:274-343) instead of libjpeg's reduced IDCT.
 * Supported: scale_num 1..6 and 8 (7/8 is never requested, mozjpeg_decoder.rs:603-606) for grayscale, 4:4:4, 4:2:2 (h2v1),
 * 4:4:0 (h1v2) and 4:2:0 -- libjpeg's scaled IDCTs (jidctred.c 1x1/2x2/4x4, jidctint.c 3x3/5x5/6x6/10x10/12x12), its
 * per-component IDCT size rule (jdmaster.c: 4:2:0 chroma decodes at 2*scale_num, no up-sampling) and its up-sampler
 * choice (jdsample.c: triangle forms need scale_num > 1 and downsampled_width > 2, else replication).  The output
 * bitmap is ceil(width*scale_num/8) x ceil(height*scale_num/8).
 */
IFHIP_API int ifhip_jpeg_idct_color(const int16_t* coef0, const int16_t* coef1, const int16_t* coef2,
                                    const uint16_t* qt, int n_components,
                                    const uint8_t* h_samp, const uint8_t* v_samp,
                                    uint32_t width, uint32_t height,
                                    int scale_num, int luma_spatial, int luma_srgb,
                                    uint8_t* bgra, uint32_t stride);

/* Device-resident batch of equally shaped frames.  The stage object owns the component planes between the two
 * kernels.  d_coef[c]: image i at d_coef[c] + i * blocks_w_c*blocks_h_c*64; d_qt: [n_images][n_components][64]. */
typedef struct ifhip_jpeg_stage ifhip_jpeg_stage;
IFHIP_API int ifhip_jpeg_stage_create(ifhip_jpeg_stage** stage, uint32_t width, uint32_t height, int n_components,
                                      const uint8_t* h_samp, const uint8_t* v_samp,
                                      int scale_num, int luma_spatial, int luma_srgb, uint32_t max_images);
IFHIP_API int ifhip_jpeg_stage_output_size(const ifhip_jpeg_stage* stage, uint32_t* out_w, uint32_t* out_h);
IFHIP_API void ifhip_jpeg_stage_destroy(ifhip_jpeg_stage* stage);
IFHIP_API int ifhip_jpeg_stage_block_dims(const ifhip_jpeg_stage* stage, uint32_t* blocks_w3, uint32_t* blocks_h3);
IFHIP_API int ifhip_jpeg_idct_color_batch_device(ifhip_jpeg_stage* stage, const int16_t* d_coef0,
                                                 const int16_t* d_coef1, const int16_t* d_coef2,
                                                 const uint16_t* d_qt, uint32_t n_images,
                                                 uint8_t* d_bgra, size_t image_bytes, uint32_t stride, void* hip_stream);

/* Decode and resample as one device call: replaces MzDec::read_frame (codecs/mozjpeg_decoder.rs:346-362) producing the
 * bitmap that DrawImageDef::render (flow/nodes/scale_render.rs:304-313) hands to scale_and_render -- the pair every
 * `decode -> resample_2d / constrain` job runs.  `plan` must resample the stage's output size (ifhip_jpeg_stage_output_size).
 * When the component planes leave the IDCT at output resolution (4:2:0 decoded at 1/8 .. 4/8, where chroma takes the
 * twice-larger IDCT; 4:4:4 at any scale) the resampler reads the three planes and converts YCbCr -> RGB in its row fetch:
 * no decoded BGRA frame is written to or read from HBM, *fused = 1.  Every other case (fancy up-sampling, grayscale,
 * shapes the fused resampler does not take) runs ifhip_jpeg_idct_color_batch_device into a stream-ordered scratch
 * and ifhip_scale_and_render_batch_device, *fused = 0.  The canvas bytes are the same either way.  `fused` may be NULL. */
IFHIP_API int ifhip_jpeg_decode_resample_batch_device(ifhip_jpeg_stage* stage, const int16_t* d_coef0,
                                                      const int16_t* d_coef1, const int16_t* d_coef2,
                                                      const uint16_t* d_qt, uint32_t n_images,
                                                      const ifhip_resample_plan* plan,
                                                      uint8_t* d_canvas, size_t canvas_image_bytes, uint32_t canvas_w,
                                                      uint32_t canvas_h, uint32_t canvas_stride, uint32_t x, uint32_t y,
                                                      int working_space, int compositing, uint32_t matte_bgra,
                                                      int* fused, void* hip_stream);

/* Entropy stage: baseline sequential-Huffman decode of whole files on the GPU, in place of
 * the serial jpeg_read_coefficients / decode_mcu loop MzDec::read_frame drives on the host
 * (codecs/mozjpeg_decoder.rs:346-362).  ifhip_jpeg_parse_headers is host-only (no GPU): the SOF / DQT / DRI facts the
 * decoder's get_image_info needs (mozjpeg_decoder.rs:245-293).  A batch = n files of one geometry (size + sampling);
 * create() parses, un-stuffs and uploads the scans, decode_device() fills the coefficient planes the pixel stage reads
 * ([n][blocks_h][blocks_w][64] int16, natural order) and synchronises the stream.  Progressive, arithmetic-coded,
 * 12-bit, multi-scan and CMYK files return IFHIP_METHOD_NOT_IMPLEMENTED: keep those on libjpeg. */
typedef struct ifhip_jpeg_entropy ifhip_jpeg_entropy;
/* Diagnostic, host only (no GPU, nothing decoded into coefficients): the decode tables and the scan layout of one file,
 * checked against each other -- what tests/test_jpeg_headers.py asserts on every committed file without a device. */
typedef struct ifhip_jpeg_scan_report {
    uint32_t segments, sub_sequences, scan_complete;       /* restart segments; 1 024-bit sub-sequences; every MCU is covered */
    uint32_t pool_entries, pool_entries_used, prefixes_left_to_search, pair_entries;   /* second-level pool; first-level entries */
    uint32_t segments_with_wrong_block_count, segments_with_invalid_codes;           /* a serial walk with the tables */
    uint32_t pair_walk_mismatches, count_walk_mismatches;  /* sub-sequence boundaries where a pair-table walk differs from the plain one */
    uint64_t symbols, table_reads_with_pairs, blocks;
    int32_t dc_sum[3], dc_last_segment[3];                 /* sums of the DC differences per component (all segments / the last one) */
} ifhip_jpeg_scan_report;
IFHIP_API int ifhip_jpeg_debug_scan_report(const uint8_t* jpeg, size_t len, ifhip_jpeg_scan_report* out);
IFHIP_API int ifhip_jpeg_parse_headers(const uint8_t* jpeg, size_t len, uint32_t* width, uint32_t* height,
                                       int* n_components, uint8_t* h_samp3, uint8_t* v_samp3, uint32_t* blocks_w3,
                                       uint32_t* blocks_h3, uint16_t* qt3x64, uint32_t* restart_interval);
/* EXIF orientation as MozJpegDecoder::get_exif_rotation_flag reads it (codecs/mozjpeg_decoder.rs:290-292, :625-627 ->
 * mozjpeg_decoder_helpers.rs:107-202): *flag = -1 when the file carries none, else the tag's value 0..8.  Host only. */
IFHIP_API int ifhip_jpeg_exif_orientation(const uint8_t* jpeg, size_t len, int* flag);
/* The embedded colour profile as MozJpegDecoder sees it (APP2 "ICC_PROFILE" chunks, codecs/mozjpeg_decoder.rs:370-420):
 * the reference transforms a frame to sRGB whenever the file carries ANY profile (:409, SourceProfile::is_srgb is true
 * only for "no profile") unless the job told the decoder discard_color_profile (:88-95).  This library converts only
 * where the caller asks for it (ifhip_color_plan_from_icc / ifhip_color_transform below; the shim's colour-management
 * switch), so callers must know when a file needs it.  *kind = 0: no profile;
 * (also: a chunk set libjpeg's reassembly rule rejects -- mozjpeg_decoder_helpers.rs:42-83 returns None -- and a GRAY
 * profile on a colour frame, which the reference maps to SourceProfile::Srgb, mozjpeg_decoder.rs:391-395);
 * 1: a profile that describes sRGB itself (RGB matrix profile, sRGB primaries within 0.003 after D50 adaptation, the sRGB
 * tone curve) -- the reference's transform is the identity up to its own rounding; 2: any other profile (Display P3,
 * Adobe RGB, CMYK, grey on a grey frame, a profile too short to parse ...) -- decoding the samples as they are gives other colours than the
 * reference.  Host only. */
IFHIP_API int ifhip_jpeg_icc_profile_kind(const uint8_t* jpeg, size_t len, int* kind);
/* Host-side entropy decoding of the Huffman JPEGs the GPU entropy stage does not take -- progressive (SOF2: what the
 * reference's own mozjpeg encoder preset writes, codecs/mozjpeg.rs:121-123) and sequential files with several / non-
 * interleaved scans -- into the same coefficient planes ([blocks_h][blocks_w][64] int16, natural order, MCU-padded), so
 * that the pixel stage behind it is the GPU path unchanged (csrc/jpeg_read.cpp; libjpeg's jdphuff.c / jdhuff.c scans).
 * ifhip_jpeg_frame_info: the frame facts of any such file (and of baseline ones), *progressive = 1 for SOF2.
 * ifhip_jpeg_read_coefficients_host: planes sized by those facts (blocks_w * blocks_h * 64 each), cleared and filled;
 * qt3x64 (optional) receives each component's quantisation table. */
IFHIP_API int ifhip_jpeg_frame_info(const uint8_t* jpeg, size_t len, uint32_t* width, uint32_t* height, int* n_components,
                                    uint8_t* h_samp3, uint8_t* v_samp3, uint32_t* blocks_w3, uint32_t* blocks_h3,
                                    uint16_t* qt3x64, int* progressive);
IFHIP_API int ifhip_jpeg_read_coefficients_host(const uint8_t* jpeg, size_t len, int16_t* coef0, int16_t* coef1,
                                                int16_t* coef2, uint16_t* qt3x64);
IFHIP_API int ifhip_jpeg_entropy_create(ifhip_jpeg_entropy** out, const uint8_t* const* files, const size_t* lengths,
                                        uint32_t n_images);
IFHIP_API void ifhip_jpeg_entropy_destroy(ifhip_jpeg_entropy* e);
/* The same batch assembled from files that were PREPARED one by one (host only, any thread: parse, un-stuff, cut at the
 * restart markers, pack into pinned memory, derive the decode tables -- everything ifhip_jpeg_entropy_create does per
 * file).  A host that runs one job per thread prepares each job's file on that job's thread and hands whatever is waiting
 * to one create + decode call; the prepared handles may be destroyed as soon as create_prepared returns.  Errors of a
 * file (ImageMalformed, MethodNotImplemented) are reported by its prepare call. */
typedef struct ifhip_jpeg_prepared ifhip_jpeg_prepared;
IFHIP_API int ifhip_jpeg_entropy_prepare(ifhip_jpeg_prepared** out, const uint8_t* jpeg, size_t len);
IFHIP_API void ifhip_jpeg_prepared_destroy(ifhip_jpeg_prepared* p);
/* Optional, on a thread with a HIP device: queue the prepared scan's copy to the device on `hip_stream` NOW (asynchronous; the
 * call does not wait).  ifhip_jpeg_entropy_create_prepared then takes the words device to device behind that copy instead
 * of uploading them itself: with one job per thread the PCIe transfer of a job's file overlaps its wait for the next
 * coalesced batch instead of lengthening that batch.  A handle uploaded on one device and handed to a batch on another is
 * uploaded again from its pinned copy.  Destroying the handle waits for the queued copy if it is still running. */
IFHIP_API int ifhip_jpeg_prepared_upload(ifhip_jpeg_prepared* p, void* hip_stream);
IFHIP_API int ifhip_jpeg_prepared_info(const ifhip_jpeg_prepared* p, uint32_t* width, uint32_t* height, int* n_components,
                                       uint8_t* h_samp3, uint8_t* v_samp3);
IFHIP_API int ifhip_jpeg_entropy_create_prepared(ifhip_jpeg_entropy** out, ifhip_jpeg_prepared* const* prepared, uint32_t n_images);
IFHIP_API int ifhip_jpeg_entropy_info(const ifhip_jpeg_entropy* e, uint32_t* width, uint32_t* height, int* n_components,
                                      uint8_t* h_samp3, uint8_t* v_samp3, uint32_t* blocks_w3, uint32_t* blocks_h3,
                                      uint32_t* n_subsequences, uint32_t* n_segments);
IFHIP_API int ifhip_jpeg_entropy_quant_tables(const ifhip_jpeg_entropy* e, uint16_t* qt_n3x64);
IFHIP_API int ifhip_jpeg_entropy_decode_device(ifhip_jpeg_entropy* e, int16_t* d_coef0, int16_t* d_coef1,
                                               int16_t* d_coef2, uint32_t* rounds, void* hip_stream);

/* Encode-side pixel stage ("next" row 1): what libjpeg runs before entropy coding when
 * MozjpegEncoder::write_frame (codecs/mozjpeg.rs:78-160, classic preset = set_fastest_defaults, input JCS_EXT_BGRA /
 * JCS_EXT_BGRX) compresses a flattened frame: rgb_ycc_convert, chroma down-sampling with libjpeg's edge expansion,
 * the islow forward DCT, quantisation (round-half-up division by 8*Q) and the dummy blocks of the last MCU
 * column/row.  Output = the quantised coefficient planes jpeg_write_coefficients / the entropy coder consume
 * (same layout as the decode stage's input); sampling factors and quantisation tables come from the host
 * (evalchroma / set_quality stay host logic).  Call ifhip_apply_matte first when alpha is meaningful (:88-94). */
typedef struct ifhip_jpeg_fwd_stage ifhip_jpeg_fwd_stage;
IFHIP_API int ifhip_jpeg_fwd_stage_create(ifhip_jpeg_fwd_stage** stage, uint32_t width, uint32_t height,
                                          const uint8_t* h_samp, const uint8_t* v_samp, uint32_t max_images);
IFHIP_API void ifhip_jpeg_fwd_stage_destroy(ifhip_jpeg_fwd_stage* stage);
IFHIP_API int ifhip_jpeg_fwd_stage_block_dims(const ifhip_jpeg_fwd_stage* stage, uint32_t* blocks_w3, uint32_t* blocks_h3);
IFHIP_API int ifhip_jpeg_forward_batch_device(ifhip_jpeg_fwd_stage* stage, const uint8_t* d_bgra, size_t image_bytes,
                                              uint32_t stride, const uint16_t* d_qt, uint32_t n_images,
                                              int16_t* d_coef0, int16_t* d_coef1, int16_t* d_coef2, void* hip_stream);
IFHIP_API int ifhip_jpeg_forward(const uint8_t* bgra, uint32_t width, uint32_t height, uint32_t stride,
                                 const uint8_t* h_samp, const uint8_t* v_samp, const uint16_t* qt,
                                 int16_t* coef0, int16_t* coef1, int16_t* coef2);
/* The same stage without quantize_coef, for the trellis stage below: jpeg_fdct_islow's outputs as jfdctint.c leaves them
 * (scaled by 8) in int16 planes of the same layout; dummy blocks are zero, DC included.  Same stage object and argument
 * checks as ifhip_jpeg_forward_batch_device; no quantisation tables are read. */
IFHIP_API int ifhip_jpeg_forward_raw_batch_device(ifhip_jpeg_fwd_stage* stage, const uint8_t* d_bgra, size_t image_bytes,
                                                  uint32_t stride, uint32_t n_images, int16_t* d_raw0, int16_t* d_raw1,
                                                  int16_t* d_raw2, void* hip_stream);
/* Trellis quantisation for the mozjpeg preset: the interface this stands in for is the reference's default JPEG encoder
 * (codecs/mozjpeg.rs:37-59: MozjpegEncoder::create selects mozjpeg's own defaults, whose quantiser is mozjpeg's
 * jcdctmgr.c quantize_trellis).  Rate-distortion optimised quantisation of the raw planes, AC only: per frame and table
 * class (luma; Cb and Cr together) the plain quantiser's sequential AC symbols are counted, libjpeg's optimal code lengths
 * for them (every legal symbol counted once more) are the rate model, and every real block's levels minimise
 * sum w_i (|x_i| - level_i 8 Q_i)^2 + lambda_b * bits over the candidates 0, q_i and q_i - 1 (q_i the plain level; the
 * sign is x_i's), w_i = 1 / Q_i^2, lambda_b falling with the block's AC energy (mozjpeg's published lambda_log_scale1 /
 * lambda_log_scale2 = 14.75 / 16.5).  DC keeps its plain level; dummy blocks are as ifhip_jpeg_forward_batch_device
 * leaves them.  Integer arithmetic (csrc/jpeg_trellis_core.hpp): this project's restatement of the published algorithm,
 * pinned to its CPU emulation and not to mozjpeg's bytes.  lambda_scale: in 1/256ths of the tuned factor, at most 65535;
 * 256 is the preset's, 0 gives exactly the planes of ifhip_jpeg_forward_batch_device.  d_qt: [n_images][3][64] as there.
 * Planes are 16-byte aligned; every store is inside the planes' block counts.  Asynchronous on hip_stream. */
#define IFHIP_JPEG_TRELLIS_LAMBDA_ONE 256
typedef struct ifhip_jpeg_trellis_stage ifhip_jpeg_trellis_stage;
IFHIP_API int ifhip_jpeg_trellis_stage_create(ifhip_jpeg_trellis_stage** stage, uint32_t width, uint32_t height,
                                              const uint8_t* h_samp, const uint8_t* v_samp, uint32_t max_images);
IFHIP_API void ifhip_jpeg_trellis_stage_destroy(ifhip_jpeg_trellis_stage* stage);
IFHIP_API int ifhip_jpeg_trellis_batch_device(ifhip_jpeg_trellis_stage* stage, const int16_t* d_raw0, const int16_t* d_raw1,
                                              const int16_t* d_raw2, const uint16_t* d_qt, uint32_t lambda_scale,
                                              uint32_t n_images, int16_t* d_coef0, int16_t* d_coef1, int16_t* d_coef2,
                                              void* hip_stream);
/* The synchronous host-buffer drop-in (same stand-in, codecs/mozjpeg.rs:37-59 / jcdctmgr.c quantize_trellis): one frame's
 * raw planes and tables [3][64] in host memory, staged through the device. */
IFHIP_API int ifhip_jpeg_trellis(const int16_t* raw0, const int16_t* raw1, const int16_t* raw2, uint32_t width, uint32_t height,
                                 const uint8_t* h_samp, const uint8_t* v_samp, const uint16_t* qt, uint32_t lambda_scale,
                                 int16_t* coef0, int16_t* coef1, int16_t* coef2);
/* Host half of the same encoder: jpeg_set_quality's tables (jcparam.c: Annex K tables scaled, force_baseline; [0] luma,
 * [1] chroma, natural order) and the baseline file writer -- markers in jcmarker.c's order plus the sequential Huffman
 * coder with the Annex K tables (set_fastest_defaults: no optimised tables, not progressive).  Byte-identical to
 * libjpeg-turbo for the same pixels, quality and sampling.  coef*: host planes in the layout of ifhip_jpeg_forward.
 * out == NULL: only *len (the size needed) is written. */
IFHIP_API int ifhip_jpeg_quality_tables(int quality, uint16_t* qt2x64);
IFHIP_API int ifhip_jpeg_write_baseline(const int16_t* coef0, const int16_t* coef1, const int16_t* coef2,
                                        const uint32_t* blocks_w3, const uint32_t* blocks_h3, int n_components,
                                        const uint8_t* h_samp, const uint8_t* v_samp, uint32_t width, uint32_t height,
                                        int quality, uint8_t* out, size_t capacity, size_t* len);
/* The same writer with the classic preset's two options (codecs/mozjpeg.rs:121-129: set_progressive_mode,
 * set_optimize_coding over set_fastest_defaults).  IFHIP_JPEG_OPTIMIZE_HUFFMAN: two passes per scan -- symbol statistics,
 * then jchuff.c jpeg_gen_optimal_table's codes in the DHT segments.  IFHIP_JPEG_PROGRESSIVE: SOF2 and jcparam.c
 * jpeg_simple_progression's scan script (10 scans for YCbCr, 6 for gray; spectral selection + successive approximation,
 * jcphuff.c's end-of-band runs and correction bits), every scan with its own optimal tables as libjpeg does.
 * Byte-identical to libjpeg-turbo (Pillow optimize=True / progressive=True) for the same coefficients. */
#define IFHIP_JPEG_OPTIMIZE_HUFFMAN 1
#define IFHIP_JPEG_PROGRESSIVE 2
IFHIP_API int ifhip_jpeg_write(const int16_t* coef0, const int16_t* coef1, const int16_t* coef2,
                               const uint32_t* blocks_w3, const uint32_t* blocks_h3, int n_components,
                               const uint8_t* h_samp, const uint8_t* v_samp, uint32_t width, uint32_t height,
                               int quality, int flags, uint8_t* out, size_t capacity, size_t* len);
/* The batch form: n_images of one geometry, planes [n_images][bh_c][bw_c][64] (what ifhip_jpeg_forward_batch_device leaves,
 * downloaded), coded on up to `threads` host threads (0: one per core, at most n_images).  Files are packed into `out`
 * in image order at offsets[i], lengths[i] long; out == NULL queries *total. */
IFHIP_API int ifhip_jpeg_write_batch(const int16_t* coef0, const int16_t* coef1, const int16_t* coef2,
                                     const uint32_t* blocks_w3, const uint32_t* blocks_h3, int n_components,
                                     const uint8_t* h_samp, const uint8_t* v_samp, uint32_t width, uint32_t height,
                                     int quality, int flags, uint32_t n_images, uint32_t threads,
                                     uint8_t* out, size_t capacity, size_t* offsets, size_t* lengths, size_t* total);

/* Device entropy coder: the same baseline files without the host loop.  Replaces, for the classic preset's default
 * (codecs/mozjpeg.rs:108-129 with neither progressive nor optimize_coding), what compressor.write_scanlines / finish
 * (mozjpeg.rs:155-175) run behind the pixel stage: jchuff.c encode_mcu_huff / encode_one_block / emit_bits with byte
 * stuffing, and jcmarker.c's segments around the scan.  Coefficient planes stay in HBM ([n_images][bh_c][bw_c][64], the
 * layout ifhip_jpeg_forward_batch_device leaves); image i's file is written to d_files + i * file_pitch and its length to
 * d_lengths[i] -- 0 when the image was dropped, with the reason in d_status[i] (nullable): IFHIP_ENC_BAD_COEFFICIENT (a
 * coefficient with more magnitude bits than 8-bit JPEG codes: JERR_BAD_DCT_COEF), IFHIP_ENC_SCAN_OVERFLOW (the scan is
 * longer than the stage's scan_capacity), IFHIP_ENC_FILE_OVERFLOW (the file is longer than file_pitch).  Asynchronous on
 * hip_stream.  scan_capacity: bound of an image's entropy-coded bytes before stuffing, 0 = the most the geometry can
 * produce (208 bytes per block), with which no image is ever dropped for the scan's length.  Files are byte-identical to
 * ifhip_jpeg_write_baseline's for the same coefficients and quality.
 * A stage is bound to ONE stream at a time: it owns the scratch of a call in flight (bit counts, the word stream, the
 * marker segments of the current quality), so a second call must be ordered behind the first -- same stream, or an
 * event between them; use one stage per stream for concurrent batches. */
#define IFHIP_ENC_BAD_COEFFICIENT 1
#define IFHIP_ENC_SCAN_OVERFLOW 2
#define IFHIP_ENC_FILE_OVERFLOW 4
typedef struct ifhip_jpeg_enc_stage ifhip_jpeg_enc_stage;
IFHIP_API int ifhip_jpeg_enc_stage_create(ifhip_jpeg_enc_stage** stage, uint32_t width, uint32_t height, int n_components,
                                          const uint8_t* h_samp, const uint8_t* v_samp, const uint32_t* blocks_w3,
                                          const uint32_t* blocks_h3, uint32_t max_images, size_t scan_capacity);
IFHIP_API void ifhip_jpeg_enc_stage_destroy(ifhip_jpeg_enc_stage* stage);
/* a file_pitch with which no file overflows (marker segments + every stream byte stuffed + EOI) */
/* The files of a batch as ONE message for the job's final gather: image i's file (d_lengths[i] bytes
 * at d_files + i * file_pitch, as ifhip_jpeg_encode_batch_device leaves it; a dropped image has length 0) is copied to
 * d_out + d_offsets[i], every start rounded up to 16 bytes; d_offsets[n_files] = the bytes used.  When that exceeds
 * out_capacity the files that do not fit are not copied (the caller compares).  file_pitch, d_files and d_out 16-byte
 * aligned; a file's padding bytes are unspecified.  Asynchronous on hip_stream. */
IFHIP_API int ifhip_pack_files_device(const uint8_t* d_files, size_t file_pitch, const uint32_t* d_lengths, uint32_t n_files,
                                      uint8_t* d_out, size_t out_capacity, uint64_t* d_offsets, void* hip_stream);
IFHIP_API size_t ifhip_jpeg_enc_stage_max_file_bytes(const ifhip_jpeg_enc_stage* stage);
IFHIP_API int ifhip_jpeg_encode_batch_device(ifhip_jpeg_enc_stage* stage, const int16_t* d_coef0, const int16_t* d_coef1,
                                             const int16_t* d_coef2, int quality, uint32_t n_images, uint8_t* d_files,
                                             size_t file_pitch, uint32_t* d_lengths, uint32_t* d_status, void* hip_stream);
/* The preset's two options on the device: flags = IFHIP_JPEG_OPTIMIZE_HUFFMAN | IFHIP_JPEG_PROGRESSIVE as for
 * ifhip_jpeg_write; files are byte-identical to ifhip_jpeg_write's (and libjpeg-turbo's) for the same flags.  flags == 0
 * IS ifhip_jpeg_encode_batch_device.  Optimised tables alone: one interleaved sequential scan against per-image tables
 * (jpeg_gen_optimal_table).  Progressive: SOF2, jpeg_simple_progression's 10 scans (6 for gray), every scan with optimal
 * tables of its own.  Passes of one call, all images and scans in each, no host round trip between them: symbol statistics
 * per (scan, block); end-of-band runs (a maximal sequence of blocks without a symbol of their own, cut greedily at 0x7FFF
 * blocks or more than 937 buffered correction bits, resolved by one wave per 2048 blocks walking the runs that start there);
 * one wave per table builds the code; bit counts; prefix sums per scan; the write pass; byte stuffing, every scan a stream
 * of its own behind its DHT and SOS segments, whose offsets come from a per-image scan on the device.
 * The stage allocates the extra scratch on the FIRST flagged call (about 6 bytes per block and scan, 20 KiB of tables per
 * image, and a word stream of its own) and keeps it until the stage is destroyed; that call can therefore fail with
 * IFHIP_ALLOCATION_FAILED / IFHIP_GPU_ERROR, or with IFHIP_INVALID_ARGUMENT when the streams of an image could exceed
 * 2^32 bit positions (bound them with scan_capacity).  scan_capacity bounds an image's entropy-coded bytes before stuffing
 * SUMMED over its scans.  Status bits, drop semantics (length 0, neighbours untouched, nothing stored behind a slot) and the
 * one-stream-per-stage rule are those of ifhip_jpeg_encode_batch_device.
 *
 * ifhip_jpeg_enc_stage_max_file_bytes_for(stage, flags): an arithmetic file_pitch with which no file of these flags
 * overflows (0: unknown flags, or the geometry is refused); for flags == 0 exactly ifhip_jpeg_enc_stage_max_file_bytes.
 * Derivation.  Bits of one block in one scan, with codes of at most 16 bits: sequential 16 + 11 + 63 * (16 + 10); DC
 * first 16 + 11; DC refinement 1; AC first (Se - Ss + 1) * (16 + 10) + 30 (the EOBn field, 16 + 14, charged to a run's
 * first block); AC refinement (Se - Ss + 1) * 17 + 4 * 16 + 30 + 63 (code and sign per new coefficient, ZRLs, EOBn, 63
 * correction bits).  worst = the sum over scans of ceil(blocks * bits / 8); stream = min(scan_capacity, worst) rounded up
 * to 4 KiB chunks, plus one chunk per scan and one to spare (every scan starts on a chunk boundary of the word stream; an
 * image whose scans need more chunks is dropped with IFHIP_ENC_SCAN_OVERFLOW).  Every stream byte may be stuffed, so
 * bound = 177 (SOI, APP0, two DQT, SOF) + 14 per SOS + 277 per DHT (one per table of every scan) + 2 * stream + 2 (EOI). */
IFHIP_API size_t ifhip_jpeg_enc_stage_max_file_bytes_for(const ifhip_jpeg_enc_stage* stage, int flags);
IFHIP_API int ifhip_jpeg_encode_flags_batch_device(ifhip_jpeg_enc_stage* stage, const int16_t* d_coef0, const int16_t* d_coef1,
                                                   const int16_t* d_coef2, int quality, int flags, uint32_t n_images,
                                                   uint8_t* d_files, size_t file_pitch, uint32_t* d_lengths,
                                                   uint32_t* d_status, void* hip_stream);

/* Device PNG coder: EncoderPreset::Libpng {depth, matte, zlib_compression} (imageflow_types/src/lib.rs:751-755, chosen in
 * codecs/auto.rs:241-268) without the host: what LibPngEncoder::write_frame (codecs/libpng_encoder.rs:43-72,134-160) has
 * flow_codecs_png_encoder_write_frame / png_write_image do (c_components/lib/codec_png_wrapper.c:349-430) -- 8-bit RGB or
 * RGBA, non-interlaced, png_set_sRGB_gAMA_and_cHRM's three chunks, libpng's default adaptive row filters, one zlib stream --
 * on BGRA / BGRX frames that stay in HBM.  Every row carries the filter libpng's default choice takes; the deflate blocks
 * are this coder's own (a parallel parse: 32 KiB blocks, each closed to a byte boundary), so a file is NOT libpng's byte
 * for byte -- it decodes to the same pixels and is never larger than stored blocks.
 * color_type: IFHIP_PNG_RGB drops the alpha byte (it is not flattened: apply a matte first), IFHIP_PNG_RGBA keeps it.
 * A stage owns the scratch of a call in flight (filtered streams, tokens, symbol counts, code tables, scan arrays; it is
 * allocated by the first batch), so it is bound to ONE stream at a time: a second call must be ordered behind the first --
 * same stream, or an event between them; use one stage per stream for concurrent batches. */
#define IFHIP_PNG_RGB 2
#define IFHIP_PNG_RGBA 6
#define IFHIP_PNG_FILE_OVERFLOW 1
typedef struct ifhip_png_enc_stage ifhip_png_enc_stage;
IFHIP_API int ifhip_png_enc_stage_create(ifhip_png_enc_stage** stage, uint32_t width, uint32_t height, int color_type,
                                         uint32_t max_images);
IFHIP_API void ifhip_png_enc_stage_destroy(ifhip_png_enc_stage* stage);
/* a file_pitch with which no file overflows: every block stored (codec_png_wrapper.c's worst case too: zlib never grows a
 * stream by more than its stored form) plus the framing.  With it IFHIP_PNG_FILE_OVERFLOW is never raised. */
IFHIP_API size_t ifhip_png_enc_stage_max_file_bytes(const ifhip_png_enc_stage* stage);
/* n_images frames of the stage's geometry at d_images + i * image_bytes (rows of `stride` bytes; the frame checks of every
 * batch entry, made before the device is asked for).  Image i's file goes to d_files + i * file_pitch, its length to
 * d_lengths[i] -- 0 when the file is longer than file_pitch, with IFHIP_PNG_FILE_OVERFLOW in d_status[i] (nullable).
 * zlib_level is the preset's zlib_compression (codec_png_wrapper.c:380-387 png_set_compression_level): 0 writes stored
 * blocks only; 1..9 and -1 all run the ONE device strategy -- levels do not change the search, only the FLEVEL bits of the
 * zlib header.  Asynchronous on hip_stream.  The same pixels give the same bytes on every run and in every batch. */
IFHIP_API int ifhip_png_encode_batch_device(ifhip_png_enc_stage* stage, const uint8_t* d_images, size_t image_bytes,
                                            uint32_t stride, uint32_t n_images, int zlib_level, uint8_t* d_files,
                                            size_t file_pitch, uint32_t* d_lengths, uint32_t* d_status, void* hip_stream);
/* The synchronous host-buffer drop-in for flow_codecs_png_encoder_write_frame (codec_png_wrapper.c:349-430): one frame.
 * out == NULL: only *len (the size needed) is written. */
IFHIP_API int ifhip_png_encode(const uint8_t* bgra, uint32_t width, uint32_t height, uint32_t stride, int color_type,
                               int zlib_level, uint8_t* out, size_t capacity, size_t* len);

/* Device palette PNG coder: EncoderPreset::Pngquant {quality, minimum_quality, speed, maximum_deflate}
 * (imageflow_types/src/lib.rs:756-761) without the host: what PngquantEncoder (codecs/pngquant.rs:35-139) has libimagequant
 * and lode::LodepngEncoder::write_png8 (lode.rs:162-195) do -- at most 256 RGBA colours, Floyd-Steinberg dithering at full
 * strength, an 8-bit palette PNG: colour type 3, filter 0 on every row, IHDR, PLTE, tRNS (only when an entry has alpha
 * below 255; such entries come first), one IDAT, IEND, no gAMA / sRGB / cHRM -- on BGRA / BGRX frames that stay in HBM.
 * The quantiser is this library's own: a frame of at most 256 distinct colours keeps exactly those (all pixels of alpha 0
 * count as 00 00 00 00); otherwise the palette is NOT libimagequant's, and the quality scale is not pinned to it either.
 * The zlib stream comes from the coder above (same blocks, same notes).  A stage owns the scratch of a call in flight and
 * is bound to ONE stream at a time, like ifhip_png_enc_stage. */
#define IFHIP_PNG_QUALITY_TOO_LOW 2
typedef struct ifhip_png_quant_stage ifhip_png_quant_stage;
/* refused: zero dimensions, more than 2^28 pixels, and frames of 1024 rows or more that are wider than 16384 pixels */
IFHIP_API int ifhip_png_quant_stage_create(ifhip_png_quant_stage** stage, uint32_t width, uint32_t height, uint32_t max_images);
IFHIP_API void ifhip_png_quant_stage_destroy(ifhip_png_quant_stage* stage);
/* a file_pitch with which no file overflows: every block stored, plus the framing with a full PLTE and tRNS */
IFHIP_API size_t ifhip_png_quant_stage_max_file_bytes(const ifhip_png_quant_stage* stage);
/* n_images frames as in ifhip_png_encode_batch_device.  alpha_meaningful 0: every alpha byte counts as 255
 * (normalize_unused_alpha).  quality / min_quality / speed as PngquantEncoder::create clamps them (codecs/pngquant.rs:50-57):
 * speed 1..10, target = quality 0..100, minimum 0..target; a negative value stands for an absent one (100, 0, and
 * libimagequant's default speed 4).  max_colors 2..256 (the preset passes 256), dither 0 or 1 (the preset passes 1),
 * zlib_level as above (maximum_deflate: 9; it changes the FLEVEL bits only).
 * Image i's file goes to d_files + i * file_pitch and its length to d_lengths[i].  d_status[i] (nullable):
 * IFHIP_PNG_QUALITY_TOO_LOW when the palette's error, before dithering, is above what min_quality allows -- length 0, the
 * caller writes a lossless file instead (codecs/pngquant.rs:105-139); IFHIP_PNG_FILE_OVERFLOW as above.  Neither touches
 * the other images of the batch.  Nullable taps: d_palettes (per image 256 RGBA entries in file order, then the count
 * as a little-endian u32: 1028 bytes), d_indices (per image width * height palette indices), d_mse (per image the mean
 * error before dithering as a double, 1.0 = black against white).
 * Asynchronous on hip_stream.  The same pixels give the same bytes on every run and in every batch position. */
IFHIP_API int ifhip_png_quantize_batch_device(ifhip_png_quant_stage* stage, const uint8_t* d_images, size_t image_bytes,
                                              uint32_t stride, int alpha_meaningful, uint32_t n_images, int quality,
                                              int min_quality, int speed, uint32_t max_colors, int dither, int zlib_level,
                                              uint8_t* d_files, size_t file_pitch, uint32_t* d_lengths, uint32_t* d_status,
                                              uint8_t* d_palettes, uint8_t* d_indices, double* d_mse, void* hip_stream);
/* The synchronous host-buffer form (codecs/pngquant.rs:35-139 up to the fallback): one frame, 256 colours, dithered,
 * zlib level 6.  *status (nullable) gets the status word; with IFHIP_PNG_QUALITY_TOO_LOW the call succeeds and *len is 0.
 * out == NULL: only *len (the size needed) is written. */
IFHIP_API int ifhip_png_quantize(const uint8_t* bgra, uint32_t width, uint32_t height, uint32_t stride, int alpha_meaningful,
                                 int quality, int min_quality, int speed, uint8_t* out, size_t capacity, size_t* len,
                                 uint32_t* status);

/* Device lossless WebP coder: EncoderPreset::WebPLossless (imageflow_types/src/lib.rs EncoderPreset, chosen in
 * codecs/auto.rs:282-319) without the host: what WebPEncoder::write_frame (codecs/webp.rs:281-345) has libwebp's
 * WebPEncodeLosslessBGRA / WebPEncodeLosslessBGR do -- a VP8L stream in a RIFF container -- on BGRA / BGRX frames that stay
 * in HBM.  A lossless coder is free in its choices: the file is NOT libwebp's byte for byte, it decodes through libwebp to
 * exactly the frame's pixels.  The choices are this coder's own: subtract green, one of the 14 predictors per 16 x 16 tile,
 * matches over the residual pixels one pixel back and one row up, a group of five prefix codes per band of 64 rows, no
 * colour cache; colour indexing only where the stage's flags ask for it (ifhip_webp_enc_stage_create_flags).
 * alpha_meaningful 0 (normalize_unused_alpha): every pixel is coded with alpha 255 and the header says alpha_is_used = 0.
 * There is no matte (the reference passes None).  A stage owns the scratch of a call in flight (residuals, tokens, symbol
 * counts, code tables, bit offsets; allocated by the first batch) and is bound to ONE stream at a time, like
 * ifhip_png_enc_stage. */
#define IFHIP_WEBP_FILE_OVERFLOW 1
typedef struct ifhip_webp_enc_stage ifhip_webp_enc_stage;
/* refused: zero dimensions, a width or a height above 16384 (the format's 14 bits), max_images outside 1..65535 */
IFHIP_API int ifhip_webp_enc_stage_create(ifhip_webp_enc_stage** stage, uint32_t width, uint32_t height, int alpha_meaningful,
                                          uint32_t max_images);
/* The same with flags; 0 is ifhip_webp_enc_stage_create to the byte, an unknown bit is refused.
 * IFHIP_WEBP_ENC_COLOR_INDEXING: a frame of at most 256 distinct colours (alpha forced to 255 where it is not meaningful) is
 * also sized as a stream that opens with the colour-indexing transform -- the palette in ascending ARGB order, 8, 4 or 2
 * indices bundled into a pixel for up to 2, 4 or 16 colours, matches and codes over the packed pixels -- and the smaller of
 * the two files is written, the plain one on a tie: no file is larger than without the flag, so the bound below holds
 * unchanged.  A frame of more colours is the file without the flag, byte for byte, at the price of a partial read of it.
 * The stage then owns a second set of scratch for the packed image. */
#define IFHIP_WEBP_ENC_COLOR_INDEXING 1u
IFHIP_API int ifhip_webp_enc_stage_create_flags(ifhip_webp_enc_stage** stage, uint32_t width, uint32_t height, int alpha_meaningful,
                                                uint32_t max_images, uint32_t flags);
IFHIP_API void ifhip_webp_enc_stage_destroy(ifhip_webp_enc_stage* stage);
/* a file_pitch with which no file overflows, by arithmetic over the coder's choices (csrc/webp_encode_core.hpp
 * webp_max_file_bytes): a band that would take more is written as literals under four flat codes, which gives 32 bits a
 * pixel, plus the worst-case head, the bands' flat-code headers and the RIFF framing.  With it IFHIP_WEBP_FILE_OVERFLOW is never raised. */
IFHIP_API size_t ifhip_webp_enc_stage_max_file_bytes(const ifhip_webp_enc_stage* stage);
/* n_images frames of the stage's geometry at d_images + i * image_bytes (rows of `stride` bytes; the frame checks of every
 * batch entry, made before the device is asked for).  Image i's file goes to d_files + i * file_pitch, its length to
 * d_lengths[i] -- 0 when the file is longer than file_pitch, with IFHIP_WEBP_FILE_OVERFLOW in d_status[i] (nullable); its
 * neighbours are untouched.  All of d_files' n_images * file_pitch bytes are written (zeros behind a file) and none
 * beyond them; d_files must be 4-byte aligned, file_pitch may be any size from 28 bytes on.
 * Asynchronous on hip_stream.  The same pixels give the same bytes on every run and in every batch position. */
IFHIP_API int ifhip_webp_encode_batch_device(ifhip_webp_enc_stage* stage, const uint8_t* d_images, size_t image_bytes,
                                             uint32_t stride, uint32_t n_images, uint8_t* d_files, size_t file_pitch,
                                             uint32_t* d_lengths, uint32_t* d_status, void* hip_stream);
/* The synchronous host-buffer drop-in for WebPEncodeLosslessBGRA / WebPEncodeLosslessBGR (codecs/webp.rs:281-345): one
 * frame.  out == NULL: only *len (the size needed) is written. */
IFHIP_API int ifhip_webp_encode(const uint8_t* bgra, uint32_t width, uint32_t height, uint32_t stride, int alpha_meaningful,
                                uint8_t* out, size_t capacity, size_t* len);

/* Which coder the shim's `encode` node hands an EncoderPreset to (imageflow_types/src/lib.rs:745-774, chosen in
 * codecs/auto.rs), given the preset's JSON text: an object with the key libjpeg_turbo / libpng / pngquant / mozjpeg, or the string
 * "webplossless" (a unit variant); every other preset ("gif", webplossy in any form, lodepng, ...) gets the raw BGRA
 * container.  -1: the text is no JSON.  Host only: it lets a test see the dispatch without a device. */
#define IFHIP_ENCODE_CODER_RAW 0
#define IFHIP_ENCODE_CODER_JPEG 1
#define IFHIP_ENCODE_CODER_PNG 2
#define IFHIP_ENCODE_CODER_PNGQUANT 3
#define IFHIP_ENCODE_CODER_WEBP_LOSSLESS 4
#define IFHIP_ENCODE_CODER_MOZJPEG 5      /* the key mozjpeg: the libjpeg_turbo chain with the trellis stage, always progressive */
IFHIP_API int ifhip_encode_preset_coder(const char* preset_json, size_t len);

/* Device PNG decoder: what LibPngDecoder (imageflow_core/src/codecs/libpng_decoder.rs:36-104,297-299,340-383) gets from
 * libpng (c_components/lib/codec_png_wrapper.c:131-212 wrap_png_decode_image_info, :215-246 wrap_png_decode_finish, :266-292
 * wrap_png_decoder_get_info) -- all 15 legal (colour type, bit depth) pairs, interlaced or not, normalised to 8-bit BGRA in
 * libpng's order: expand (palette -> RGB, gray 1/2/4 -> 8 bits, tRNS -> alpha with the key compared at the file's depth),
 * filler 0xFF, strip 16 -> 8 by the high byte, gray -> RGB, BGR, Adam7 resolved.  The host parses the chunks and gathers the
 * IDAT payloads (csrc/png_read.cpp); inflate, un-filter and expansion run on the device (csrc/png_decode.hip).
 *
 * alpha_used (-> alpha_meaningful, frame_decodes_into bgra_32 / bgr_32) is true for colour types with alpha and for palette
 * files with or without tRNS (codec_png_wrapper.c:176-186): gray / RGB with a tRNS key decode with real alpha bytes in a
 * frame marked bgr_32.  uses_palette: colour type bit 0 (:270).  color_kind, in the convention of
 * ifhip_jpeg_icc_profile_kind: 0 no colour chunks, or gAMA alone (honor_gama_only = false, libpng_decoder.rs:234); 1 sRGB
 * declared (an sRGB chunk, an iCCP profile that describes sRGB, gAMA + cHRM with the specification's sRGB values); 2 any
 * other colour space (another iCCP profile, other gAMA + cHRM) -- the reference converts such frames (:340-383); this
 * decoder never does, so callers must refuse, be told discard_color_profile, or convert the decoded frame themselves
 * (ifhip_color_plan_from_icc / _from_gamma_primaries + ifhip_color_transform_batch_device, as the shim does once switched on).
 *
 * Status word of a file (d_status[i]): 0, or why its stream is no image -- libpng's errors. */
#define IFHIP_PNG_DEC_TRUNCATED 1        /* the zlib stream ends early                                        */
#define IFHIP_PNG_DEC_BLOCK_TYPE 2       /* deflate block type 3                                              */
#define IFHIP_PNG_DEC_STORED_LENGTH 3    /* LEN / NLEN of a stored block do not match                          */
#define IFHIP_PNG_DEC_CODE_LENGTHS 4     /* over-subscribed or incomplete code, bad repeat, no end-of-block    */
#define IFHIP_PNG_DEC_BAD_CODE 5         /* bits that are no code, or a reserved symbol                       */
#define IFHIP_PNG_DEC_DISTANCE 6         /* a distance that reaches before the stream's start                 */
#define IFHIP_PNG_DEC_ZLIB_HEADER 7
#define IFHIP_PNG_DEC_ADLER 8            /* Adler-32 mismatch: refused                                        */
#define IFHIP_PNG_DEC_TOO_LITTLE 9       /* "Not enough image data"                                           */
#define IFHIP_PNG_DEC_FILTER 10          /* "bad adaptive filter value"                                       */
#define IFHIP_PNG_DEC_CONTAINER 11       /* batch only: the file's chunks did not parse (signature, CRC, IHDR, PLTE ...),
                                          * or its image would inflate beyond 2^31 bytes                              */
typedef struct ifhip_png_file_info {
    uint32_t width, height, bit_depth, color_type, interlace;
    uint32_t alpha_used, uses_palette;
    int32_t color_kind;
} ifhip_png_file_info;
/* Header facts (png_read_info; libpng_decoder.rs:40-52 get_unscaled_image_info = get_scaled_image_info :36-38).  Walks all
 * chunks: a bad CRC on IHDR / PLTE / tRNS / IDAT / IEND / the colour chunks, a malformed critical chunk or a missing IEND is
 * IFHIP_INVALID_ARGUMENT with an "ImageMalformed: LibPNG error: ..." message.  Host only, no device needed. */
IFHIP_API int ifhip_png_info(const uint8_t* png, size_t len, ifhip_png_file_info* info);
/* n files (host memory), each with its own geometry, type and depth, into n device frames: d_frames[i] holds height_i rows of
 * strides[i] bytes inside frame_bytes[i]; only the 4 * width_i bytes of a row are written.  d_status[i] (device) receives the
 * file's status word; a damaged file leaves its frame untouched and never disturbs its neighbours.  Three launches per
 * batch, every file in each: inflate (one wave per stream), un-filter (a skewed wavefront over 64 rows), expansion.  The
 * streams are uploaded before the call returns; the kernels are asynchronous on hip_stream.  Colour chunks are NOT acted
 * on here (see color_kind).  Argument and frame checks come before the device check. */
IFHIP_API int ifhip_png_decode_batch_device(const uint8_t* const* files, const size_t* lens, uint32_t n_files,
                                            uint8_t* const* d_frames, const size_t* frame_bytes, const uint32_t* strides,
                                            uint32_t* d_status, void* hip_stream);
/* The synchronous host-buffer drop-in for wrap_png_decode_image_info + wrap_png_decode_finish (codec_png_wrapper.c:131-246):
 * one file into `height` BGRA rows of `stride` bytes at bgra (capacity bytes; bytes between rows are kept).  A non-zero
 * status word comes back in *status (nullable) with IFHIP_INVALID_ARGUMENT and an "ImageMalformed: LibPNG error" message. */
IFHIP_API int ifhip_png_decode(const uint8_t* png, size_t len, uint8_t* bgra, uint32_t stride, size_t capacity,
                               uint32_t* status);

/* Device WebP decoder, lossless files: what WebPDecoder (imageflow_core/src/codecs/webp.rs:20-248) gets from WebPGetFeatures
 * and WebPDecode(MODE_BGRA) for a VP8L file -- BGRA bytes, the alpha bytes as coded whatever has_alpha says.  The host walks
 * the RIFF container and prepares the stream (header, transforms with their sub-images, entropy image, every group's codes:
 * csrc/webp_read.cpp); the main image's token loop and the inverse transforms run on the device (csrc/webp_decode.hip).
 * Not built: lossy VP8 (+ ALPH), animation, libwebp's decode-time rescaler.
 *
 * has_alpha (-> frame_decodes_into bgra_32 / bgr_32, webp.rs:144-148,204) is what WebPGetFeatures reports: for a lossless
 * file the VP8L header's bit, whatever a VP8X chunk's ALPHA flag says.  color_kind, in the convention of
 * ifhip_jpeg_icc_profile_kind: 0 no ICCP chunk (or the VP8X ICC flag clear), 1 a profile that describes sRGB, 2 any other --
 * this decoder never converts, so callers must refuse, be told discard_color_profile, or convert the decoded frame themselves
 * (ifhip_color_plan_from_icc + ifhip_color_transform_batch_device, as the shim does once switched on).
 *
 * Status word of a file (d_status[i]): 0, or why its stream is no image. */
#define IFHIP_WEBP_DEC_TRUNCATED 1       /* a bit was used that the stream does not have                       */
#define IFHIP_WEBP_DEC_CODE_LENGTHS 2    /* over-subscribed or incomplete code, no symbol, a repeat or max_symbol beyond the alphabet */
#define IFHIP_WEBP_DEC_BAD_CODE 3        /* bits that are no code                                               */
#define IFHIP_WEBP_DEC_DISTANCE 4        /* a copy from before the image's first pixel                          */
#define IFHIP_WEBP_DEC_COPY_END 5        /* a copy past the image's last pixel                                  */
#define IFHIP_WEBP_DEC_CACHE_SYMBOL 6    /* a colour cache symbol beyond the cache (no file reaches it: a guard) */
#define IFHIP_WEBP_DEC_TRANSFORM 7       /* a transform twice, colour cache bits outside 1..11                  */
#define IFHIP_WEBP_DEC_TOO_LITTLE 8      /* the payload ends inside the VP8L header (the container walk refuses it first: CONTAINER) */
#define IFHIP_WEBP_DEC_CONTAINER 9       /* batch only: the RIFF container did not parse, or the file is lossy or animated */
typedef struct ifhip_webp_file_info {
    uint32_t width, height;
    uint32_t has_alpha, lossless, animated;
    int32_t color_kind;
} ifhip_webp_file_info;
/* Container facts (WebPGetFeatures).  A lossy file (lossless = 0) and an animation (animated = 1, the canvas size) are
 * answered here and refused by the decode calls.  A truncated or inconsistent container is IFHIP_INVALID_ARGUMENT with an
 * "ImageMalformed: libwebp decoding error ..." message.  Host only, no device needed. */
IFHIP_API int ifhip_webp_info(const uint8_t* webp, size_t len, ifhip_webp_file_info* info);
/* n files (host memory), each with its own size and transforms, into n device frames: d_frames[i] holds height_i rows of
 * strides[i] bytes inside frame_bytes[i]; only the 4 * width_i bytes of a row are written.  d_status[i] (device) receives the
 * file's status word; a damaged file leaves its frame untouched and never disturbs its neighbours.  A fixed number of
 * launches per batch, every file in each: the token loop (one wave per file) and at most four inverse-transform steps.
 * The streams are uploaded before the call returns; the kernels are asynchronous on hip_stream.  ICCP chunks are NOT acted
 * on here (see color_kind).  Argument and frame checks come before the device check. */
IFHIP_API int ifhip_webp_decode_batch_device(const uint8_t* const* files, const size_t* lens, uint32_t n_files,
                                             uint8_t* const* d_frames, const size_t* frame_bytes, const uint32_t* strides,
                                             uint32_t* d_status, void* hip_stream);
/* The synchronous host-buffer drop-in for WebPDecode(MODE_BGRA): one file into `height` BGRA rows of `stride` bytes at bgra
 * (capacity bytes; bytes between rows are kept).  A non-zero status word comes back in *status (nullable) with
 * IFHIP_INVALID_ARGUMENT and an "ImageMalformed: libwebp decoding error" message; a lossy file is
 * IFHIP_METHOD_NOT_IMPLEMENTED with an "ImageTypeNotSupported" message. */
IFHIP_API int ifhip_webp_decode(const uint8_t* webp, size_t len, uint8_t* bgra, uint32_t stride, size_t capacity,
                                uint32_t* status);

/* Device WebP decoder, lossy files: what WebPDecoder (imageflow_core/src/codecs/webp.rs:162-248) gets from WebPDecode(MODE_BGRA)
 * for a still `VP8 ` file, with or without an `ALPH` chunk -- libwebp 1.6.0's default options: fancy upsampling, the loop filter
 * honoured, no dithering, alpha not premultiplied.  The host walks the container, reads the key frame's header and bool-decodes
 * its partitions (csrc/vp8_read.cpp: modes and un-dequantised coefficient levels); dequantisation, the inverse transforms,
 * intra prediction, the loop filter, the alpha plane and the conversion to BGRA run on the device (csrc/vp8_decode.hip).
 * ifhip_webp_info answers the container's facts for these files too (lossless = 0; has_alpha is the VP8X ALPHA flag or an ALPH
 * chunk).  The batch form, ifhip_webp_lossy_decode_batch_device, is declared in imageflow_hip_webp_lossy.h.
 * Not built: animation, libwebp's decode-time rescaler.
 *
 * Status word of a file: 0, or why it is no image. */
#define IFHIP_VP8_DEC_CONTAINER 1        /* batch only: the RIFF container did not parse, or the file is animated        */
#define IFHIP_VP8_DEC_NOT_LOSSY 2        /* batch only: a lossless file (ifhip_webp_decode_batch_device reads those)      */
#define IFHIP_VP8_DEC_FRAME_HEADER 3     /* no shown key frame of profile 0..3 with its start code, or its header ends early */
#define IFHIP_VP8_DEC_PARTITIONS 4       /* the first partition or the table of partition sizes reaches beyond the chunk  */
#define IFHIP_VP8_DEC_END_OF_MODES 5     /* premature end of the first partition (segments, skip flags, modes)           */
#define IFHIP_VP8_DEC_END_OF_TOKENS 6    /* premature end of a token partition                                           */
#define IFHIP_VP8_DEC_ALPHA_HEADER 7     /* ALPH: a compression above 1, pre-processing above 1 or a reserved value      */
#define IFHIP_VP8_DEC_ALPHA_STREAM 8     /* ALPH: raw bytes fewer than the plane, or a VP8L stream that is no image       */
/* The synchronous host-buffer drop-in for WebPDecode(MODE_BGRA) on a lossy file: one file into `height` BGRA rows of `stride`
 * bytes at bgra (capacity bytes; bytes between rows are kept).  A non-zero status word comes back in *status (nullable) with
 * IFHIP_INVALID_ARGUMENT and an "ImageMalformed: libwebp decoding error" message; a lossless file is
 * IFHIP_METHOD_NOT_IMPLEMENTED with an "ImageTypeNotSupported" message. */
IFHIP_API int ifhip_webp_lossy_decode(const uint8_t* webp, size_t len, uint8_t* bgra, uint32_t stride, size_t capacity,
                                      uint32_t* status);

/* Device GIF decoder: what GifDecoder (imageflow_core/src/codecs/gif/mod.rs:21-309) hands on for one frame of a file -- the
 * logical screen after frames 0..frame_index were composed in order with their disposal (gif/screen.rs:25-95,
 * gif/disposal.rs:29-77), as BGRA with meaningful alpha.  The host walks the container (csrc/gif_read.cpp: header, screen,
 * colour tables, graphic control extensions, image descriptors, the data sub-blocks gathered into one LZW stream per frame;
 * unknown extensions are skipped, a missing trailer is the end of the file, mod.rs:123-129); the LZW streams are decoded
 * and the frames composed on the device (csrc/gif_decode.hip): segment-parallel, a segment being what lies between two
 * clear codes.
 * Known differences: the reference's LZW reader (the gif crate) is not on hand -- a stream that yields fewer indices than
 * width x height is refused (TOO_LITTLE) as Pillow refuses it; indices beyond width x height and bytes behind the end code
 * are ignored; a code that names an entry the table does not hold yet is BAD_CODE wherever it stands in the stream.
 * Every screen of an animation in one pass: ifhip_gif_decode_frames_device; the frames' count and timing: ifhip_gif_frame_count.
 *
 * Status word of a file (d_status[i]): 0, or why no frame was written. */
#define IFHIP_GIF_DEC_TOO_LITTLE 1       /* a frame's stream holds fewer indices than width x height            */
#define IFHIP_GIF_DEC_BAD_CODE 2         /* a code that names a table entry which does not exist yet            */
#define IFHIP_GIF_DEC_CONTAINER 3        /* no GIF signature / screen descriptor, a screen without pixels, a colour table cut short, an unknown block */
#define IFHIP_GIF_DEC_MIN_CODE_SIZE 4    /* a minimum code size outside 1..8                                    */
#define IFHIP_GIF_DEC_NO_PALETTE 5       /* a frame with neither a local nor a global colour table (screen.rs:52-57) */
#define IFHIP_GIF_DEC_FRAME_TOO_LARGE 6  /* a frame of more than 16 Mi indices (mod.rs:226-233)                 */
#define IFHIP_GIF_DEC_NO_SUCH_FRAME 7    /* frame_index beyond the file's last frame (mod.rs:217-224)           */
typedef struct ifhip_gif_file_info {
    uint32_t width, height;              /* the logical screen */
    uint32_t has_global_palette;
    uint32_t background_index;
} ifhip_gif_file_info;
/* The header's facts (what GifDecoder::create has read, mod.rs:45-101): no frame has been looked at, so a frame count is
 * not promised.  IFHIP_INVALID_ARGUMENT with an "ImageMalformed: GIF decoding error" message where the signature or the
 * screen descriptor is missing.  Host only, no device needed. */
IFHIP_API int ifhip_gif_info(const uint8_t* gif, size_t len, ifhip_gif_file_info* info);
/* n files (host memory) into n device frames of their logical screens' sizes: file i is decoded and composed up to frame
 * frame_index[i] (null: frame 0 of every file; GifDecoder::read_frame with SelectFrame, mod.rs:207-298).  d_frames[i] holds
 * height_i rows of strides[i] bytes inside frame_bytes[i]; only the 4 * width_i bytes of a row are written.  d_status[i]
 * (device) receives the file's status word; a damaged file leaves its frame untouched and never disturbs its neighbours.
 * Five launches per batch, every frame of every file in each.  The streams are uploaded before the call returns; the
 * kernels are asynchronous on hip_stream.  Argument and frame checks come before the device check. */
IFHIP_API int ifhip_gif_decode_batch_device(const uint8_t* const* files, const size_t* lens, uint32_t n_files, const uint32_t* frame_index,
                                            uint8_t* const* d_frames, const size_t* frame_bytes, const uint32_t* strides,
                                            uint32_t* d_status, void* hip_stream);
/* The synchronous host-buffer drop-in: frame `frame_index` of one file into `height` BGRA rows of `stride` bytes at bgra
 * (capacity bytes; bytes between rows are kept).  A non-zero status word comes back in *status (nullable) with
 * IFHIP_INVALID_ARGUMENT and an "ImageMalformed: GIF decoding error" message (NO_SUCH_FRAME: "InvalidArgument: frame=N
 * requested but GIF only has M frames"). */
IFHIP_API int ifhip_gif_decode(const uint8_t* gif, size_t len, uint32_t frame_index, uint8_t* bgra, uint32_t stride, size_t capacity,
                               uint32_t* status);
/* The walk of the container to its end (GifDecoder::has_more_frames until it says no, mod.rs:300-305): *n_frames, and for
 * the first `capacity` frames delays[k] (hundredths of a second) and flags[k] (the user-input flag) of their graphic control
 * extensions (both arrays nullable).  A file without a frame counts 0; a file the walk refuses is IFHIP_INVALID_ARGUMENT
 * with an "ImageMalformed: GIF decoding error" message, *n_frames the frames seen up to there.  Host only, no device needed. */
IFHIP_API int ifhip_gif_frame_count(const uint8_t* gif, size_t len, uint32_t* n_frames, uint32_t* delays, uint32_t* flags, uint32_t capacity);
/* Every composed screen of ONE file in one pass: screen k -- the logical screen behind Screen::blit of frame k, exactly what
 * ifhip_gif_decode(..., frame_index = k) gives -- lands at d_screens + k * screen_pitch as BGRA rows of `stride` bytes; only
 * 4 * width bytes of a row are written.  The block holds max_frames screens; a file of more frames is refused.  The LZW
 * launches are the batch's; the replay runs ONCE over the frame list and stores the pixel into screen k behind each blit.
 * A damaged frame anywhere fails the file: no screen is written, d_status[0] (device) holds the status word and
 * *n_frames_out is 0; otherwise *n_frames_out is the number of screens.  What the host walk finds is refused as
 * ifhip_gif_decode refuses it.  The call waits for hip_stream once, for the status word.  Argument and frame checks come
 * before the device check. */
IFHIP_API int ifhip_gif_decode_frames_device(const uint8_t* gif, size_t len, uint8_t* d_screens, size_t screen_pitch, uint32_t stride,
                                             uint32_t max_frames, uint32_t* d_status, uint32_t* n_frames_out, void* hip_stream);

/* Device GIF coder: EncoderPreset::Gif without the host: what GifEncoder::write_frame (imageflow_core/src/codecs/gif/mod.rs:385-592)
 * has the gif crate do -- one frame as a GIF89a file: the logical screen of the frame's size (size_16(): both sides at most
 * 65535) without a global colour table, an optional NETSCAPE2.0 block, a graphic control extension, the image with a local
 * colour table of at most 256 entries (padded with black to a power of two), no dithering -- on BGRA / BGRX frames that
 * stay in HBM.  A pixel of meaningful alpha below 16 becomes the transparent entry, which is then entry 0; every other
 * pixel counts as opaque.  The palette is this library's own (the integer quantiser of the palette PNG coder above, at its
 * defaults: target 100, minimum 0, speed 4): a frame of at most 256 distinct colours after the alpha rule keeps exactly
 * those; otherwise it is NOT the gif crate's NeuQuant palette.  The LZW stream carries a clear code every
 * IFHIP_GIF_ENC_SEGMENT_PIXELS pixels, so that a wave codes a segment on its own (csrc/gif_encode.hip); every reader takes
 * it.  N frames into one file: ifhip_gif_encode_animation_device.  Not built: dithering, frame differencing, a shared
 * palette.  A stage owns the scratch of a call in flight and is bound to ONE stream
 * at a time, like ifhip_png_quant_stage. */
#ifndef IFHIP_GIF_ENC_SEGMENT_PIXELS
#define IFHIP_GIF_ENC_SEGMENT_PIXELS 16384
#endif
#define IFHIP_GIF_FILE_OVERFLOW 1
typedef struct ifhip_gif_enc_stage ifhip_gif_enc_stage;
/* refused: zero dimensions, a side above 65535 ("InvalidArgument"), more than 2^28 pixels */
IFHIP_API int ifhip_gif_enc_stage_create(ifhip_gif_enc_stage** stage, uint32_t width, uint32_t height, uint32_t max_images);
IFHIP_API void ifhip_gif_enc_stage_destroy(ifhip_gif_enc_stage* stage);
/* a file_pitch with which no file overflows, by arithmetic alone: every pixel a 12-bit code, the clear codes of full tables
 * and of the segments, a length byte per 255 data bytes, the head with NETSCAPE2.0 and 256 entries, the tail */
IFHIP_API size_t ifhip_gif_enc_stage_max_file_bytes(const ifhip_gif_enc_stage* stage);
/* n_images frames as in ifhip_png_quantize_batch_device.  alpha_meaningful 0: every pixel is opaque (Bgr32).  repeat: the
 * loop count of the NETSCAPE2.0 block (0: for ever), -1: no block.  delay (hundredths of a second, 0..65535) and
 * needs_user_input go into the graphic control extension.  Image i's file goes to d_files + i * file_pitch and its length
 * to d_lengths[i] -- 0 when the file is longer than file_pitch, with IFHIP_GIF_FILE_OVERFLOW in d_status[i] (nullable).
 * Nullable taps: d_palettes (per image 256 RGBA entries in file order, then the count as a little-endian u32: 1028 bytes),
 * d_indices (per image width * height palette indices).  A fixed number of launches per batch; nothing is read back.
 * Asynchronous on hip_stream.  The same pixels give the same bytes on every run and in every batch position. */
IFHIP_API int ifhip_gif_encode_batch_device(ifhip_gif_enc_stage* stage, const uint8_t* d_images, size_t image_bytes, uint32_t stride,
                                            int alpha_meaningful, uint32_t n_images, int repeat, uint32_t delay, int needs_user_input,
                                            uint8_t* d_files, size_t file_pitch, uint32_t* d_lengths, uint32_t* d_status,
                                            uint8_t* d_palettes, uint8_t* d_indices, void* hip_stream);
/* A `capacity` with which no animation of n_frames frames overflows, by arithmetic alone: the head with NETSCAPE2.0, n_frames
 * times ifhip_gif_enc_stage_max_file_bytes, the trailer.  2^32 bytes or more: IFHIP_INVALID_ARGUMENT (byte offsets are 32 bits). */
IFHIP_API int ifhip_gif_enc_stage_max_animation_bytes(const ifhip_gif_enc_stage* stage, uint32_t n_frames, size_t* bytes);
/* n_frames frames (as the batch's images) into ONE GIF89a file at d_file (4-byte aligned, `capacity` bytes): the logical screen
 * of the frame size, no global table, NETSCAPE2.0 when repeat >= 0, then per frame a graphic control extension (delays[k],
 * user_input[k] -- both arrays in HOST memory, read before the call returns -- and the transparent entry if any), an image
 * descriptor at (0, 0) of the full size with a local colour table, and the frame's LZW data: exactly the bytes the one-frame
 * coder writes for that frame; then ';'.  A one-frame file is ifhip_gif_encode_batch_device's, byte for byte.  In a file of
 * more than one frame, frames of meaningful alpha carry disposal 2 (restore to background) -- the reference writes the gif
 * crate's Keep there (mod.rs:500-504), which lets frame k - 1 show through the transparent pixels of frame k; frames without
 * alpha carry Keep as the one-frame file does.  n_frames may exceed the stage's max_images: the stage then runs in chunks of
 * max_images frames with a running byte offset on the device, nothing is read back in between.  d_length[0]: the file's
 * length, 0 with IFHIP_GIF_FILE_OVERFLOW in d_status[0] (nullable) where it exceeds `capacity`.  Asynchronous on hip_stream
 * behind the upload of the two arrays. */
IFHIP_API int ifhip_gif_encode_animation_device(ifhip_gif_enc_stage* stage, const uint8_t* d_images, size_t image_bytes, uint32_t stride,
                                                int alpha_meaningful, uint32_t n_frames, int repeat, const uint32_t* delays,
                                                const uint8_t* user_input, uint8_t* d_file, size_t capacity, uint32_t* d_length,
                                                uint32_t* d_status, void* hip_stream);
/* The synchronous host-buffer form: one frame.  out == NULL: only *len (the size needed) is written. */
IFHIP_API int ifhip_gif_encode(const uint8_t* bgra, uint32_t width, uint32_t height, uint32_t stride, int alpha_meaningful, int repeat,
                               uint32_t delay, int needs_user_input, uint8_t* out, size_t capacity, size_t* len);

/* Host, for tests: what the device coder works from -- the Annex K Huffman tables in encode form (dc0, ac0, dc1, ac1; 256
 * entries `code | length << 16`) and the marker segments in front of the scan (SOI ... SOS). */
IFHIP_API int ifhip_jpeg_debug_encode_tables(uint32_t* tabs4x256, int n_components, const uint8_t* h_samp, const uint8_t* v_samp,
                                             uint32_t width, uint32_t height, int quality, uint8_t* header, size_t capacity,
                                             size_t* header_len);
/* Host, for tests: ifhip_jpeg_enc_stage_max_file_bytes_for without a stage (0: the geometry or the flags are refused). */
IFHIP_API size_t ifhip_jpeg_debug_enc_max_file_bytes_for(uint32_t width, uint32_t height, int n_components, const uint8_t* h_samp,
                                                         const uint8_t* v_samp, const uint32_t* blocks_w3, const uint32_t* blocks_h3,
                                                         int flags, size_t scan_capacity);

/* imageflow's 8x8 -> NxN spatial block scalers for the luma plane of a scaled decode: replaces
 * flow_scale_spatial[_srgb]_{1..7}x{1..7} (c_components/lib/codecs_jpeg_idct_fast.c, .h:17-43), the functions the IDCT
 * method selector installs for component 1 (codec_jpeg_wrapper.c:274-343).  `srgb` selects the linear-light variants.
 * Plane form: blocks_w x blocks_h blocks of 8x8 bytes in, n x n bytes out per block (device pointers).
 * Block form: host array [n_blocks][64] -> [n_blocks][n][n]. */
IFHIP_API int ifhip_scale_spatial_plane_device(const uint8_t* d_in, uint32_t in_pitch, uint32_t blocks_w,
                                               uint32_t blocks_h, int n, int srgb, uint8_t* d_out, uint32_t out_pitch,
                                               void* hip_stream);
IFHIP_API int ifhip_scale_spatial_blocks(const uint8_t* blocks, uint32_t n_blocks, int n, int srgb, uint8_t* out);
/* The tables behind them (rebuilt from populate_weights(Robidoux, n, 8) as tests/integration/variation.rs does):
 * int8 weights [7][8], log2 of each output's divisor [7], lut_srgb_to_linear[256], lut_linear_to_srgb[4096]. */
IFHIP_API int ifhip_block_scaler_tables(int n, int8_t* weights_7x8, uint8_t* log2_divisors_7,
                                        uint16_t* srgb_to_linear_256, uint8_t* linear_to_srgb_4096);

/* ---- Inner D: whole-bitmap operations around the resampler ------------- */
/* Byte-exact replacements for the bitmap primitives imageflow's graphs run between decode, resample and encode, so a
 * frame batch stays in HBM for the whole chain.  In-place unless a canvas is named; BGRA8, any 4-byte aligned stride.
 * Every *_batch_device call works on n_images equally shaped frames at a fixed byte pitch. */

/* graphics::color_matrix::window_bgra32_apply_color_matrix (graphics/color_matrix.rs:5-29): matrix25 = row-major
 * [[f32; 5]; 5] (host memory) as built by flow/nodes/color.rs:86-230 (ColorFilterSrgb; watermark opacity = Alpha(a),
 * flow/nodes/watermark.rs:165-172). */
IFHIP_API int ifhip_apply_color_matrix(uint8_t* bgra, uint32_t w, uint32_t h, uint32_t stride, const float* matrix25);
IFHIP_API int ifhip_apply_color_matrix_batch_device(uint8_t* d_bgra, size_t image_bytes, uint32_t n_images, uint32_t w,
                                                    uint32_t h, uint32_t stride, const float* matrix25, void* hip_stream);

/* graphics::copy_rect::copy_rectangle (graphics/copy_rect.rs:12-119; crop / clone / expand_canvas /
 * copy_rect_to_canvas, flow/nodes/clone_crop_fill_expand.rs).  Alpha bookkeeping as the reference: a Bgr32 canvas
 * receiving a Bgra32 input gets its alpha set to 255 and *canvas_alpha_meaningful = 1 (:47-54); a Bgr32 input copied
 * into a Bgra32 canvas has its own alpha set to 255 first (:64-66, the input bitmap is modified). */
IFHIP_API int ifhip_copy_rect(uint8_t* input, uint32_t in_w, uint32_t in_h, uint32_t in_stride, int in_alpha_meaningful,
                              uint8_t* canvas, uint32_t canvas_w, uint32_t canvas_h, uint32_t canvas_stride,
                              int* canvas_alpha_meaningful, uint32_t from_x, uint32_t from_y, uint32_t to_x,
                              uint32_t to_y, uint32_t w, uint32_t h);
IFHIP_API int ifhip_copy_rect_batch_device(uint8_t* d_in, size_t in_image_bytes, uint32_t in_w, uint32_t in_h,
                                           uint32_t in_stride, int in_alpha_meaningful, uint8_t* d_canvas,
                                           size_t canvas_image_bytes, uint32_t canvas_w, uint32_t canvas_h,
                                           uint32_t canvas_stride, int* canvas_alpha_meaningful, uint32_t from_x,
                                           uint32_t from_y, uint32_t to_x, uint32_t to_y, uint32_t w, uint32_t h,
                                           uint32_t n_images, void* hip_stream);

/* BitmapWindowMut::fill_rectangle (graphics/bitmaps.rs:1504-1548): [x1, x2) x [y1, y2) := color (Color32 0xAARRGGBB);
 * empty rectangles succeed, BlendWithMatte canvases only accept the full rectangle. */
IFHIP_API int ifhip_fill_rect(uint8_t* bgra, uint32_t w, uint32_t h, uint32_t stride, int compositing, uint32_t x1,
                              uint32_t y1, uint32_t x2, uint32_t y2, uint32_t color_bgra);
IFHIP_API int ifhip_fill_rect_batch_device(uint8_t* d_bgra, size_t image_bytes, uint32_t n_images, uint32_t w, uint32_t h,
                                           uint32_t stride, int compositing, uint32_t x1, uint32_t y1, uint32_t x2,
                                           uint32_t y2, uint32_t color_bgra, void* hip_stream);

/* BitmapWindowMut::normalize_unused_alpha (graphics/bitmaps.rs:1570-1576): alpha := 255 unless it is meaningful
 * (EnableTransparency, flow/nodes/enable_transparency.rs:70-84). */
IFHIP_API int ifhip_normalize_unused_alpha_batch_device(uint8_t* d_bgra, size_t image_bytes, uint32_t n_images, uint32_t w,
                                                        uint32_t h, uint32_t stride, int alpha_meaningful, void* hip_stream);

/* graphics::flip::flow_bitmap_bgra_flip_{vertical,horizontal}_safe (graphics/flip.rs:10-38); row padding stays. */
IFHIP_API int ifhip_flip_vertical(uint8_t* bgra, uint32_t w, uint32_t h, uint32_t stride);
IFHIP_API int ifhip_flip_horizontal(uint8_t* bgra, uint32_t w, uint32_t h, uint32_t stride);
IFHIP_API int ifhip_flip_vertical_batch_device(uint8_t* d_bgra, size_t image_bytes, uint32_t n_images, uint32_t w,
                                               uint32_t h, uint32_t stride, void* hip_stream);
IFHIP_API int ifhip_flip_horizontal_batch_device(uint8_t* d_bgra, size_t image_bytes, uint32_t n_images, uint32_t w,
                                                 uint32_t h, uint32_t stride, void* hip_stream);

/* graphics::transpose::bitmap_window_transpose (graphics/transpose.rs:95-121): to(y, x) = from(x, y); needs
 * from_w == to_h and from_h == to_w, distinct bitmaps (flow/nodes/rotate_flip_transpose.rs:150-153). */
IFHIP_API int ifhip_transpose(const uint8_t* from, uint32_t from_w, uint32_t from_h, uint32_t from_stride, uint8_t* to,
                              uint32_t to_w, uint32_t to_h, uint32_t to_stride);
IFHIP_API int ifhip_transpose_batch_device(const uint8_t* d_from, size_t from_image_bytes, uint32_t from_w,
                                           uint32_t from_h, uint32_t from_stride, uint8_t* d_to, size_t to_image_bytes,
                                           uint32_t to_w, uint32_t to_h, uint32_t to_stride, uint32_t n_images,
                                           void* hip_stream);

/* graphics::whitespace::detect_content (graphics/whitespace.rs:284-334, the search of :336-634): the content rectangle
 * x1, y1, x2, y2 of each frame -- exactly the reference's sequential windowed search, not a whole-frame box.  Grey as
 * approximate_grayscale: Bgra32 when alpha_meaningful, Bgr32 otherwise.  Frames narrower or shorter than 3 px and frames
 * without energy give the whole frame.  d_rects: 4 uint32 per frame on the device, written on hip_stream (scratch comes
 * from the library's stream cache).  The host form stages one bitmap and returns the rectangle in rect[4]. */
IFHIP_API int ifhip_detect_content(const uint8_t* bgra, uint32_t w, uint32_t h, uint32_t stride, int alpha_meaningful,
                                   uint32_t threshold, uint32_t* rect);
IFHIP_API int ifhip_detect_content_batch_device(const uint8_t* d_bgra, size_t image_bytes, uint32_t n_images, uint32_t w,
                                                uint32_t h, uint32_t stride, int alpha_meaningful, uint32_t threshold,
                                                uint32_t* d_rects, void* hip_stream);

/* graphics::rounded_corners::flow_bitmap_bgra_clear_around_rounded_corners (graphics/rounded_corners.rs:187-346; the pixel
 * work of RoundImageCornersMut, flow/nodes/round_corners.rs:56-93), in place: outside the rounded corners every pixel
 * becomes the matte's raw bytes, the anti-aliased ring blends the matte over the stored pixel in linear light.  mode is a
 * RoundCornersMode (imageflow_types lib.rs:1254-1268); radii[4] are in the JSON order top_left, top_right, bottom_right,
 * bottom_left (percentage / pixels / circle read radii[0] or nothing).  get_radius and plan_quadrants (:5-137) run on the
 * host in f32; one launch applies the four quadrants in the reference's order.  The caller sets the frame's compositing
 * to BlendWithSelf and, for a colour that is not opaque, runs EnableTransparency first (round_corners.rs:30-34, :72-73).
 * The host form stages one bitmap. */
typedef enum ifhip_round_corners_mode {
    IFHIP_ROUND_CORNERS_PERCENTAGE = 0, IFHIP_ROUND_CORNERS_PIXELS = 1, IFHIP_ROUND_CORNERS_CIRCLE = 2,
    IFHIP_ROUND_CORNERS_PERCENTAGE_CUSTOM = 3, IFHIP_ROUND_CORNERS_PIXELS_CUSTOM = 4
} ifhip_round_corners_mode;
IFHIP_API int ifhip_round_corners(uint8_t* bgra, uint32_t w, uint32_t h, uint32_t stride, int mode, const float* radii,
                                  uint32_t matte_bgra);
IFHIP_API int ifhip_round_corners_batch_device(uint8_t* d_bgra, size_t image_bytes, uint32_t n_images, uint32_t w,
                                               uint32_t h, uint32_t stride, int mode, const float* radii,
                                               uint32_t matte_bgra, void* hip_stream);

/* WhiteBalanceSrgbMutDef::mutate (flow/nodes/white_balance.rs:106-122, the maps of :13-93, the counts of
 * graphics/histogram.rs), in place: per frame, the R, G and B histograms, the area thresholds in f64 and the byte maps
 * applied to R, G and B (alpha keeps its value).  threshold: the node's Option<f32>, None being 0.006f.  d_histograms
 * (nullable, 8-byte aligned): receives the 3 x 256 counts of each frame, R then G then B, as uint64 [n_images][3][256];
 * otherwise the counts live in scratch from the library's stream cache.  Two launches on hip_stream, no host wait.  The
 * host form stages one bitmap; its `histograms` (nullable) is a host array of 768 counts. */
IFHIP_API int ifhip_white_balance(uint8_t* bgra, uint32_t w, uint32_t h, uint32_t stride, float threshold,
                                  uint64_t* histograms);
IFHIP_API int ifhip_white_balance_batch_device(uint8_t* d_bgra, size_t image_bytes, uint32_t n_images, uint32_t w,
                                               uint32_t h, uint32_t stride, float threshold, uint64_t* d_histograms,
                                               void* hip_stream);

/* ---- colour management: matrix/TRC sources to sRGB ------------------------------------------------------- */
/* What a conversion to sRGB needs (codecs/cms.rs::transform_to_srgb for SourceProfile::IccProfile and ::GammaPrimaries,
 * pinned to the reference's lcms2 back end, codecs/lcms2_transform.rs): the source's tone curves as linear light per byte
 * value, R then G then B, and the row-major matrix from source linear RGB to sRGB linear RGB (row = output R, G, B). */
typedef struct ifhip_color_plan {
    float linear[3][256];
    float matrix[9];
} ifhip_color_plan;
typedef enum ifhip_color_plan_status {
    IFHIP_COLOR_PLANNED = 0,          /* *out is filled */
    IFHIP_COLOR_NOT_CONVERTIBLE = 1,  /* a sound profile of a kind this library does not convert: GRAY / CMYK space, Lab PCS, LUT-based */
    IFHIP_COLOR_MALFORMED = 2         /* the bytes are no usable profile (the reference: ErrorKind::ColorProfileError) */
} ifhip_color_plan_status;
/* "planned" / "not convertible here" / "malformed" */
IFHIP_API const char* ifhip_color_plan_status_text(int status);
/* Replaces lcms2_transform.rs:219-242 (Profile::new_icc + Transform::new, Intent::Perceptual) for RGB matrix/TRC profiles,
 * v2 or v4, XYZ PCS: rXYZ / gXYZ / bXYZ as stored (lcms2's matrix-shaper does not consult chad or wtpt), rTRC / gTRC / bTRC
 * as curv (0 entries: identity, 1: a u8.8 gamma, n: a 16-bit table read with linear interpolation) or para (types 0..4);
 * matrix = inv(the colourants of lcms2's built-in sRGB profile, s15.16) x the source's, in f64, rounded to f32.  A profile
 * with an A2B0 / D2B0 tag is LUT-based for lcms2 even when matrix tags are present, and is not converted here.  Every tag is
 * bounds-checked against `len`.  Returns an ifhip_color_plan_status; other than PLANNED, ifhip_last_error_message() names the
 * case.  Host only. */
IFHIP_API int ifhip_color_plan_from_icc(const uint8_t* icc, size_t len, ifhip_color_plan* out);
/* Replaces lcms2_transform.rs:245-283 (cmsCreateRGBProfile from PNG gAMA + cHRM, SourceProfile::GammaPrimaries): the curve
 * x^(1/gamma), the primaries' RGB -> XYZ matrix adapted from the stated white to D50 with Bradford.  xy = white x, y, red
 * x, y, green x, y, blue x, y.  Values the reference rejects or takes for sRGB (source_profile.rs:225-242: a gamma that is
 * not positive and finite, a chromaticity that is not finite or has y = 0; a neutral gamma with sRGB's primaries) give the
 * plan that changes nothing (sRGB's curve, the identity matrix).  Primaries on one line are MALFORMED.  Host only. */
IFHIP_API int ifhip_color_plan_from_gamma_primaries(double gamma, const double xy[8], ifhip_color_plan* out);
/* codecs/cms.rs::transform_to_srgb on the device, in place: per pixel three table reads, the matrix in f32 (per row
 * fma(m2, b, fma(m1, g, m0 * r))), a clamp to [0, 1] with NaN -> 0 and LINEAR_TO_SRGB_LUT[(v * 16383) as usize]; the fourth
 * byte keeps its value.  Row padding is neither read as pixels nor written.  One launch on hip_stream, no host wait; the plan
 * is read during the call.  The host form stages one bitmap. */
IFHIP_API int ifhip_color_transform(uint8_t* bgra, uint32_t w, uint32_t h, uint32_t stride, const ifhip_color_plan* plan);
IFHIP_API int ifhip_color_transform_batch_device(uint8_t* d_bgra, size_t image_bytes, uint32_t n_images, uint32_t w,
                                                 uint32_t h, uint32_t stride, const ifhip_color_plan* plan,
                                                 void* hip_stream);

/* ---- measurement helpers (bench.py) -------------------------------------------------------------------- */
/* Runs `launches` back-to-back launches of the batch op on `hip_stream` bracketed by hipEvents on that stream
 * and returns the average milliseconds per launch. */
IFHIP_API int ifhip_time_scale_and_render_batch_device(const ifhip_resample_plan* plan,
                                                       const uint8_t* d_in, size_t in_image_bytes, uint32_t in_stride,
                                                       int in_alpha_meaningful, uint32_t n_images,
                                                       uint8_t* d_canvas, size_t canvas_image_bytes,
                                                       uint32_t canvas_w, uint32_t canvas_h, uint32_t canvas_stride,
                                                       uint32_t x, uint32_t y,
                                                       int working_space, int compositing, uint32_t matte_bgra,
                                                       int force_kernel, void* hip_stream, int launches,
                                                       float* avg_ms_per_launch);
/* device-to-device copy bandwidth probe (bytes read + bytes written per second), for the "measured roofline" note */
IFHIP_API int ifhip_measure_copy_bandwidth(size_t bytes, int iters, double* bytes_per_second);
/* read-only streaming probe (bytes read per second; 16-byte non-temporal loads, one XOR per load): the yardstick for
 * the resample kernel, whose traffic is 99.5 % reads */
IFHIP_API int ifhip_measure_read_bandwidth(size_t bytes, int iters, double* bytes_per_second);
/* the same with writes mixed in: one 16-byte vector stored per `read_vectors_per_write` vectors read (bytes read + written
 * per second) -- the yardstick for the moderate ratios, whose canvas stores are 15 - 36 % of their bytes: reads and writes
 * together run at 5.3 - 5.5 TB/s on MI355X where reads alone reach 7 */
IFHIP_API int ifhip_measure_mixed_bandwidth(size_t read_bytes, uint32_t read_vectors_per_write, int iters, double* bytes_per_second);

#ifdef __cplusplus
}
#endif
#endif /* IMAGEFLOW_HIP_H */
