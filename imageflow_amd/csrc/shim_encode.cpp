// shim_encode.cpp -- the encode stage of the ABI shim's job interpreter (Job, shim_job.hpp): the presets of an `encode` node as
// files -- JPEG (libjpeg_turbo, mozjpeg), PNG (libpng, pngquant), WebP (lossless, lossy), GIF (one frame or an animation's
// collected frames) and the raw BGRA container -- and the checks of a preset that run before the first node.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

#include "../../include/imageflow_hip_webp_lossy_enc.h"   // the device lossy WebP coder (vp8_encode.hip), in a header of its own
#include "shim_job.hpp"

namespace ifshim {
namespace {

// EncoderPreset::Mozjpeg's quality is an Option<u8>: the reference refuses the message when it is deserialised, before any
// node runs -- so every encode node's mozjpeg preset is looked at before the first node runs, and again where it is used
void check_mozjpeg_preset(const JVal* preset) {
    const JVal* moz = preset ? preset->get("mozjpeg") : nullptr;
    const JVal* q = moz ? moz->get("quality") : nullptr;
    if (q && q->t == JVal::Num && (q->n != std::floor(q->n) || q->n < 0.0 || q->n > 255.0))
        raise(kInvalidJson, "InvalidJson: encode.preset.mozjpeg.quality is an integer 0..255");
}
// EncoderPreset::WebPLossy is a struct variant with a required f32: the bare string, a missing or a non-numeric quality do
// not deserialise.  Looked at only where the context's lossy WebP encoder is on; -> the quality.
bool names_webplossy(const JVal* preset) {
    return preset && ((preset->t == JVal::Str && preset->s == "webplossy") || (preset->t == JVal::Obj && preset->get("webplossy")));
}
float check_webplossy_preset(const JVal* preset) {
    const JVal* lossy = preset->t == JVal::Obj ? preset->get("webplossy") : nullptr;
    const JVal* q = lossy && lossy->t == JVal::Obj ? lossy->get("quality") : nullptr;
    if (!q || q->t != JVal::Num) raise(kInvalidJson, "InvalidJson: encode.preset.webplossy.quality is a number");
    return static_cast<float>(q->n);
}

// The file a device coder writes for one frame: `pitch` bytes on the device, 16 to spare, and the coder's length and
// status words behind it at `tail` (the pitch, rounded up as the coder's caller chooses).
struct CodedFile {
    uint8_t* d = nullptr;
    uint32_t* d_len = nullptr;                                                   // length, status behind the file
    uint32_t len = 0, status = 0;
    ~CodedFile() { job_free(d); }
    hipError_t alloc(size_t pitch, size_t tail) {
        const hipError_t e = job_malloc(reinterpret_cast<void**>(&d), pitch + 16u);
        if (e == hipSuccess) d_len = reinterpret_cast<uint32_t*>(d + tail);
        return e;
    }
    void fetch(Io& o) {                                                          // after the coder's call; with status 0 the file goes into o.owned
        uint32_t len_status[2] = {0, 0};
        hip_check(static_cast<hipError_t>(ifhip::copy_to_host(len_status, d_len, 8)), "download(file length)");
        len = len_status[0]; status = len_status[1];
        if (status != 0 || len == 0) return;
        o.owned.assign(len, 0);
        hip_check(static_cast<hipError_t>(ifhip::copy_to_host(o.owned.data(), d, len)), "download(file)");
    }
};

// What a device coder's call in a job is named by: the label of its file's allocation, the coder in "dropped a file", the record.
struct CoderNames { const char *label, *coder, *mime, *ext; };
constexpr CoderNames kPngNames{"hipMalloc(png file)", "PNG", "image/png", "png"}, kPalettePngNames{"hipMalloc(png file)", "palette PNG", "image/png", "png"},
    kWebpNames{"hipMalloc(webp file)", "WebP", "image/webp", "webp"}, kGifNames{"hipMalloc(gif file)", "GIF", "image/gif", "gif"};

// Behind the stage: a file of `pitch` bytes, call(file) as the coder's one call on t_job_stream, and the file into `o`.
// Returns the status word: 0 with the file written, or `lets_through` (not 0), which the caller answers itself.
template <typename Call>
uint32_t fetch_coded_file(Job& j, Io& o, size_t pitch, const CoderNames& names, uint32_t lets_through, Call call) {
    CodedFile file;
    hip_check(file.alloc(pitch, pitch), names.label);
    check(call(file));
    j.poll_cancel();
    file.fetch(o);
    if (lets_through != 0 && file.status == lets_through) return file.status;
    if (file.status != 0 || file.len == 0) raise(kInternalError, "InternalError: the %s coder dropped a file sized for its worst case (status %u)", names.coder, file.status);
    o.written = true;
    return 0;
}
// One frame through a device file coder: create(&stage) for one image, a file of the stage's bound (rounded up to 16),
// batch(stage, d_file, pitch, d_len) (d_len + 1: the status word), the file into `o` and its record.
template <typename Stage, typename Create, typename Batch>
uint32_t write_coded_frame(Job& j, const FramePtr& f, Io& o, int32_t io_id, const CoderNames& names, uint32_t lets_through, Create create, void (*destroy)(Stage*),
                           size_t (*max_file_bytes)(const Stage*), Batch batch) {
    Stage* stage = nullptr;
    check(create(&stage));
    struct Guard { Stage* s; void (*destroy)(Stage*); ~Guard() { quiesce(); destroy(s); } } guard{stage, destroy};
    const size_t pitch = (max_file_bytes(stage) + 15u) & ~static_cast<size_t>(15u);
    const uint32_t status = fetch_coded_file(j, o, pitch, names, lets_through, [&](CodedFile& file) { return batch(stage, file.d, pitch, file.d_len); });
    if (status == 0) j.encodes.push_back({io_id, f->w, f->h, names.mime, names.ext});
    return status;
}
// the coefficients back to the host, Huffman coding and markers there (csrc/jpeg_write.cpp)
void write_jpeg_on_host(Job& j, const FramePtr& f, Io& o, int32_t io_id, const int16_t* d_coef, const size_t off[4], const uint32_t bw[3], const uint32_t bh[3],
                        const uint8_t hs[3], const uint8_t vs[3], int quality, int write_flags) {
    std::vector<int16_t> coef(off[3]);
    hip_check(static_cast<hipError_t>(ifhip::copy_to_host(coef.data(), d_coef, off[3] * 2u)), "download(coefficients)");
    size_t len = 0;
    o.owned.assign(std::max<size_t>(4096u, off[3]), 0);                          // a file is smaller than its coefficients: one pass
    int wrc = ifhip_jpeg_write(coef.data() + off[0], coef.data() + off[1], coef.data() + off[2], bw, bh, 3, hs, vs, f->w, f->h, quality, write_flags,
                               o.owned.data(), o.owned.size(), &len);
    if (wrc != IFHIP_OK && len > o.owned.size()) {
        o.owned.assign(len, 0);
        wrc = ifhip_jpeg_write(coef.data() + off[0], coef.data() + off[1], coef.data() + off[2], bw, bh, 3, hs, vs, f->w, f->h, quality, write_flags,
                               o.owned.data(), o.owned.size(), &len);
    }
    check(wrc);
    o.owned.resize(len);
    o.written = true;
    j.encodes.push_back({io_id, f->w, f->h, "image/jpeg", "jpg"});
}

}  // namespace

// a truecolour PNG of the frame by the device coder (csrc/png_encode.hip): only the file's bytes leave the device
void Job::write_png(const FramePtr& f, int color_type, int level, Io& o, int32_t io_id) {
    write_coded_frame(
        *this, f, o, io_id, kPngNames, 0u, [&](ifhip_png_enc_stage** s) { return ifhip_png_enc_stage_create(s, f->w, f->h, color_type, 1); }, ifhip_png_enc_stage_destroy,
        ifhip_png_enc_stage_max_file_bytes, [&](ifhip_png_enc_stage* s, uint8_t* d_file, size_t pitch, uint32_t* d_len) {
            return ifhip_png_encode_batch_device(s, dev(f), f->bytes(), f->stride, 1, level, d_file, pitch, d_len, d_len + 1, t_job_stream);
        });
}

// encode: EncoderPreset::LibjpegTurbo is written as a real JPEG (codecs/mozjpeg.rs:78-160, create_classic :62-77):
// apply_matte + forward DCT / quantisation on the device, the Huffman coder and the markers on the host
// (csrc/jpeg_write.cpp) -- baseline, with optimize_huffman_coding libjpeg's optimal tables, with progressive its
// standard scan script (:121-129).  The content-adaptive sampling choice
// (evalchroma, an external crate) is not reproduced: the file uses the maximum the reference allows (:133, 4:2:0).
// EncoderPreset::Libpng is written as a real PNG by the device coder (csrc/png_encode.hip), EncoderPreset::Pngquant as
// a palette PNG by the device quantiser (csrc/png_quantize.hip), or losslessly where it misses minimum_quality.
// EncoderPreset::WebPLossless is written as a real lossless WebP by the device coder (csrc/webp_encode.hip).
// EXTENSION: every other preset writes the raw BGRA container (lodepng / lossy WebP coders are out of scope) -- "gif" too,
// unless the context's GIF encoder is switched on (ifhip_shim_context_set_gif_encoder): then it is a GIF89a file of the device coder.
// EXTENSION (ifhip_shim_context_set_encoder_selection): EncoderPreset::Auto and ::Format are resolved to one of those coders
// (encode_selected, below); without the switch they are among the presets that write the raw container.
// `shared`: other consumers still read this frame -- the matte is then applied to a private copy.
void Job::encode(FramePtr f, int32_t io_id, const JVal* preset, bool shared) {
    Timed t(this, "primitive_encoder");
    Io& o = output(io_id);
    if (o.out_state == OutState::Taken) raise(kArgumentInvalid, "InvalidArgument: Output buffer for io_id %d has already been taken", io_id);
    poll_cancel();
    const bool selection = c->encoder_selection.load(std::memory_order_relaxed) && ifsel::names_selection(preset);
    if (anim.active) {                                                           // every frame to the "gif" nodes, frame 0 to every other encoder
        // (an `auto` / `format` preset that comes to GIF is a "gif" node: Job::animation_plan decided it before the first frame)
        const bool named_gif = preset && preset->t == JVal::Str && preset->s == "gif" && c->gif_encoder.load(std::memory_order_relaxed);
        if (named_gif || (selection && anim.selected_gif.count(io_id))) { collect_frame(f, io_id); return; }
        if (anim.k > 0) return;
    }
    if (selection) return encode_selected(f, o, io_id, preset, shared);
    const int coder = encode_coder(preset);
    // EncoderPreset::Mozjpeg {quality, progressive, matte} -> MozjpegEncoder::create (codecs/mozjpeg.rs:37-59): mozjpeg's own
    // defaults.  Of those the trellis quantisation is built (csrc/jpeg_trellis.hip, this project's restatement of
    // jcdctmgr.c quantize_trellis, AC only) between the raw forward stage and the device entropy coder; tables are always
    // optimised (:56) and the file always progressive (`progressive` only ever switches it on, :121-125, over defaults
    // that already are).  Annex K tables, libjpeg's standard scan script, no deringing, 4:2:0.
    const bool moz = coder == IFHIP_ENCODE_CODER_MOZJPEG;
    const JVal* classic = coder == IFHIP_ENCODE_CODER_JPEG ? preset->get("libjpeg_turbo") : moz ? preset->get("mozjpeg") : nullptr;
    if (classic) return encode_jpeg(f, o, io_id, preset, classic, moz, shared);
    if (const JVal* png = coder == IFHIP_ENCODE_CODER_PNG ? preset->get("libpng") : nullptr) return encode_png(f, o, io_id, png, shared);
    if (const JVal* pq = coder == IFHIP_ENCODE_CODER_PNGQUANT ? preset->get("pngquant") : nullptr) return encode_pngquant(f, o, io_id, pq);
    if (coder == IFHIP_ENCODE_CODER_WEBP_LOSSLESS) return encode_webp_lossless(f, o, io_id);
    if (preset && preset->t == JVal::Str && preset->s == "gif" && c->gif_encoder.load(std::memory_order_relaxed)) return encode_gif(f, o, io_id);
    if (names_webplossy(preset) && c->webp_lossy_encoder.load(std::memory_order_relaxed)) return encode_webp_lossy(f, o, io_id, preset);
    encode_raw(f, o, io_id);
}

// the libjpeg_turbo and mozjpeg presets: `classic` is the preset's object
void Job::encode_jpeg(FramePtr f, Io& o, int32_t io_id, const JVal* preset, const JVal* classic, bool moz, bool shared) {
    auto flag = [&](const char* k) { const JVal* v = classic->get(k); return v && v->t == JVal::Bool && v->b; };
    const int write_flags = moz ? (IFHIP_JPEG_PROGRESSIVE | IFHIP_JPEG_OPTIMIZE_HUFFMAN)
                                : (flag("progressive") ? IFHIP_JPEG_PROGRESSIVE : 0) | (flag("optimize_huffman_coding") ? IFHIP_JPEG_OPTIMIZE_HUFFMAN : 0);
    const JVal* q = classic->get("quality");
    int quality = 75;                                                            // mozjpeg.rs:32 DEFAULT_QUALITY
    if (moz) check_mozjpeg_preset(preset);
    if (moz && q && q->t == JVal::Num) quality = std::min(100, static_cast<int>(q->n));   // Option<u8> -> u8::min(100, ..) (mozjpeg.rs:53)
    // Option<i32> -> `q as u8` (codecs/auto.rs:201: the value WRAPS, 300 is 44 and -5 is 251) -> u8::min(100, ..) (mozjpeg.rs:71)
    if (!moz && q && q->t == JVal::Num) {
        if (q->n != std::floor(q->n) || q->n < -2147483648.0 || q->n > 2147483647.0) raise(kInvalidJson, "InvalidJson: encode.preset.libjpeg_turbo.quality is a 32-bit integer");
        quality = std::min(100, static_cast<int>(static_cast<uint8_t>(static_cast<int32_t>(q->n))));
    }
    const JVal* m = classic->get("matte");
    const uint32_t matte = m && !m->is_null() ? parse_color(m, moz ? "encode.preset.mozjpeg.matte" : "encode.preset.libjpeg_turbo.matte") : 0xFFFFFFFFu;   // :88-92
    if (shared && f->alpha) f = clone(f);
    check(ifhip_apply_matte_batch_device(dev(f), f->bytes(), 1, f->w, f->h, f->stride, f->alpha ? 1 : 0, matte, t_job_stream));
    f->alpha = false;                                                            // :94 set_alpha_meaningful(false)
    const uint8_t hs[3] = {2, 1, 1}, vs[3] = {2, 1, 1};
    uint16_t qt2[2][64], qt3[3][64];
    ifhip_jpeg_quality_tables(quality, &qt2[0][0]);
    std::memcpy(qt3[0], qt2[0], 128); std::memcpy(qt3[1], qt2[1], 128); std::memcpy(qt3[2], qt2[1], 128);
    ifhip_jpeg_fwd_stage* st = nullptr;
    check(ifhip_jpeg_fwd_stage_create(&st, f->w, f->h, hs, vs, 1));
    std::unique_ptr<ifhip_jpeg_fwd_stage, void (*)(ifhip_jpeg_fwd_stage*)> st_guard(st, ifhip_jpeg_fwd_stage_destroy);
    uint32_t bw[3], bh[3];
    check(ifhip_jpeg_fwd_stage_block_dims(st, bw, bh));
    size_t off[4] = {0, 0, 0, 0};
    for (int k = 0; k < 3; ++k) off[k + 1] = off[k] + static_cast<size_t>(bw[k]) * bh[k] * 64u;
    int16_t* d_coef = nullptr;
    uint16_t* d_qt = nullptr;
    // (the mozjpeg preset: the raw planes of the trellis stage lie behind the quantised ones)
    hip_check(job_malloc(reinterpret_cast<void**>(&d_coef), off[3] * (moz ? 4u : 2u) + 384u), "hipMalloc(coefficients)");
    std::unique_ptr<int16_t, void (*)(int16_t*)> coef_guard(d_coef, [](int16_t* p) { job_free(p); });
    int16_t* d_raw = d_coef + off[3];
    d_qt = reinterpret_cast<uint16_t*>(d_coef + off[3] * (moz ? 2u : 1u));
    hip_check(static_cast<hipError_t>(ifhip::copy_to_device(d_qt, qt3, 384)), "upload(quant tables)");
    if (moz) {
        ifhip_jpeg_trellis_stage* ts = nullptr;
        check(ifhip_jpeg_trellis_stage_create(&ts, f->w, f->h, hs, vs, 1));
        std::unique_ptr<ifhip_jpeg_trellis_stage, void (*)(ifhip_jpeg_trellis_stage*)> ts_guard(ts, [](ifhip_jpeg_trellis_stage* q) { quiesce(); ifhip_jpeg_trellis_stage_destroy(q); });
        check(ifhip_jpeg_forward_raw_batch_device(st, dev(f), f->bytes(), f->stride, 1, d_raw + off[0], d_raw + off[1], d_raw + off[2], t_job_stream));
        check(ifhip_jpeg_trellis_batch_device(ts, d_raw + off[0], d_raw + off[1], d_raw + off[2], d_qt, IFHIP_JPEG_TRELLIS_LAMBDA_ONE, 1, d_coef + off[0],
                                              d_coef + off[1], d_coef + off[2], t_job_stream));
    } else {
        check(ifhip_jpeg_forward_batch_device(st, dev(f), f->bytes(), f->stride, d_qt, 1, d_coef + off[0], d_coef + off[1], d_coef + off[2], t_job_stream));
    }
    poll_cancel();
    // (the mozjpeg preset goes to the device coder without the switch: that guards what older callers pinned for libjpeg_turbo)
    if (write_flags == 0 || moz || c->device_jpeg_options.load(std::memory_order_relaxed)) {
        // the preset's default (baseline, Annex K tables) -- and, where the caller switched it on
        // (ifhip_shim_context_set_device_jpeg_options), progressive / optimize_huffman_coding:
        // the device entropy coder -- only the file leaves the device.
        // First with room for a scan half the size of its coefficients (what the host path assumes too), then, for an
        // image that is denser than that, with the geometry's worst case.
        for (int attempt = 0; attempt < 2; ++attempt) {
            const size_t scan_cap = attempt == 0 ? std::max<size_t>(65536u, off[3]) : 0u;
            // A geometry the coder does not take (more than 2.58 M blocks: a `security` override above ~110 MP) or a
            // stage that cannot be allocated is not the job's failure: the host writer below codes the same file.
            ifhip_jpeg_enc_stage* es = nullptr;
            if (ifhip_jpeg_enc_stage_create(&es, f->w, f->h, 3, hs, vs, bw, bh, 1, scan_cap) != IFHIP_OK) break;
            std::unique_ptr<ifhip_jpeg_enc_stage, void (*)(ifhip_jpeg_enc_stage*)> es_guard(es, [](ifhip_jpeg_enc_stage* q) { quiesce(); ifhip_jpeg_enc_stage_destroy(q); });
            const size_t pitch = ifhip_jpeg_enc_stage_max_file_bytes_for(es, write_flags);
            if (pitch == 0) break;                                               // (the flagged forms refuse the geometry)
            CodedFile file;
            if (file.alloc(pitch, (pitch + 3u) & ~static_cast<size_t>(3u)) != hipSuccess) break;
            // (a flagged call allocates its scratch first; where that fails the host writer codes the file)
            const int erc = ifhip_jpeg_encode_flags_batch_device(es, d_coef + off[0], d_coef + off[1], d_coef + off[2], quality, write_flags, 1, file.d,
                                                                 pitch, file.d_len, file.d_len + 1, t_job_stream);
            if (erc != IFHIP_OK && write_flags != 0) break;
            check(erc);
            file.fetch(o);
            if (file.status & IFHIP_ENC_BAD_COEFFICIENT)
                raise(kArgumentInvalid, "InvalidArgument: coefficient out of range for 8-bit JPEG (more than 11 DC / 10 AC magnitude bits)");
            if (file.status != 0) continue;
            o.written = true;
            encodes.push_back({io_id, f->w, f->h, "image/jpeg", "jpg"});
            c->device_coded_files.fetch_add(1, std::memory_order_relaxed);
            return;
        }
    }                                                                            // (not coded on the device: the host writer)
    write_jpeg_on_host(*this, f, o, io_id, d_coef, off, bw, bh, hs, vs, quality, write_flags);
}
void Job::encode_png(FramePtr f, Io& o, int32_t io_id, const JVal* png, bool shared) {
    // EncoderPreset::Libpng {depth, matte, zlib_compression} (imageflow_types/src/lib.rs:751-755, codecs/auto.rs:241-268)
    // -> LibPngEncoder::write_frame (codecs/libpng_encoder.rs:43-72): the file is coded on the device
    // (csrc/png_encode.hip), only its bytes leave it.
    int color_type = -1;                                                         // by the frame's alpha, below
    if (const JVal* d = png->get("depth"); d && !d->is_null()) {
        if (d->t != JVal::Str || (d->s != "png_32" && d->s != "png_24")) raise(kInvalidJson, "InvalidJson: encode.preset.libpng.depth is \"png_32\" or \"png_24\"");
        if (d->s == "png_24") color_type = IFHIP_PNG_RGB;
    }
    int level = -1;                                                              // absent: zlib's default (6)
    if (const JVal* z = png->get("zlib_compression"); z && !z->is_null()) {
        if (z->t != JVal::Num || z->n != std::floor(z->n) || z->n < -2147483648.0 || z->n > 2147483647.0)
            raise(kInvalidJson, "InvalidJson: encode.preset.libpng.zlib_compression is a 32-bit integer");
        // i32 clamped to 0..255 (auto.rs:265); above 9 libpng is left at its default (codec_png_wrapper.c:380-387)
        const int v = static_cast<int>(std::min(255.0, std::max(0.0, z->n)));
        level = v > 9 ? -1 : v;
    }
    const JVal* m = png->get("matte");
    if (m && !m->is_null() && f->alpha) {                                       // libpng_encoder.rs:55-57, bitmaps.rs:528-541
        const uint32_t matte = parse_color(m, "encode.preset.libpng.matte");
        if (shared) f = clone(f);
        check(ifhip_apply_matte_batch_device(dev(f), f->bytes(), 1, f->w, f->h, f->stride, 1, matte, t_job_stream));
        if ((matte >> 24) == 0xFFu) f->alpha = false;                            // matte.is_opaque(): set_alpha_meaningful(false)
    } else if (m && !m->is_null()) {
        (void)parse_color(m, "encode.preset.libpng.matte");                      // (still parsed: a malformed colour is an error)
    }
    if (color_type < 0) color_type = f->alpha ? IFHIP_PNG_RGBA : IFHIP_PNG_RGB;  // codec_png_wrapper.c:402-410
    write_png(f, color_type, level, o, io_id);
}
void Job::encode_pngquant(const FramePtr& f, Io& o, int32_t io_id, const JVal* pq) {
    // EncoderPreset::Pngquant {quality, minimum_quality, speed, maximum_deflate} (imageflow_types/src/lib.rs:756-761)
    // -> PngquantEncoder (codecs/pngquant.rs:35-139): quantised, dithered and written as a palette PNG on the device
    // (csrc/png_quantize.hip); no matte (codecs/auto.rs:98-110).  The three numbers are u8.
    auto u8_option = [&](const char* key) -> int {
        const JVal* v = pq->get(key);
        if (!v || v->is_null()) return -1;
        if (v->t != JVal::Num || v->n != std::floor(v->n) || v->n < 0.0 || v->n > 255.0) raise(kInvalidJson, "InvalidJson: encode.preset.pngquant.%s is an integer in 0..255", key);
        return static_cast<int>(v->n);
    };
    const int quality = u8_option("quality"), min_quality = u8_option("minimum_quality"), speed = u8_option("speed");
    bool maximum_deflate = false;
    if (const JVal* z = pq->get("maximum_deflate"); z && !z->is_null()) {
        if (z->t != JVal::Bool) raise(kInvalidJson, "InvalidJson: encode.preset.pngquant.maximum_deflate is a boolean");
        maximum_deflate = z->b;
    }
    const int level = maximum_deflate ? 9 : 6;                                    // lode.rs:162-195
    const uint32_t status = write_coded_frame(
        *this, f, o, io_id, kPalettePngNames, IFHIP_PNG_QUALITY_TOO_LOW, [&](ifhip_png_quant_stage** s) { return ifhip_png_quant_stage_create(s, f->w, f->h, 1); },
        ifhip_png_quant_stage_destroy, ifhip_png_quant_stage_max_file_bytes, [&](ifhip_png_quant_stage* s, uint8_t* d_file, size_t pitch, uint32_t* d_len) {
            return ifhip_png_quantize_batch_device(s, dev(f), f->bytes(), f->stride, f->alpha ? 1 : 0, 1, quality, min_quality, speed, 256, 1, level, d_file, pitch,
                                                   d_len, d_len + 1, nullptr, nullptr, nullptr, t_job_stream);
        });
    // pngquant.rs:105-139: below minimum_quality the frame is written losslessly, RGBA or RGB by its alpha
    if (status == IFHIP_PNG_QUALITY_TOO_LOW) write_png(f, f->alpha ? IFHIP_PNG_RGBA : IFHIP_PNG_RGB, level, o, io_id);
}
void Job::encode_webp_lossless(const FramePtr& f, Io& o, int32_t io_id) {
    // EncoderPreset::WebPLossless (imageflow_types/src/lib.rs:773, codecs/auto.rs:282-319) -> WebPEncoder::write_frame
    // (codecs/webp.rs:281-345: WebPEncodeLosslessBGRA, or ...BGR when the frame's alpha is not meaningful); no matte
    // (the reference passes None).  The file is coded on the device (csrc/webp_encode.hip), only its bytes leave it.
    // The stage is made per frame with the context's flags (ifhip_shim_context_set_webp_lossless_flags), so none outlives a change of them.
    const uint32_t flags = c->webp_lossless_flags.load(std::memory_order_relaxed);
    write_coded_frame(
        *this, f, o, io_id, kWebpNames, 0u, [&](ifhip_webp_enc_stage** s) { return ifhip_webp_enc_stage_create_flags(s, f->w, f->h, f->alpha ? 1 : 0, 1, flags); },
        ifhip_webp_enc_stage_destroy, ifhip_webp_enc_stage_max_file_bytes, [&](ifhip_webp_enc_stage* s, uint8_t* d_file, size_t pitch, uint32_t* d_len) {
            return ifhip_webp_encode_batch_device(s, dev(f), f->bytes(), f->stride, 1, d_file, pitch, d_len, d_len + 1, t_job_stream);
        });
}
void Job::encode_gif(const FramePtr& f, Io& o, int32_t io_id) {
    // EXTENSION (ifhip_shim_context_set_gif_encoder): EncoderPreset::Gif -> GifEncoder::write_frame (codecs/gif/mod.rs:385-592):
    // the alpha rule, the palette and the LZW stream on the device (csrc/gif_encode.hip), only the file leaves it.  The
    // frame itself is left as it is (the rule is applied where the pixels are read); a side above 65535 is size_16()'s
    // InvalidArgument.  A GIF decoder of the job hands on its repeat count and its last frame's delay and user-input flag.
    write_coded_frame(
        *this, f, o, io_id, kGifNames, 0u, [&](ifhip_gif_enc_stage** s) { return ifhip_gif_enc_stage_create(s, f->w, f->h, 1); }, ifhip_gif_enc_stage_destroy,
        ifhip_gif_enc_stage_max_file_bytes, [&](ifhip_gif_enc_stage* s, uint8_t* d_file, size_t pitch, uint32_t* d_len) {
            return ifhip_gif_encode_batch_device(s, dev(f), f->bytes(), f->stride, f->alpha ? 1 : 0, 1, gif_source.seen ? gif_source.repeat : -1, gif_source.delay,
                                                 gif_source.user_input ? 1 : 0, d_file, pitch, d_len, d_len + 1, nullptr, nullptr, t_job_stream);
        });
}
void Job::encode_webp_lossy(const FramePtr& f, Io& o, int32_t io_id, const JVal* preset) {
    // EXTENSION (ifhip_shim_context_set_webp_lossy_encoder): EncoderPreset::WebPLossy {quality} -> WebPEncoder::write_frame
    // (codecs/webp.rs: WebPEncodeBGRA, or ...BGR when the frame's alpha is not meaningful; quality clamped to 0..100); no matte.
    // The file is coded on the device (csrc/vp8_encode.hip), only its bytes leave it.  libwebp returns nothing for a side
    // above 16383, which the reference answers with ImageEncodingError.  The switch's value 2 adds the 4x4 luma modes.
    const float quality = check_webplossy_preset(preset);
    const uint32_t flags = c->webp_lossy_intra4.load(std::memory_order_relaxed) ? IFHIP_VP8_ENC_INTRA4 : 0u;
    if (f->w > 16383u || f->h > 16383u) raise(kInternalError, "ImageEncodingError: libwebp encoding error");
    write_coded_frame(
        *this, f, o, io_id, kWebpNames, 0u, [&](ifhip_webp_lossy_enc_stage** s) { return ifhip_webp_lossy_enc_stage_create_flags(s, f->w, f->h, f->alpha ? 1 : 0, 1, flags); },
        ifhip_webp_lossy_enc_stage_destroy, ifhip_webp_lossy_enc_stage_max_file_bytes, [&](ifhip_webp_lossy_enc_stage* s, uint8_t* d_file, size_t pitch, uint32_t* d_len) {
            return ifhip_webp_lossy_encode_batch_device(s, dev(f), f->bytes(), f->stride, 1, quality, d_file, pitch, d_len, d_len + 1, t_job_stream);
        });
}
// EXTENSION: the raw BGRA container
void Job::encode_raw(const FramePtr& f, Io& o, int32_t io_id) {
    o.owned.assign(kRawHeader + f->bytes(), 0);
    std::memcpy(o.owned.data(), kRawMagic, 8);
    const uint32_t hdr[4] = {f->w, f->h, f->stride, f->alpha ? 1u : 0u};
    std::memcpy(o.owned.data() + 8, hdr, 16);
    { uint8_t* src = dev(f); hip_check(static_cast<hipError_t>(ifhip::copy_to_host(o.owned.data() + kRawHeader, src, f->bytes())), "download(frame)"); }
    o.written = true;
    encodes.push_back({io_id, f->w, f->h, "application/x-imageflow-bgra", "ifbgra"});
}

// EXTENSION (ifhip_shim_context_set_encoder_selection): EncoderPreset::Auto / ::Format -> create_encoder_auto (codecs/auto.rs:
// 368-566): the preset is resolved against the job's source (Job::find_source) and this frame (csrc/encoder_select.cpp), and the
// coder that comes out writes the file with the parameters of its named preset.  A resolved preset never writes the raw
// container, and it does not ask for the GIF or lossy WebP switches.  `jpegli` is the mozjpeg route; webp_m, jpeg_xyb and
// color_profiles have nothing to act on here (DESIGN "Encoder selection").
void Job::encode_selected(FramePtr f, Io& o, int32_t io_id, const JVal* preset, bool shared) {
    const ifsel::Resolved r = ifsel::resolve(ifsel::read_preset(*preset), has_source_io ? source_facts(source_io) : ifsel::Source(), f->alpha, f->w, f->h);
    const std::string json = ifsel::resolved_json(r);
    const JVal resolved = parse_json(reinterpret_cast<const uint8_t*>(json.data()), json.size());
    const JVal* params = resolved.get("params");
    auto named = [&](const char* name) { JVal v; v.t = JVal::Obj; v.o.emplace_back(name, *params); return v; };
    switch (r.coder) {
    case ifsel::kCoderMozjpeg: { const JVal p = named("mozjpeg"); return encode_jpeg(f, o, io_id, &p, &p.o[0].second, true, shared); }
    case ifsel::kCoderLibjpegTurbo: { const JVal p = named("libjpeg_turbo"); return encode_jpeg(f, o, io_id, &p, &p.o[0].second, false, shared); }
    case ifsel::kCoderLibpng: return encode_png(f, o, io_id, params, shared);
    case ifsel::kCoderLodepng:                                                  // lode.rs:51-53, 98-104: the matte, then BGRA or BGRX by the frame's alpha
        f = matted(f, r, shared);
        return write_png(f, f->alpha ? IFHIP_PNG_RGBA : IFHIP_PNG_RGB, r.maximum_deflate == 1 ? 9 : -1, o, io_id);
    case ifsel::kCoderPngquant: return encode_pngquant(matted(f, r, shared), o, io_id, params);   // pngquant.rs:74
    case ifsel::kCoderWebpLossless: return encode_webp_lossless(matted(f, r, shared), o, io_id);  // webp.rs:292
    case ifsel::kCoderWebpLossy: { const JVal p = named("webplossy"); return encode_webp_lossy(matted(f, r, shared), o, io_id, &p); }
    default: return encode_gif(f, o, io_id);                                    // (GifEncoder::create takes no matte, auto.rs:392-395)
    }
}
// The preset's matte before a coder that takes one, as encode_jpeg and encode_png treat theirs: Bitmap::apply_matte
// (bitmaps.rs:528-541) in place -- on a private copy where other consumers still read the frame -- and an opaque matte ends
// the alpha's meaning.
FramePtr Job::matted(FramePtr f, const ifsel::Resolved& r, bool shared) {
    if (!r.has_matte || !f->alpha) return f;
    if (shared) f = clone(f);
    check(ifhip_apply_matte_batch_device(dev(f), f->bytes(), 1, f->w, f->h, f->stride, 1, r.matte, t_job_stream));
    if ((r.matte >> 24) == 0xFFu) f->alpha = false;
    return f;
}

void Job::check_encode_node(const JVal& n) {
    if (n.t != JVal::Obj || n.o.size() != 1 || n.o[0].first != "encode") return;
    const JVal* preset = n.o[0].second.get("preset");
    // (serde refuses the message before any node runs: a missing required field, a wrong type, an unknown variant)
    if (c->encoder_selection.load(std::memory_order_relaxed) && ifsel::names_selection(preset)) (void)ifsel::read_preset(*preset);
    if (encode_coder(preset) == IFHIP_ENCODE_CODER_MOZJPEG) check_mozjpeg_preset(preset);
    if (names_webplossy(preset) && c->webp_lossy_encoder.load(std::memory_order_relaxed)) (void)check_webplossy_preset(preset);
}

// a "gif" encode node in run k: its input joins the node's block
void Job::collect_frame(const FramePtr& f, int32_t io_id) {
    std::unique_ptr<AnimCollect>& slot = anim.collects[io_id];
    if (anim.k == 0) {
        if (slot) raise(kArgumentInvalid, "InvalidArgument: io_id %d is written by two encode nodes", io_id);
        slot = std::make_unique<AnimCollect>();
        check(ifhip_gif_enc_stage_create(&slot->stage, f->w, f->h, std::min(anim.n, 32u)));   // (size_16(): a side above 65535 is refused here)
        add_animation_pixels(static_cast<uint64_t>(f->w) * f->h);                  // before the block is allocated
        slot->w = f->w; slot->h = f->h; slot->stride = f->stride; slot->alpha = f->alpha;
        hip_check(job_malloc(reinterpret_cast<void**>(&slot->d), f->bytes() * anim.n + 64), "hipMalloc(collected frames)");
        encodes.push_back({io_id, f->w, f->h, "image/gif", "gif"});
    }
    if (!slot || slot->w != f->w || slot->h != f->h || slot->stride != f->stride || slot->alpha != f->alpha)
        raise(kArgumentInvalid, "InvalidArgument: frame %u reaches the GIF encoder of io_id %d as %ux%u, frame 0 was %ux%u", anim.k, io_id, f->w, f->h, slot ? slot->w : 0u,
              slot ? slot->h : 0u);
    hip_check(hipMemcpyAsync(slot->d + static_cast<size_t>(anim.k) * f->bytes(), dev(f), f->bytes(), hipMemcpyDeviceToDevice, t_job_stream), "copy(collected frame)");
}
void Job::write_animations() {
    for (auto& kv : anim.collects) {
        Timed t(this, "primitive_encoder");
        AnimCollect& a = *kv.second;
        Io& o = output(kv.first);
        size_t capacity = 0;
        check(ifhip_gif_enc_stage_max_animation_bytes(a.stage, anim.n, &capacity));
        const size_t pitch = (capacity + 15u) & ~static_cast<size_t>(15u);
        const size_t image_bytes = static_cast<size_t>(a.h) * a.stride;
        fetch_coded_file(*this, o, pitch, kGifNames, 0u, [&](CodedFile& file) {
            return ifhip_gif_encode_animation_device(a.stage, a.d, image_bytes, a.stride, a.alpha ? 1 : 0, anim.n, anim.repeat, anim.delays.data(), anim.user_input.data(), file.d,
                                                     capacity, file.d_len, file.d_len + 1, t_job_stream);
        });
    }
}

}  // namespace ifshim
