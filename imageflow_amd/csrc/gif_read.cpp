// gif_read.cpp -- the host side of the GIF decoder: the walk of the container, what the gif crate's reader does for the
// reference (imageflow_core/src/codecs/gif/mod.rs:45-131; sniffed at codecs/mod.rs by "GIF87a" / "GIF89a").  The rules:
//   * header, logical screen descriptor, global colour table; the background colour is Screen::new's (gif/screen.rs:29-37):
//     the global table's entry at the background index with alpha 255, (0,0,0,0) without a table or beyond it;
//   * a graphic control extension (0x21 0xF9, four bytes) belongs to the next image: disposal (values above 3 are Keep, the
//     frame's default), the transparent index where its flag is set, delay, user input;
//   * every other extension is skipped, whatever its label (allow_unknown_blocks(true), mod.rs:47); of a NETSCAPE2.0
//     application extension the loop count is noted on the way (the GIF coder of a job writes it again);
//   * an image: descriptor, local colour table, minimum code size, and the data sub-blocks gathered into ONE contiguous LZW
//     stream; sub-blocks cut short by the end of the file give what they hold, and the LZW stage decides whether that is enough;
//   * the end of the file in front of or inside the next frame's header is the end of the stream, trailer or not
//     (mod.rs:123-129); a block that is none of 0x21, 0x2C, 0x3B is IFHIP_GIF_DEC_CONTAINER;
//   * the walk stops behind the frame the job needs;
//   * limits: a minimum code size outside 1..8, a frame of more than 16 Mi indices (mod.rs:226-233), a frame with no colour
//     table at all (screen.rs:52-57) are status words.
// Host only: nothing here needs a device, and tests/gif_decode_emulate.cpp and tools/sanitize/gif_fuzz.cpp compile this file
// as it is.
#include "gif_read.hpp"

#include <algorithm>
#include <cstring>

#include "common.hpp"

namespace ifhip {
namespace {

uint32_t le16(const uint8_t* p) { return static_cast<uint32_t>(p[0]) | static_cast<uint32_t>(p[1]) << 8; }

void read_table(const uint8_t* p, uint32_t n, std::vector<uint32_t>* out) {
    for (uint32_t i = 0; i < n; ++i)
        out->push_back(0xFF000000u | static_cast<uint32_t>(p[3u * i]) << 16 | static_cast<uint32_t>(p[3u * i + 1u]) << 8 | p[3u * i + 2u]);
}

}  // namespace

int parse_gif_header(const uint8_t* d, size_t len, GifParsed* out) {
    *out = GifParsed();
    if (!d || len < 13u || (std::memcmp(d, "GIF87a", 6) != 0 && std::memcmp(d, "GIF89a", 6) != 0))
        return fail(IFHIP_INVALID_ARGUMENT, "ImageMalformed: GIF decoding error (no GIF signature and logical screen descriptor)");
    out->w = le16(d + 6); out->h = le16(d + 8);
    out->has_global = (d[10] & 0x80u) != 0u;
    out->global_n = out->has_global ? 2u << (d[10] & 7u) : 0u;
    out->bg_index = d[11];
    return IFHIP_OK;
}

int parse_gif(const uint8_t* d, size_t len, uint32_t target, GifParsed* out) {
    if (int rc = parse_gif_header(d, len, out)) return rc;
    GifParsed& P = *out;
    size_t pos = 13;
    if (P.has_global) {
        if (pos + 3u * P.global_n > len) { P.status = IFHIP_GIF_DEC_CONTAINER; return IFHIP_OK; }
        read_table(d + pos, P.global_n, &P.palettes);
        pos += 3u * P.global_n;
        if (P.bg_index < P.global_n) P.bg = P.palettes[P.bg_index];
    }
    GifFrameInfo pending;                                            // what a graphic control extension said about the next image
    while (P.frames.size() <= target) {
        if (pos >= len || d[pos] == 0x3Bu) break;
        const uint8_t kind = d[pos++];
        if (kind == 0x21u) {
            if (pos >= len) break;
            const uint8_t label = d[pos++];
            if (label == 0xF9u && pos + 5u <= len && d[pos] == 4u) {
                const uint32_t flags = d[pos + 1u], dispose = (flags >> 2) & 7u;
                pending.dispose = dispose <= 3u ? dispose : 1u;
                pending.transparent = (flags & 1u) ? d[pos + 4u] : 0xFFFFFFFFu;
                pending.user_input = (flags >> 1) & 1u;
                pending.delay = le16(d + pos + 2u);
            }
            // the application extension NETSCAPE2.0 with the sub-block 03 01 <loop count>: what the GIF coder hands on
            if (label == 0xFFu && pos + 16u <= len && d[pos] == 11u && std::memcmp(d + pos + 1u, "NETSCAPE2.0", 11) == 0 && d[pos + 12u] == 3u && d[pos + 13u] == 1u)
                P.repeat = static_cast<int32_t>(le16(d + pos + 14u));
            bool ended = false;
            for (;;) {                                               // the extension's sub-blocks
                if (pos >= len) { ended = true; break; }
                const size_t n = d[pos++];
                if (!n) break;
                pos += n;
            }
            if (ended) break;
        } else if (kind == 0x2Cu) {
            if (pos + 9u > len) break;
            GifFrameInfo f = pending;
            pending = GifFrameInfo();
            f.left = le16(d + pos); f.top = le16(d + pos + 2u); f.w = le16(d + pos + 4u); f.h = le16(d + pos + 6u);
            const uint32_t flags = d[pos + 8u];
            pos += 9u;
            f.interlace = (flags >> 6) & 1u;
            f.pal_off = 0; f.pal_n = P.global_n;
            if (flags & 0x80u) {
                const uint32_t n = 2u << (flags & 7u);
                if (pos + 3u * n > len) break;
                f.pal_off = static_cast<uint32_t>(P.palettes.size()); f.pal_n = n;
                read_table(d + pos, n, &P.palettes);
                pos += 3u * n;
            }
            if (pos >= len) break;
            f.min_code = d[pos++];
            f.stream_off = P.streams.size();
            uint64_t gathered = 0;
            while (pos < len && d[pos]) {
                const size_t n = std::min<size_t>(d[pos], len - pos - 1u);
                P.streams.insert(P.streams.end(), d + pos + 1u, d + pos + 1u + n);
                gathered += n;
                pos += 1u + static_cast<size_t>(d[pos]);
            }
            if (pos < len) ++pos;                                    // the terminator
            else pos = len;
            P.streams.resize(((P.streams.size() + 15u) & ~static_cast<size_t>(15)) + 16u, 0u);
            const bool has_table = (flags & 0x80u) || P.has_global;
            if (gathered > 0x7FFF0000ull) { P.status = IFHIP_GIF_DEC_CONTAINER; return IFHIP_OK; }
            f.stream_len = static_cast<uint32_t>(gathered);
            P.frames.push_back(f);
            if (f.min_code < 1u || f.min_code > 8u) { P.status = IFHIP_GIF_DEC_MIN_CODE_SIZE; return IFHIP_OK; }
            if (static_cast<uint64_t>(f.w) * f.h > 16ull * 1024u * 1024u) { P.status = IFHIP_GIF_DEC_FRAME_TOO_LARGE; return IFHIP_OK; }
            if (!has_table) { P.status = IFHIP_GIF_DEC_NO_PALETTE; return IFHIP_OK; }
        } else {
            P.status = IFHIP_GIF_DEC_CONTAINER;
            return IFHIP_OK;
        }
    }
    if (P.frames.size() <= target) P.status = IFHIP_GIF_DEC_NO_SUCH_FRAME;
    return IFHIP_OK;
}

int parse_gif_all(const uint8_t* d, size_t len, GifParsed* out) {
    if (int rc = parse_gif(d, len, 0xFFFFFFFFu, out)) return rc;
    if (out->status == IFHIP_GIF_DEC_NO_SUCH_FRAME && !out->frames.empty()) out->status = 0;     // (the walk's end, not a frame someone asked for)
    return IFHIP_OK;
}

const char* gif_status_text(uint32_t s) {
    switch (s) {
    case IFHIP_GIF_DEC_TOO_LITTLE: return "the image data holds fewer indices than the frame has pixels";
    case IFHIP_GIF_DEC_BAD_CODE: return "a code that names no table entry";
    case IFHIP_GIF_DEC_MIN_CODE_SIZE: return "a minimum code size outside 1..8";
    case IFHIP_GIF_DEC_NO_PALETTE: return "the frame must have _some_ palette";
    case IFHIP_GIF_DEC_FRAME_TOO_LARGE: return "GIF frame buffer_size exceeds 16MP limit";
    case IFHIP_GIF_DEC_NO_SUCH_FRAME: return "the file has no such frame";
    default: return "the container did not parse";
    }
}

}  // namespace ifhip

using namespace ifhip;

extern "C" int ifhip_gif_info(const uint8_t* gif, size_t len, ifhip_gif_file_info* info) {
    if (!info) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: null out-pointer");
    std::memset(info, 0, sizeof *info);
    if (!gif) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: null file pointer");
    GifParsed P;
    if (int rc = parse_gif_header(gif, len, &P)) return rc;
    info->width = P.w; info->height = P.h; info->has_global_palette = P.has_global ? 1u : 0u; info->background_index = P.bg_index;
    return IFHIP_OK;
}

extern "C" int ifhip_gif_frame_count(const uint8_t* gif, size_t len, uint32_t* n_frames, uint32_t* delays, uint32_t* flags, uint32_t capacity) {
    if (!n_frames) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: null out-pointer");
    *n_frames = 0;
    if (!gif) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: null file pointer");
    GifParsed P;
    if (int rc = parse_gif_all(gif, len, &P)) return rc;
    *n_frames = static_cast<uint32_t>(P.frames.size());
    for (uint32_t k = 0; k < *n_frames && k < capacity; ++k) {
        if (delays) delays[k] = P.frames[k].delay;
        if (flags) flags[k] = P.frames[k].user_input;
    }
    if (P.status && P.status != IFHIP_GIF_DEC_NO_SUCH_FRAME)      // (a file without a frame counts 0)
        return fail(IFHIP_INVALID_ARGUMENT, "ImageMalformed: GIF decoding error: %s", gif_status_text(P.status));
    return IFHIP_OK;
}
