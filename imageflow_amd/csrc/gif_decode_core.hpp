// gif_decode_core.hpp -- the one statement of GIF's LZW and of the frame replay for the device GIF decoder
// (csrc/gif_decode.hip), written so that it compiles for the gfx950 kernels AND for a plain host compiler: the CPU emulation
// of the tests (tests/gif_decode_emulate.cpp) and the sanitizer program (tools/sanitize/gif_fuzz.cpp) run the same scan, the
// same lengths and resolve steps and the same compositing, over a block laid out by the same gif_layout_batch.
//
// Two facts about the format carry the design:
//   1. Code positions are closed-form between clear codes.  The k-th code after a clear (k = 0 is the first) is read when
//      the table holds size(k) = min(clear + 2 + max(k - 1, 0), 4096) entries, and is as wide as the smallest w >= m + 1
//      with size(k) < 2^w, 12 at the most (m: the minimum code size, clear = 1 << m; the first code is m + 1 bits wide,
//      which the rule gives for every m but 1).  So codes of width <= w are the first cum(w) = 2^w - clear - 1 of a segment,
//      and bit_offset(k) = 12 k - sum over w in m+1 .. 11 of min(k, cum(w)).  64 lanes read 256 codes a step and find the
//      next clear or end code with a ballot; only the segments' starts are sequential.
//   2. Within a segment LZW output is LZ77 copies.  A literal (< clear) writes one byte.  A table code c names the entry
//      made when code j + 1 was read, j = c - clear - 2, 0 <= j < k: the output of code j followed by the first output byte
//      of code j + 1.  So outlen[k] = outlen[j] + 1 (pointer jumping over j(k) < k), off = the exclusive sum of outlen, and
//      byte i of code k is found by walking k -> j(k) from the string's end.  A clear resets the table: segments share
//      nothing.  Once the table is full (a deferred clear) codes add no entries, so every later code names one of the
//      segment's first 4096 codes: the tail is read in chunks against the first chunk's arrays.
//
// The wide parts go through executors:
//   wave   W.ballot(f)      the mask of lanes 0..63 with f(lane) true              (CPU: a loop)
//          W.one(f)         f() on one lane
//   block  X.threads(f)     f(tid) for the 256 threads, a barrier in front and behind (CPU: a loop)
//          X.scan(a, &sum)  a[0..255] in LDS -> its exclusive prefix sums, the total in sum
#pragma once
#include <cstdint>
#include <cstring>

#include <vector>

#include "gif_read.hpp"
#include "prefix_code_core.hpp"      // IFHIP_HD

namespace ifhip {

enum : uint32_t {
    kGifDecOk = 0,
    kGifDecTooLittle = 1,        // fewer indices than width x height
    kGifDecBadCode = 2,          // a table code with j >= k
    kGifDecContainer = 3,
    kGifDecMinCodeSize = 4,
    kGifDecNoPalette = 5,
    kGifDecFrameTooLarge = 6,
    kGifDecNoSuchFrame = 7,
};

constexpr uint32_t kGifThreads = 256;            // of the lengths / resolve / place workgroups
constexpr uint32_t kGifChunk = 4096;             // codes of a segment's first chunk: every table entry is made by one of them
constexpr uint32_t kGifTail = 1024;              // codes of a later chunk (a deferred clear's tail)
constexpr uint32_t kGifScanUnroll = 4;           // codes a lane of the scan reads per step
constexpr uint32_t kGifSizeCap = 1u << 30;       // a segment's recorded size saturates here (a frame holds 2^24 indices at most)

struct GifSegment {
    uint64_t start_bit;          // of the segment's first code
    uint32_t n_codes;            // up to, not counting, the clear / end code or the end of the data
    uint32_t size;               // indices it writes (the lengths step), saturated
};
struct GifFrameDesc {            // offsets: bytes into the batch's block, multiples of 16
    uint64_t stream_off, seg_off, place_off, index_off;
    uint32_t stream_len, min_code, max_segments, n_pix;
    uint32_t left, top, w, h;
    uint32_t interlace, dispose, transparent, file;
    uint32_t pal_off, pal_n;     // dwords from the file's palettes
    uint32_t pad[2];
};
struct GifFileDesc {
    uint8_t* frame;
    uint64_t pal_off;
    uint32_t w, h, stride, bg;
    uint32_t first_frame, n_frames;
    uint32_t preset_status, pad;
};
struct GifFrameState { uint32_t n_segments, status; };

struct GifLds {
    uint16_t code[kGifChunk];
    uint32_t a[kGifChunk], b[kGifChunk];         // hops << 16 | pointer, ping-pong; afterwards one of them holds `off`
    uint16_t tcode[kGifTail];
    uint32_t toff[kGifTail];
    uint32_t part[kGifThreads];
    uint32_t scan_scratch[kGifThreads / 64u];
    uint32_t changed[14];                        // [0]: a bad code; [1 + r]: round r of the pointer jumping moved something
};

// ---- fact 1: where a code lies ---------------------------------------------------------------------------------------------------
IFHIP_HD uint32_t gif_width_at(uint32_t m, uint64_t k) {
    const uint32_t clear = 1u << m;
    uint32_t w = m + 1u;
    while (w < 12u && k >= (1u << w) - clear - 1u) ++w;
    return w;
}
IFHIP_HD uint64_t gif_bit_offset(uint32_t m, uint64_t k) {
    const uint32_t clear = 1u << m;
    uint64_t off = 12u * k;
    for (uint32_t w = m + 1u; w < 12u; ++w) {
        const uint64_t cum = (1u << w) - clear - 1u;
        off -= k < cum ? k : cum;
    }
    return off;
}
// src holds the stream, zeros behind it up to a multiple of 16 and 16 bytes more; bit + width <= 8 * len
IFHIP_HD uint32_t gif_read_code(const uint8_t* src, uint64_t bit, uint32_t width) {
    const uint8_t* p = src + (bit >> 3);
    const uint32_t v = static_cast<uint32_t>(p[0]) | static_cast<uint32_t>(p[1]) << 8 | static_cast<uint32_t>(p[2]) << 16;
    return (v >> (bit & 7u)) & ((1u << width) - 1u);
}
// records a frame's scan can emit: every record but the last is a code and a clear code, m + 1 bits each at the least
IFHIP_HD uint32_t gif_max_segments(uint32_t stream_len, uint32_t m) { return static_cast<uint32_t>(static_cast<uint64_t>(stream_len) * 8u / (2u * (m + 1u))) + 1u; }

// ---- the scan: one wave per frame ------------------------------------------------------------------------------------------------
// A stream whose first code is no clear is read as if one stood in front; empty segments (a clear behind a clear) emit nothing.
template <typename W>
IFHIP_HD uint32_t gif_scan_frame(W& x, const uint8_t* src, uint32_t len, uint32_t m, GifSegment* recs, uint32_t max_recs) {
    const uint64_t nbits = static_cast<uint64_t>(len) * 8u;
    const uint32_t clear = 1u << m;
    uint64_t p0 = 0;
    uint32_t n = 0;
    for (;;) {
        uint64_t k0 = 0, kt = 0;
        uint32_t how = 0;                                        // 1: a clear code at kt; 2: the end code or the end of the data
        while (!how) {
            const uint64_t mask = x.ballot([&](uint32_t lane) {
                bool hit = false;
                for (uint32_t u = 0; u < kGifScanUnroll; ++u) {
                    const uint64_t k = k0 + lane * kGifScanUnroll + u, bit = p0 + gif_bit_offset(m, k);
                    const uint32_t w = gif_width_at(m, k);
                    if (bit + w > nbits) { hit = true; break; }
                    const uint32_t c = gif_read_code(src, bit, w);
                    hit = hit || c == clear || c == clear + 1u;
                }
                return hit;
            });
            if (!mask) { k0 += 64u * kGifScanUnroll; continue; }
            const uint32_t first = static_cast<uint32_t>(__builtin_ctzll(mask));
            for (uint32_t u = 0; u < kGifScanUnroll && !how; ++u) {          // uniform: the first lane's codes again
                kt = k0 + first * kGifScanUnroll + u;
                const uint64_t bit = p0 + gif_bit_offset(m, kt);
                const uint32_t w = gif_width_at(m, kt);
                if (bit + w > nbits) how = 2u;
                else {
                    const uint32_t c = gif_read_code(src, bit, w);
                    if (c == clear) how = 1u;
                    else if (c == clear + 1u) how = 2u;
                }
            }
        }
        if (kt) {
            if (n >= max_recs) return n;                         // (the arithmetic of gif_max_segments rules it out)
            const GifSegment s = {p0, static_cast<uint32_t>(kt), 0u};
            x.one([&] { recs[n] = s; });
            ++n;
        }
        if (how == 2u) return n;
        p0 += gif_bit_offset(m, kt) + gif_width_at(m, kt);
    }
}

// ---- fact 2: a segment's lengths, and its indices ----------------------------------------------------------------------------------
// The string of code c, n bytes of it, written from its end at out[base ...]: stores below `cap` only.  F: the finished
// pointer jumping of the first chunk (the low half of F[k]: the literal at the bottom of code k's chain).
IFHIP_HD void gif_write_string(const GifLds& S, const uint32_t* F, uint32_t clear, uint32_t c, uint32_t n, uint64_t base, uint8_t* out, uint64_t cap) {
    for (uint32_t i = n; i-- > 0u;) {
        uint32_t byte = c;
        if (c >= clear + 2u) {
            const uint32_t j = c - clear - 2u;
            byte = S.code[F[j + 1u] & 0xFFFFu];
            c = S.code[j];
        }
        if (base + i < cap) out[base + i] = static_cast<uint8_t>(byte);
    }
}

// One segment by one workgroup.  out == nullptr: the lengths step alone.  Returns the indices the segment writes, saturated
// at kGifSizeCap and not counted beyond `cap` (what the frame still needs: more changes nothing); *status: kGifDecBadCode.
template <typename X>
IFHIP_HD uint32_t gif_segment(X& x, GifLds& S, const uint8_t* src, uint32_t m, const GifSegment seg, uint8_t* out, uint64_t cap, uint32_t* status) {
    const uint32_t clear = 1u << m, n0 = seg.n_codes < kGifChunk ? seg.n_codes : kGifChunk;
    x.threads([&](uint32_t tid) { if (tid < 14u) S.changed[tid] = 0u; });
    x.threads([&](uint32_t tid) {
        for (uint32_t k = tid; k < n0; k += kGifThreads) {
            const uint32_t c = gif_read_code(src, seg.start_bit + gif_bit_offset(m, k), gif_width_at(m, k));
            S.code[k] = static_cast<uint16_t>(c);
            if (c >= clear + 2u) {
                const uint32_t j = c - clear - 2u;
                if (j >= k) S.changed[0] = 1u;
                S.a[k] = 1u << 16 | (j & 0xFFFu);
            } else S.a[k] = k;
        }
    });
    if (S.changed[0]) { *status = kGifDecBadCode; return 0u; }
    uint32_t* F = S.a;
    uint32_t* other = S.b;
    for (uint32_t round = 0; round < 12u; ++round) {             // hops += hops[pointer]; pointer = pointer[pointer]
        x.threads([&](uint32_t tid) {
            for (uint32_t k = tid; k < n0; k += kGifThreads) {
                const uint32_t v = F[k], pv = F[v & 0xFFFFu];
                other[k] = ((v >> 16) + (pv >> 16)) << 16 | (pv & 0xFFFFu);
                if (pv >> 16) S.changed[1u + round] = 1u;
            }
        });
        uint32_t* t = F; F = other; other = t;
        if (!S.changed[1u + round]) break;
    }
    uint32_t* off = other;
    constexpr uint32_t per = kGifChunk / kGifThreads;
    x.threads([&](uint32_t tid) {
        uint32_t sum = 0;
        for (uint32_t k = tid * per; k < (tid + 1u) * per && k < n0; ++k) sum += (F[k] >> 16) + 1u;
        S.part[tid] = sum;
    });
    uint32_t total = 0;
    x.scan(S.part, &total);
    uint64_t acc = total;
    if (out) {
        x.threads([&](uint32_t tid) {
            uint32_t run = S.part[tid];
            for (uint32_t k = tid * per; k < (tid + 1u) * per && k < n0; ++k) { off[k] = run; run += (F[k] >> 16) + 1u; }
        });
        x.threads([&](uint32_t tid) {
            for (uint32_t k = tid; k < n0; k += kGifThreads) gif_write_string(S, F, clear, S.code[k], (F[k] >> 16) + 1u, off[k], out, cap);
        });
    }
    constexpr uint32_t tper = kGifTail / kGifThreads;
    for (uint32_t done = n0; done < seg.n_codes && acc < cap; done += kGifTail) {     // the tail behind a full table
        const uint32_t nt = seg.n_codes - done < kGifTail ? seg.n_codes - done : kGifTail;
        x.threads([&](uint32_t tid) {
            uint32_t sum = 0;
            for (uint32_t t = tid * tper; t < (tid + 1u) * tper && t < nt; ++t) {
                const uint64_t k = static_cast<uint64_t>(done) + t;
                const uint32_t c = gif_read_code(src, seg.start_bit + gif_bit_offset(m, k), gif_width_at(m, k));
                S.tcode[t] = static_cast<uint16_t>(c);
                S.toff[t] = sum;
                sum += c >= clear + 2u ? (F[c - clear - 2u] >> 16) + 2u : 1u;
            }
            S.part[tid] = sum;
        });
        x.scan(S.part, &total);
        if (out)
            x.threads([&](uint32_t tid) {
                for (uint32_t t = tid * tper; t < (tid + 1u) * tper && t < nt; ++t) {
                    const uint32_t c = S.tcode[t];
                    gif_write_string(S, F, clear, c, c >= clear + 2u ? (F[c - clear - 2u] >> 16) + 2u : 1u, acc + S.part[tid] + S.toff[t], out, cap);
                }
            });
        acc += total;
    }
    return acc < kGifSizeCap ? static_cast<uint32_t>(acc) : kGifSizeCap;
}

// Every segment's place among the frame's indices, by one workgroup; returns what the frame got, not counted beyond n_pix.
template <typename X, typename Lds>
IFHIP_HD uint32_t gif_place_segments(X& x, Lds& S, const GifSegment* recs, uint32_t n, uint32_t* place, uint32_t n_pix) {
    uint64_t base = 0;
    for (uint32_t r0 = 0; r0 < n; r0 += kGifThreads) {
        x.threads([&](uint32_t tid) { S.part[tid] = r0 + tid < n ? recs[r0 + tid].size : 0u; });
        uint32_t total = 0;
        x.scan(S.part, &total);
        x.threads([&](uint32_t tid) {
            if (r0 + tid < n) { const uint64_t at = base + S.part[tid]; place[r0 + tid] = at < n_pix ? static_cast<uint32_t>(at) : n_pix; }
        });
        base += total;
    }
    return base < n_pix ? static_cast<uint32_t>(base) : n_pix;
}

// ---- the replay: one lane per screen pixel ---------------------------------------------------------------------------------------------
// the row of an interlaced frame's data that holds image row y
IFHIP_HD uint32_t gif_interlace_source_row(uint32_t y, uint32_t h) {
    const uint32_t n1 = (h + 7u) / 8u, n2 = (h + 3u) / 8u, n3 = (h + 1u) / 4u;
    if ((y & 7u) == 0u) return y >> 3;
    if ((y & 7u) == 4u) return n1 + (y >> 3);
    if ((y & 1u) == 0u) return n1 + n2 + (y >> 2);
    return n1 + n2 + n3 + (y >> 1);
}
// Screen::blit for frames 0 .. n - 1 in the reference's order, as far as screen pixel (x, y) sees it: dispose what the
// previous frame left (gif/disposal.rs:30-53), note what lies under this one where it asks for Previous (:55-76), blit
// (gif/screen.rs:59-91).  each(k, value): the pixel of the screen behind frame k's blit -- what a reader that asked for
// frame k is handed.  The pixel's state (its value, what disposal 3 puts back) lives in registers from frame to frame.
template <typename E>
IFHIP_HD uint32_t gif_compose_replay(const GifFileDesc& f, const GifFrameDesc* frames, const uint8_t* block, uint32_t x, uint32_t y, E each) {
    const uint32_t* pal = reinterpret_cast<const uint32_t*>(block + f.pal_off);
    uint32_t cur = f.bg, saved = f.bg, method = 1u, pl = 0, pt = 0, pw = 0, ph = 0;
    for (uint32_t i = 0; i < f.n_frames; ++i) {
        const GifFrameDesc& fr = frames[f.first_frame + i];
        const uint32_t l = fr.left < f.w ? fr.left : f.w, t = fr.top < f.h ? fr.top : f.h;
        const uint32_t sw = fr.w < f.w - l ? fr.w : f.w - l, sh = fr.h < f.h - t ? fr.h : f.h - t;
        if (pw && ph && x - pl < pw && y - pt < ph && x >= pl && y >= pt) {
            if (method == 2u) cur = f.bg;
            else if (method == 3u) cur = saved;
        }
        const bool inside = sw && sh && x >= l && y >= t && x - l < sw && y - t < sh;
        if (fr.dispose == 3u && inside) saved = cur;
        method = fr.dispose; pl = l; pt = t; pw = sw; ph = sh;
        if (inside) {
            const uint32_t fy = y - t, row = fr.interlace ? gif_interlace_source_row(fy, fr.h) : fy;
            const uint32_t idx = block[fr.index_off + static_cast<uint64_t>(row) * fr.w + (x - l)];
            if (idx != fr.transparent) cur = idx < fr.pal_n ? pal[fr.pal_off + idx] : 0u;
        }
        each(i, cur);
    }
    return cur;
}
// the screen behind the file's last frame alone: what one selected frame asks for
IFHIP_HD uint32_t gif_compose_pixel(const GifFileDesc& f, const GifFrameDesc* frames, const uint8_t* block, uint32_t x, uint32_t y) {
    return gif_compose_replay(f, frames, block, x, y, [](uint32_t, uint32_t) {});
}
// every screen of the file in one replay: screen k lies `screen_pitch` bytes behind screen k - 1, rows at the file's stride
IFHIP_HD void gif_compose_all_pixel(const GifFileDesc& f, const GifFrameDesc* frames, const uint8_t* block, uint32_t x, uint32_t y, size_t screen_pitch) {
    uint8_t* at = f.frame + static_cast<size_t>(y) * f.stride + 4u * static_cast<size_t>(x);
    (void)gif_compose_replay(f, frames, block, x, y, [&](uint32_t k, uint32_t value) { *reinterpret_cast<uint32_t*>(at + k * screen_pitch) = value; });
}
// the first status among a file's frames
IFHIP_HD uint32_t gif_file_status(const GifFileDesc& f, const GifFrameState* state) {
    if (f.preset_status) return f.preset_status;
    for (uint32_t i = 0; i < f.n_frames; ++i)
        if (state[f.first_frame + i].status) return state[f.first_frame + i].status;
    return kGifDecOk;
}

// ---- the batch's block: what is uploaded (descriptors, states, palettes, streams), and the scratch behind it -------------------------------------
struct GifLayout {
    std::vector<uint8_t> blob;           // the uploaded part
    size_t total = 0;                    // with the scratch: segment records, places and index buffers, sized by arithmetic
    size_t files_off = 0, frames_off = 0, state_off = 0;
    uint32_t n_frames = 0, max_segments = 1, max_pixels = 1;
};
// files[i] == nullptr or a set status: nothing runs for the file.  frames / strides: where each file's screen goes.
inline void gif_layout_batch(const GifParsed* const* files, uint32_t n_files, uint8_t* const* frames, const uint32_t* strides, GifLayout* L) {
    auto pad16 = [](size_t v) { return (v + 15u) & ~static_cast<size_t>(15); };
    std::vector<GifFileDesc> fd(n_files);
    std::vector<GifFrameDesc> fr;
    std::memset(fd.data(), 0, sizeof(GifFileDesc) * n_files);
    for (uint32_t i = 0; i < n_files; ++i) {
        GifFileDesc& f = fd[i];
        if (!files[i]) { f.preset_status = kGifDecContainer; continue; }
        const GifParsed& P = *files[i];
        f.frame = frames[i]; f.w = P.w; f.h = P.h; f.stride = strides[i]; f.bg = P.bg;
        f.preset_status = P.status;
        if (P.status) continue;
        f.first_frame = static_cast<uint32_t>(fr.size()); f.n_frames = static_cast<uint32_t>(P.frames.size());
        for (const GifFrameInfo& g : P.frames) {
            GifFrameDesc d;
            std::memset(&d, 0, sizeof d);
            d.stream_len = g.stream_len; d.min_code = g.min_code; d.max_segments = gif_max_segments(g.stream_len, g.min_code); d.n_pix = g.w * g.h;
            d.left = g.left; d.top = g.top; d.w = g.w; d.h = g.h; d.interlace = g.interlace; d.dispose = g.dispose; d.transparent = g.transparent;
            d.file = i; d.pal_off = g.pal_off; d.pal_n = g.pal_n;
            d.stream_off = g.stream_off;                          // (relative to the file's streams until they are placed below)
            fr.push_back(d);
        }
    }
    L->n_frames = static_cast<uint32_t>(fr.size());
    size_t at = 0;
    L->files_off = at; at = pad16(at + sizeof(GifFileDesc) * n_files);
    L->frames_off = at; at = pad16(at + sizeof(GifFrameDesc) * fr.size());
    L->state_off = at; at = pad16(at + sizeof(GifFrameState) * fr.size());
    for (uint32_t i = 0; i < n_files; ++i) {
        if (fd[i].preset_status) continue;
        const GifParsed& P = *files[i];
        fd[i].pal_off = at; at = pad16(at + P.palettes.size() * 4u);
        for (uint32_t k = 0; k < fd[i].n_frames; ++k) fr[fd[i].first_frame + k].stream_off += at;
        at = pad16(at + P.streams.size());
    }
    L->blob.assign(at, 0u);
    for (GifFrameDesc& d : fr) {
        d.seg_off = at; at = pad16(at + sizeof(GifSegment) * d.max_segments);
        d.place_off = at; at = pad16(at + 4u * static_cast<size_t>(d.max_segments));
        d.index_off = at; at = pad16(at + d.n_pix);
        if (d.max_segments > L->max_segments) L->max_segments = d.max_segments;
    }
    L->total = at;
    for (uint32_t i = 0; i < n_files; ++i)
        if (!fd[i].preset_status) {
            const GifParsed& P = *files[i];
            if (static_cast<uint64_t>(P.w) * P.h > L->max_pixels) L->max_pixels = P.w * P.h;
            if (!P.palettes.empty()) std::memcpy(L->blob.data() + fd[i].pal_off, P.palettes.data(), P.palettes.size() * 4u);
            if (!P.streams.empty()) std::memcpy(L->blob.data() + fr[fd[i].first_frame].stream_off - P.frames[0].stream_off, P.streams.data(), P.streams.size());
        }
    if (n_files) std::memcpy(L->blob.data() + L->files_off, fd.data(), sizeof(GifFileDesc) * n_files);
    if (!fr.empty()) std::memcpy(L->blob.data() + L->frames_off, fr.data(), sizeof(GifFrameDesc) * fr.size());
}

#ifndef __HIPCC__
// ---- the executors and the five launches on the CPU ---------------------------------------------------------------------------------------
struct GifCpuWave {
    template <typename F> uint64_t ballot(F f) { uint64_t m = 0; for (uint32_t l = 0; l < 64u; ++l) if (f(l)) m |= 1ull << l; return m; }
    template <typename F> void one(F f) { f(); }
};
struct GifCpuBlock {
    template <typename F> void threads(F f) { for (uint32_t t = 0; t < kGifThreads; ++t) f(t); }
    void scan(uint32_t* a, uint32_t* total) { uint32_t run = 0; for (uint32_t t = 0; t < kGifThreads; ++t) { const uint32_t v = a[t]; a[t] = run; run += v; } *total = run; }
};
// The batch as the kernels run it, on a block of exactly L.total bytes; status[i]: the files' status words.  grid_x: the
// workgroups that share a frame's segments, as the kernels' grid does.
// all_screens_pitch != 0: every screen of every file, as gif_compose_all_kernel writes them.
inline void gif_decode_batch_cpu(const GifLayout& L, uint32_t n_files, uint8_t* block, uint32_t* status, uint32_t grid_x = 3u, size_t all_screens_pitch = 0) {
    std::memcpy(block, L.blob.data(), L.blob.size());
    const GifFileDesc* files = reinterpret_cast<const GifFileDesc*>(block + L.files_off);
    const GifFrameDesc* frames = reinterpret_cast<const GifFrameDesc*>(block + L.frames_off);
    GifFrameState* state = reinterpret_cast<GifFrameState*>(block + L.state_off);
    GifCpuWave wave;
    GifCpuBlock blk;
    std::vector<GifLds> lds(1);
    GifLds& S = lds[0];
    for (uint32_t f = 0; f < L.n_frames; ++f)
        state[f].n_segments = gif_scan_frame(wave, block + frames[f].stream_off, frames[f].stream_len, frames[f].min_code, reinterpret_cast<GifSegment*>(block + frames[f].seg_off), frames[f].max_segments);
    for (int pass = 0; pass < 2; ++pass) {
        for (uint32_t f = 0; f < L.n_frames; ++f) {
            GifSegment* recs = reinterpret_cast<GifSegment*>(block + frames[f].seg_off);
            uint32_t* place = reinterpret_cast<uint32_t*>(block + frames[f].place_off);
            if (pass == 1 && state[f].status) continue;
            for (uint32_t bx = 0; bx < grid_x; ++bx)
                for (uint32_t r = bx; r < state[f].n_segments; r += grid_x) {
                    uint32_t st = 0;
                    if (pass == 0) { recs[r].size = gif_segment(blk, S, block + frames[f].stream_off, frames[f].min_code, recs[r], nullptr, frames[f].n_pix, &st); if (st) state[f].status = st; }
                    else (void)gif_segment(blk, S, block + frames[f].stream_off, frames[f].min_code, recs[r], block + frames[f].index_off + place[r], frames[f].n_pix - place[r], &st);
                }
            if (pass == 0 && !state[f].status && gif_place_segments(blk, S, recs, state[f].n_segments, place, frames[f].n_pix) < frames[f].n_pix) state[f].status = kGifDecTooLittle;
        }
    }
    for (uint32_t i = 0; i < n_files; ++i) {
        status[i] = gif_file_status(files[i], state);
        if (status[i]) continue;
        for (uint32_t y = 0; y < files[i].h; ++y)
            for (uint32_t x = 0; x < files[i].w; ++x) {
                if (all_screens_pitch) { gif_compose_all_pixel(files[i], frames, block, x, y, all_screens_pitch); continue; }
                const uint32_t v = gif_compose_pixel(files[i], frames, block, x, y);
                std::memcpy(files[i].frame + static_cast<size_t>(y) * files[i].stride + 4u * x, &v, 4);
            }
    }
}
#endif

}  // namespace ifhip
