// gif_animation_emulate.cpp -- the animation paths of the two GIF cores on the CPU, from the headers the gfx950 kernels are
// built from: every composed screen of a file in one replay (csrc/gif_decode_core.hpp: gif_compose_all_pixel behind the same
// scan, lengths, place and resolve steps), and the layout of N coded frames into one file over the FILE's dwords, chunk by
// chunk with the carry word between chunks (csrc/gif_encode_core.hpp: gifenc_animation_word) -- as gif_anim_offsets_kernel and
// gif_anim_layout_kernel of csrc/gif_encode.hip run it.  Built by tests/gif_animation_emu.py with g++.
#include <cstdarg>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../imageflow_amd/csrc/gif_read.cpp"
#include "../imageflow_amd/csrc/gif_encode_core.hpp"

namespace ifhip {
int fail(int status, const char*, ...) { return status; }
}  // namespace ifhip

using namespace ifhip;

extern "C" {

// One file, every screen -> screen k at out + k * pitch, BGRA rows of `stride` bytes; `cap`: the bytes of out.  Returns the
// status word (kGifDecContainer where the header does not parse or the screens do not fit); *frames: 0 unless the status is 0.
uint32_t gif_anim_emu_decode_frames(const uint8_t* file, size_t len, uint8_t* out, uint64_t cap, uint64_t pitch, uint32_t stride, uint32_t* w, uint32_t* h,
                                    uint32_t* frames, uint32_t grid_x) {
    GifParsed P;
    *w = *h = *frames = 0;
    if (parse_gif_all(file, len, &P) != 0 || !P.w || !P.h) return kGifDecContainer;
    *w = P.w; *h = P.h;
    if (P.status) return P.status;
    if (stride < 4u * P.w || pitch < static_cast<uint64_t>(P.h) * stride || pitch * P.frames.size() > cap) return kGifDecContainer;
    const GifParsed* files[1] = {&P};
    uint8_t* dst[1] = {out};
    const uint32_t strides[1] = {stride};
    GifLayout L;
    gif_layout_batch(files, 1, dst, strides, &L);
    uint8_t* block = static_cast<uint8_t*>(std::malloc(L.total ? L.total : 1));
    std::memset(block + L.blob.size(), 0xA5, L.total - L.blob.size());      // the scratch is not cleared on the device either
    uint32_t status = 0;
    gif_decode_batch_cpu(L, 1, block, &status, grid_x ? grid_x : 1u, static_cast<size_t>(pitch));
    std::free(block);
    if (!status) *frames = static_cast<uint32_t>(P.frames.size());
    return status;
}

// N coded frames into one file, `chunk` frames at a time.  Frame i: counts[i] palette keys at keys + 256 * i (file order, the
// transparent entry first), n_trans[i], its LZW data of data_bytes[i] bytes at streams + i * stream_pitch.  Returns the file's
// length, 0 where it exceeds `cap` (*status = kGifEncFileOverflow).
uint32_t gif_anim_emu_layout(uint32_t w, uint32_t h, uint32_t n_frames, uint32_t chunk, int alpha_meaningful, int repeat, const uint32_t* delays, const uint8_t* user_input,
                             const uint32_t* counts, const uint32_t* keys, const uint32_t* n_trans, const uint8_t* streams, uint32_t stream_pitch,
                             const uint32_t* data_bytes, uint8_t* file, uint32_t cap, uint32_t* status) {
    const uint32_t dispose = gifenc_animation_dispose(n_frames, alpha_meaningful != 0);
    std::vector<uint32_t> out32((static_cast<size_t>(cap) + 3u) / 4u + 1u, 0xA5A5A5A5u);
    uint8_t* out = reinterpret_cast<uint8_t*>(out32.data());
    uint32_t run[4] = {0xA5A5A5A5u, 0xA5A5A5A5u, 0xA5A5A5A5u, 0xA5A5A5A5u}, length = 0;
    std::vector<uint32_t> off(chunk + 1u), head_bytes(chunk);
    std::vector<uint8_t> heads(kGifEncScreenPitch + static_cast<size_t>(chunk) * kGifEncFrameHeadPitch, 0xA5);
    *status = 0;
    for (uint32_t base = 0, ci = 0; base < n_frames; base += chunk, ++ci) {
        const uint32_t n = n_frames - base < chunk ? n_frames - base : chunk;
        const uint32_t first = base == 0u, last = base + n == n_frames;
        // offsets
        uint32_t at = first ? gifenc_screen_bytes(repeat) : run[0];
        for (uint32_t i = 0; i < n; ++i) {
            const uint32_t f = base + i;
            off[i] = at; head_bytes[i] = gifenc_frame_head_bytes(counts[f]);
            if (gifenc_write_frame_head(heads.data() + kGifEncScreenPitch + static_cast<size_t>(i) * kGifEncFrameHeadPitch, w, h, keys + 256u * f, counts[f], n_trans[f],
                                        delays[f], user_input[f], dispose) != head_bytes[i]) return 0xFFFFFFFFu;
            at += gifenc_body_bytes(counts[f], data_bytes[f]);
        }
        off[n] = at;
        const uint32_t seen = first ? 0u : run[1];
        run[0] = at;
        run[1] = (seen || static_cast<uint64_t>(at) + last > cap) ? 1u : 0u;
        if (first && gifenc_write_screen(heads.data(), w, h, repeat) != gifenc_screen_bytes(repeat)) return 0xFFFFFFFFu;
        // layout
        GifAnimChunk c;
        c.off = off.data(); c.heads = heads.data(); c.streams = streams + static_cast<size_t>(base) * stream_pitch; c.data_bytes = data_bytes + base;
        c.head_bytes = head_bytes.data(); c.n = n; c.stream_pitch = stream_pitch; c.first = first; c.last = last;
        c.lo = first ? 0u : off[0]; c.hi = off[n] + last;
        if (last) { length = run[1] ? 0u : c.hi; *status = run[1] ? kGifEncFileOverflow : 0u; }
        if (run[1]) continue;
        const uint32_t carry_in = first ? 0u : run[2u + ((ci + 1u) & 1u)];
        const uint32_t j0 = c.lo / 4u, j1 = c.hi / 4u;
        for (uint32_t j = j1; j-- > j0;) out32[j] = gifenc_animation_word(c, j, carry_in);          // (any order: a dword has one owner)
        const uint32_t tail = gifenc_animation_word(c, j1, carry_in);
        if (!last) run[2u + (ci & 1u)] = tail;
        else for (uint32_t p = 4u * j1; p < c.hi; ++p) out[p] = static_cast<uint8_t>(tail >> (8u * (p - 4u * j1)));
    }
    std::memcpy(file, out, length);
    return length;
}

uint64_t gif_anim_emu_max_bytes(uint32_t w, uint32_t h, uint32_t n_frames) { return gifenc_screen_bytes(0) + static_cast<uint64_t>(n_frames) * gifenc_max_file_bytes(static_cast<uint64_t>(w) * h) + 1u; }

}  // extern "C"
