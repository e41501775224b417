// webp_encode_indexed.hip -- gfx950 kernels of the device lossless-WebP coder's colour indexing (the stage flag
// IFHIP_WEBP_ENC_COLOR_INDEXING of webp_encode.hip): a frame of at most 256 distinct colours is also sized as a VP8L stream
// that opens with the colour-indexing transform, and the smaller of the two files is written.
// Launches per batch (all images in each), around the plain coder's own residual / parse / codes:
//   count     grid-wide: the image's distinct ARGB dwords into an exact hash set by atomicCAS; the 257th colour sets the
//             image's overflow word, on which every workgroup that has not started yet leaves at once -- a photograph costs
//             about one partial read of the frame
//   palette   a workgroup per image: the set's entries compacted and rank-sorted (ascending dwords: who inserted first does
//             not show), the bundling bits and the packed width into the image's record
//   bundle    a lane per packed pixel, the palette in LDS: a binary search of at most 8 steps for each of its 1, 2, 4 or 8
//             source pixels
//   parse, codes   the plain coder's bodies (webp_encode_device.hpp) on the packed image.  Its shape is known only here, so
//             the grids are sized from the stage's full geometry and the workgroups beyond the image's own segments leave
//   layout    a workgroup per image: both variants' heads and bit offsets, the two files' sizes compared (a tie goes to the
//             plain file), the overflow check and the head of the one that is written
//   emit      a workgroup per segment and per group header of either variant; those of the variant not written leave
// webp_finish_kernel (webp_encode.hip) frames either file.  An image of more than 256 colours leaves every kernel behind the
// palette at its first branch and is the flag-off file byte for byte.  The rules live in webp_encode_core.hpp, compiled
// into the CPU emulation of the tests as well (tests/webp_indexed_emulate.cpp).
#include <hip/hip_runtime.h>

#include "hip_entry.hpp"
#include "webp_encode_indexed.hpp"

namespace ifhip {

constexpr uint32_t kWebpCountPixels = 4096;             // pixels a workgroup of the count reads: 16 a lane
enum : uint32_t { kSetCount = 0, kSetOverflow = 1, kSetWhite = 2 };   // the words behind a set's slots

__device__ __forceinline__ uint32_t webp_set_hash(uint32_t c) {
    c ^= c >> 16; c *= 0x7FEB352Du; c ^= c >> 15; c *= 0x846CA68Bu; c ^= c >> 16;
    return c & (kWebpSetSlots - 1u);
}
__device__ __forceinline__ uint32_t webp_peek(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void webp_poke(uint32_t* p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// ---- count: grid-wide, a workgroup per 4096 pixels ---------------------------------------------------------------------------------
// A slot holds colour + 1 (0: empty); opaque white, the one colour that would read as empty, has a word of its own.
__global__ __launch_bounds__(256) void webp_ix_count_kernel(const WebpArgs a, const WebpIndexArgs ix) {
    const uint32_t img = blockIdx.y;
    uint32_t* set = ix.sets + static_cast<size_t>(img) * kWebpSetWords;
    uint32_t* state = set + kWebpSetSlots;
    const uint8_t* frame = a.images + static_cast<size_t>(img) * a.image_bytes;
    const uint32_t w = a.S.w, npix = a.S.w * a.S.h;
    uint32_t last = 0;
    bool have = false;
    for (uint32_t k = 0; k < kWebpCountPixels / 256u; ++k) {
        if (webp_peek(state + kSetOverflow)) return;           // more than 256 colours: the image is written plain
        const uint32_t i = blockIdx.x * kWebpCountPixels + k * 256u + threadIdx.x;
        if (i >= npix) return;
        const uint32_t y = i / w, x = i - y * w;
        const uint32_t c = webp_argb(frame, a.stride, x, y, a.alpha_or);
        if (have && c == last) continue;                       // (the lane has seen to this colour already)
        have = true; last = c;
        if (c == 0xFFFFFFFFu) { webp_poke(state + kSetWhite, 1u); continue; }
        const uint32_t key = c + 1u;
        uint32_t h = webp_set_hash(c);
        bool placed = false;
        for (uint32_t probe = 0; probe < kWebpSetSlots && !placed; ++probe) {
            if (probe >= 8u && webp_peek(state + kSetOverflow)) return;
            uint32_t held = webp_peek(set + h);
            if (held == 0u) {
                held = atomicCAS(set + h, 0u, key);
                if (held == 0u) {                              // a new colour: the 257th of them is one too many
                    if (atomicAdd(state + kSetCount, 1u) >= kWebpMaxPalette) webp_poke(state + kSetOverflow, 1u);
                    placed = true;
                }
            }
            if (held == key) placed = true;
            h = (h + 1u) & (kWebpSetSlots - 1u);
        }
        if (!placed) webp_poke(state + kSetOverflow, 1u);      // (a full set: only behind an overflow another lane is about to report)
    }
}

// ---- palette: a workgroup per image, a lane per slot -------------------------------------------------------------------------------
__global__ __launch_bounds__(kWebpSetSlots) void webp_ix_palette_kernel(const WebpArgs a, const WebpIndexArgs ix) {
    __shared__ uint32_t keys[kWebpMaxPalette], n;
    const uint32_t tid = threadIdx.x, img = blockIdx.x;
    const uint32_t* set = ix.sets + static_cast<size_t>(img) * kWebpSetWords;
    const uint32_t* state = set + kWebpSetSlots;
    WebpIndexRecord& rec = ix.rec[img];
    if (state[kSetOverflow]) {                                 // (the whole workgroup)
        if (tid == 0u) rec.n_colours = 0u;
        return;
    }
    if (tid == 0u) n = 0u;
    __syncthreads();
    const uint32_t held = set[tid];
    if (held) {
        const uint32_t at = atomicAdd(&n, 1u);
        if (at < kWebpMaxPalette) keys[at] = held - 1u;
    }
    __syncthreads();
    if (tid == 0u && state[kSetWhite]) {
        if (n < kWebpMaxPalette) keys[n] = 0xFFFFFFFFu;
        n = n + 1u;
    }
    __syncthreads();
    const uint32_t total = n;
    if (total > kWebpMaxPalette) {                             // (the whole workgroup) 256 colours and opaque white
        if (tid == 0u) rec.n_colours = 0u;
        return;
    }
    if (tid < total) {                                         // the colours are distinct: a colour's rank is its place
        const uint32_t c = keys[tid];
        uint32_t rank = 0;
        for (uint32_t j = 0; j < total; ++j) rank += keys[j] < c ? 1u : 0u;
        rec.palette[rank] = c;
    }
    if (tid == 0u) {
        const uint32_t bits = webp_index_width_bits(total);
        rec.n_colours = total; rec.width_bits = bits; rec.packed_w = webp_packed_width(a.S.w, bits); rec.unused = 0u;
    }
}

// ---- bundle: a lane per packed pixel -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void webp_ix_bundle_kernel(const WebpArgs a, const WebpIndexArgs ix) {
    __shared__ uint32_t pal[kWebpMaxPalette];
    const uint32_t tid = threadIdx.x, img = blockIdx.y;
    const WebpIndexRecord& rec = ix.rec[img];
    const uint32_t n = rec.n_colours, pw = rec.packed_w;
    if (n == 0u || blockIdx.x * 256u >= pw * a.S.h) return;    // (the whole workgroup)
    pal[tid] = tid < n ? rec.palette[tid] : 0u;
    __syncthreads();
    const uint32_t i = blockIdx.x * 256u + tid;
    if (i >= pw * a.S.h) return;
    const uint32_t y = i / pw, xp = i - y * pw;
    const uint8_t* frame = a.images + static_cast<size_t>(img) * a.image_bytes;
    a.resid[static_cast<size_t>(img) * a.px_pitch + i] = webp_bundle(frame, a.stride, a.S.w, xp, y, a.alpha_or, pal, n, rec.width_bits);
}

// ---- parse, codes: the plain coder's bodies on the packed image ---------------------------------------------------------------------
__global__ __launch_bounds__(1024) void webp_ix_parse_kernel(const WebpArgs a, const WebpIndexArgs ix) {
    const WebpIndexRecord& rec = ix.rec[blockIdx.y];
    if (rec.n_colours == 0u) return;
    const WebpShape S = webp_shape(rec.packed_w, a.S.h);
    if (blockIdx.x >= S.n_segs) return;
    webp_parse_segment(a, S, blockIdx.x, blockIdx.y);
}
__global__ __launch_bounds__(256) void webp_ix_codes_kernel(const WebpArgs a, const WebpIndexArgs ix) {
    const WebpIndexRecord& rec = ix.rec[blockIdx.y];
    if (rec.n_colours == 0u) return;
    webp_code_band(a, webp_shape(rec.packed_w, a.S.h), blockIdx.x, blockIdx.y);
}

// ---- layout: a workgroup per image; both variants, and the choice ---------------------------------------------------------------------
__global__ __launch_bounds__(1024) void webp_ix_layout_kernel(const WebpArgs plain, const WebpArgs packed, const WebpIndexArgs ix) {
    __shared__ WebpHead H_plain, H_packed;
    __shared__ WebpLayoutWork L;
    __shared__ uint32_t pal[kWebpMaxPalette], overflow;
    const uint32_t tid = threadIdx.x, img = blockIdx.x;
    const WebpIndexRecord& rec = ix.rec[img];
    const uint32_t n = rec.n_colours;
    if (tid < kWebpMaxPalette) pal[tid] = tid < n ? rec.palette[tid] : 0u;
    __syncthreads();
    uint64_t at = webp_plan_layout<false>(plain, plain.S, img, H_plain, L, plain.S.w, nullptr, 0u);
    const WebpShape S = webp_shape(n ? rec.packed_w : plain.S.w, plain.S.h);
    bool indexed = false;
    if (n) {                                                   // (the whole workgroup)
        const uint64_t at_packed = webp_plan_layout<true>(packed, S, img, H_packed, L, plain.S.w, pal, n);
        indexed = webp_file_bytes(at_packed) < webp_file_bytes(at);
        if (indexed) at = at_packed;
    }
    if (tid == 0u) {
        overflow = webp_file_bytes(at) > plain.file_pitch ? 1u : 0u;
        plain.image[4u * img] = overflow;
        plain.image[4u * img + 1u] = static_cast<uint32_t>((at + 7u) >> 3);
        plain.image[4u * img + 3u] = indexed ? 1u : 0u;
    }
    __syncthreads();
    if (overflow) return;                                      // (the whole workgroup) nothing of this image is written
    if (indexed) webp_write_head<true>(packed, S, img, H_packed, L, pal, n);
    else webp_write_head<false>(plain, plain.S, img, H_plain, L, nullptr, 0u);
}

// ---- emit: blockIdx.z is the variant; the one the layout did not pick writes nothing ---------------------------------------------------
__global__ __launch_bounds__(1024) void webp_ix_emit_kernel(const WebpArgs plain, const WebpArgs packed, const WebpIndexArgs ix) {
    const uint32_t img = blockIdx.y, variant = blockIdx.z;
    if (plain.image[4u * img] || plain.image[4u * img + 3u] != variant) return;
    const uint32_t n_segs = plain.S.n_segs;                    // (the grid's: the stage's full geometry)
    if (variant == 0u) {
        if (blockIdx.x >= n_segs) webp_emit_group_header(plain, blockIdx.x - n_segs, img);
        else webp_emit_segment(plain, plain.S, blockIdx.x, img);
        return;
    }
    if (blockIdx.x >= n_segs) { webp_emit_group_header(packed, blockIdx.x - n_segs, img); return; }
    const WebpShape S = webp_shape(ix.rec[img].packed_w, packed.S.h);
    if (blockIdx.x < S.n_segs) webp_emit_segment(packed, S, blockIdx.x, img);
}

int webp_indexed_front(const WebpArgs& packed, const WebpIndexArgs& ix, hipStream_t st) {
    const WebpShape& S = packed.S;
    const uint32_t npix = S.w * S.h;
    HIP_TRY(hipMemsetAsync(ix.sets, 0, static_cast<size_t>(packed.n_images) * kWebpSetWords * sizeof(uint32_t), st));
    hipLaunchKernelGGL(webp_ix_count_kernel, dim3((npix + kWebpCountPixels - 1u) / kWebpCountPixels, packed.n_images), dim3(256), 0, st, packed, ix);
    hipLaunchKernelGGL(webp_ix_palette_kernel, dim3(packed.n_images), dim3(kWebpSetSlots), 0, st, packed, ix);
    hipLaunchKernelGGL(webp_ix_bundle_kernel, dim3((npix + 255u) / 256u, packed.n_images), dim3(256), 0, st, packed, ix);
    return IFHIP_OK;
}

int webp_indexed_back(const WebpArgs& plain, const WebpArgs& packed, const WebpIndexArgs& ix, hipStream_t st) {
    const WebpShape& S = plain.S;
    hipLaunchKernelGGL(webp_ix_parse_kernel, dim3(S.n_segs, plain.n_images), dim3(1024), 0, st, packed, ix);
    hipLaunchKernelGGL(webp_ix_codes_kernel, dim3(S.n_bands, plain.n_images), dim3(256), 0, st, packed, ix);
    hipLaunchKernelGGL(webp_ix_layout_kernel, dim3(plain.n_images), dim3(1024), 0, st, plain, packed, ix);
    hipLaunchKernelGGL(webp_ix_emit_kernel, dim3(S.n_segs + S.n_bands, plain.n_images, 2), dim3(1024), 0, st, plain, packed, ix);
    return IFHIP_OK;
}

}  // namespace ifhip
