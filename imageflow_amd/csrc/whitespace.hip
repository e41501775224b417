// whitespace.hip -- gfx950 kernels + C ABI for graphics/whitespace.rs::detect_content (:284-634), the detector behind
// CropWhitespace (flow/nodes/clone_crop_fill_expand.rs:564-627) and the querystring's trim.* keys.
//
// The reference is a SEQUENTIAL search: regions in a fixed order, each cut into overlapping windows of at most 2048 pixels
// that are skipped, shrunk or shifted against the box found so far; inside a window every interior pixel whose Scharr
// magnitude exceeds the threshold widens the box by a 3x3-local extent.  Which pixels are visited depends on that order, so
// a one-pass box over the whole frame is a different answer.  Two launches per batch:
//   codes pass   grid-wide, HBM-bound: grey (approximate_grayscale, :437-529) of a 64x16 tile plus a 1-px halo in LDS,
//                one code byte per interior centre -- 0xFF = no hit, else the local extents of :574-615 -- and one
//                "any hit" byte per tile (block-wide OR, stored once by the owning workgroup).
//   replay pass  one workgroup per frame runs the reference's control flow exactly.  A centre's hit and extents depend on
//                its 3x3 grey neighbourhood only, never on the window that visits it, so a window's effect on the box is
//                the min/max over the codes of its interior.  The 256 lanes evaluate the next 256 windows under the current
//                box at once and find the first whose tiles hold a hit: every window before it is excluded or hit-free,
//                leaves the box unchanged and was therefore evaluated under the right box.  That window is reduced exactly,
//                the box updated, and the search resumes behind it.
// Rust release semantics throughout: u32 wrap-around, saturating f32 -> u32 casts, f32 products / quotients before the
// floors and ceils, the area test in i64.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstring>

#include "hip_entry.hpp"

namespace ifhip {
namespace {

constexpr uint32_t kTileW = 64, kTileH = 16, kThreads = 256;
constexpr uint32_t kLdsPitch = kTileW + 4;             // 1-px halo each side, row padded to a multiple of 4
constexpr uint8_t kNoHit = 0xFF;                        // extents fields are 0..2, so all-ones is never a hit's code

struct Geometry {
    uint32_t w, h, stride;
    size_t image_bytes;
    uint32_t code_pitch;                                // bytes per code row (multiple of kTileW)
    size_t code_plane, flag_plane;                      // per-frame bytes of codes and tile flags
    uint32_t tiles_x, tiles_y;
};

__device__ __forceinline__ uint8_t grey_of(uint32_t px, bool alpha) {
    const uint32_t s = 233u * (px & 255u) + 1197u * ((px >> 8) & 255u) + 610u * ((px >> 16) & 255u);
    if (alpha) {                                                                 // Bgra32 (:477-490): div_ceil by 2^19
        const uint32_t g = (s * (px >> 24) + 524287u) >> 19;
        return static_cast<uint8_t>(g > 255u ? 255u : g);
    }
    return static_cast<uint8_t>(s >> 11);                                       // Bgr32 (:506-519)
}

// sobel_scharr_detect's per-centre part (:549-615) on the 3x3 neighbourhood a[row][col]
__device__ __forceinline__ uint8_t centre_code(const int a[3][3], int thr) {
    const int gx = 3 * a[0][0] + 10 * a[1][0] + 3 * a[2][0] - 3 * a[0][2] - 10 * a[1][2] - 3 * a[2][2];
    const int gy = 3 * a[0][0] + 10 * a[0][1] + 3 * a[0][2] - 3 * a[2][0] - 10 * a[2][1] - 3 * a[2][2];
    if (!(abs(gx) + abs(gy) > thr)) return kNoHit;
    uint32_t mnx = 2, mxx = 1, mny = 2, mxy = 1;
#pragma unroll
    for (uint32_t m = 0; m < 3; ++m) {
        const bool h1 = abs(a[m][0] - a[m][1]) > thr, h2 = abs(a[m][1] - a[m][2]) > thr;   // vertical edges in row m
        if (h1) mnx = min(mnx, 1u);
        if (h2) mxx = max(mxx, 2u);
        if (h1 || h2) { mny = min(mny, m); mxy = max(mxy, m + 1u); }
        const bool v1 = abs(a[0][m] - a[1][m]) > thr, v2 = abs(a[1][m] - a[2][m]) > thr;   // horizontal edges in column m
        if (v1) mny = min(mny, 1u);
        if (v2) mxy = max(mxy, 2u);
        if (v1 || v2) { mnx = min(mnx, m); mxx = max(mxx, m + 1u); }
    }
    return static_cast<uint8_t>(mnx | ((mxx - 1u) << 2) | (mny << 4) | ((mxy - 1u) << 6));
}

__global__ void __launch_bounds__(kThreads) codes_kernel(const uint8_t* __restrict__ src, const Geometry g, uint8_t* __restrict__ codes,
                                                         uint8_t* __restrict__ flags, const int alpha, const int thr, const uint32_t vec16) {
    __shared__ uint8_t grey[kTileH + 2][kLdsPitch];
    const uint32_t t = threadIdx.x, img = blockIdx.z;
    const uint32_t x0 = blockIdx.x * kTileW, y0 = blockIdx.y * kTileH;
    const uint8_t* frame = src + static_cast<size_t>(img) * g.image_bytes;
    // body: 18 rows x 16 groups of 4 pixels, 16-byte loads where the rows allow
    for (uint32_t i = t; i < (kTileH + 2) * (kTileW / 4); i += kThreads) {
        const uint32_t ry = i >> 4, q = i & 15u;
        const int64_t gy = static_cast<int64_t>(y0) + ry - 1;
        const uint32_t gx = x0 + 4u * q;
        uint32_t px[4] = {0, 0, 0, 0};
        if (gy >= 0 && gy < g.h && gx < g.w) {
            const uint32_t* row = reinterpret_cast<const uint32_t*>(frame + static_cast<size_t>(gy) * g.stride);
            if (vec16 && gx + 3u < g.w) {
                const uint4 v = *reinterpret_cast<const uint4*>(row + gx);
                px[0] = v.x; px[1] = v.y; px[2] = v.z; px[3] = v.w;
            } else {
                for (uint32_t k = 0; k < 4u && gx + k < g.w; ++k) px[k] = row[gx + k];
            }
        }
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) grey[ry][1 + 4 * q + k] = grey_of(px[k], alpha != 0);
    }
    // halo columns x0 - 1 and x0 + 64
    for (uint32_t i = t; i < 2 * (kTileH + 2); i += kThreads) {
        const uint32_t ry = i >> 1, right = i & 1u;
        const int64_t gy = static_cast<int64_t>(y0) + ry - 1;
        const int64_t gx = right ? static_cast<int64_t>(x0) + kTileW : static_cast<int64_t>(x0) - 1;
        uint32_t px = 0;
        if (gy >= 0 && gy < g.h && gx >= 0 && gx < g.w)
            px = reinterpret_cast<const uint32_t*>(frame + static_cast<size_t>(gy) * g.stride)[gx];
        grey[ry][right ? kTileW + 1 : 0] = grey_of(px, alpha != 0);
    }
    __syncthreads();
    const uint32_t q = t & 15u, r = t >> 4, y = y0 + r;
    uint32_t packed = 0;
    bool any = false;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        const uint32_t x = x0 + 4u * q + k, c = 1u + 4u * q + k;
        uint8_t code = kNoHit;
        if (x >= 1u && x + 1u < g.w && y >= 1u && y + 1u < g.h) {               // interior centres only
            int a[3][3];
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) a[dy][dx] = grey[r + dy][c - 1 + dx];
            code = centre_code(a, thr);
        }
        any = any || code != kNoHit;
        packed |= static_cast<uint32_t>(code) << (8 * k);
    }
    if (y < g.h)                                                                 // code_pitch is a multiple of 64: in bounds
        *reinterpret_cast<uint32_t*>(codes + img * g.code_plane + static_cast<size_t>(y) * g.code_pitch + x0 + 4u * q) = packed;
    const int tile_any = __syncthreads_or(any ? 1 : 0);
    if (t == 0) flags[img * g.flag_plane + static_cast<size_t>(blockIdx.y) * g.tiles_x + blockIdx.x] = tile_any ? 1 : 0;
}

// ---- replay ------------------------------------------------------------------------------------------------------------
enum Edge : uint32_t { kTop = 0, kRight = 1, kBottom = 2, kLeft = 3, kNonDirectional = 4 };
struct Region { uint32_t edge; float x1, y1, x2, y2; };
// SCAN_QUICK_REGIONS (:30-123), SCAN_EVERYTHING_INWARD (:125-154), SCAN_FULL (:155-161); note x1%/x2% = y1%/y2%
__constant__ Region kRegions[17] = {
    {kLeft, 0.f, .5f, .5f, .5f}, {kRight, .5f, .5f, 1.f, .5f}, {kLeft, 0.f, .677f, .5f, .677f}, {kRight, .5f, .677f, 1.f, .677f},
    {kLeft, 0.f, .333f, .5f, .333f}, {kRight, .5f, .333f, 1.f, .333f}, {kTop, .5f, 0.f, .5f, .5f}, {kTop, .677f, 0.f, .677f, .5f},
    {kTop, .333f, 0.f, .333f, .5f}, {kBottom, .5f, .5f, .5f, 1.f}, {kBottom, .677f, .5f, .677f, 1.f}, {kBottom, .333f, .5f, .333f, 1.f},
    {kTop, 0.f, 0.f, 1.f, 1.f}, {kRight, 0.f, 0.f, 1.f, 1.f}, {kBottom, 0.f, 0.f, 1.f, 1.f}, {kLeft, 0.f, 0.f, 1.f, 1.f},
    {kNonDirectional, 0.f, 0.f, 1.f, 1.f}};
constexpr int kFirstInward = 12, kFull = 16;

struct Box { uint32_t min_x, max_x, min_y, max_y; };

__device__ __forceinline__ uint32_t f2u32(float v) {                              // `f32 as u32`: saturating, NaN -> 0
    return !(v > 0.f) ? 0u : v >= 4294967295.f ? UINT_MAX : static_cast<uint32_t>(v);
}

// get_search_rect (:214-282); false = None
__device__ bool search_rect(const Region& rg, uint32_t W, uint32_t H, const Box& s, uint32_t* r) {
    uint32_t x1 = min(W, f2u32(floorf(rg.x1 * static_cast<float>(W - 1u))));
    uint32_t x2 = min(W, f2u32(floorf(rg.x2 * static_cast<float>(W - 1u))));
    uint32_t y1 = min(H, f2u32(floorf(rg.y1 * static_cast<float>(H - 1u))));
    uint32_t y2 = min(H, f2u32(floorf(rg.y2 * static_cast<float>(H - 1u))));
    if (rg.edge == kLeft) { x1 = 0; x2 = min(x2, s.min_x); }
    else if (rg.edge == kRight) { x1 = max(x1, s.max_x); x2 = W; }
    else if (rg.edge == kTop) { y1 = 0; y2 = min(y2, s.min_y); }
    else if (rg.edge == kBottom) { y1 = max(y1, s.max_y); y2 = H; }
    if (x1 == x2 || y1 == y2) return false;
    const uint32_t mrw = (rg.edge == kRight || rg.edge == kLeft) ? 3u : 7u;
    const uint32_t mrh = (rg.edge == kTop || rg.edge == kBottom) ? 3u : 7u;
    while (y2 - y1 < mrh && (y1 > 0u || y2 < H)) { y1 = y1 > 0u ? y1 - 1u : 0u; y2 = min(H, y2 + 1u); }
    while (x2 - x1 < mrw && (x1 > 0u || x2 < W)) { x1 = x1 > 0u ? x1 - 1u : 0u; x2 = min(W, x2 + 1u); }
    r[0] = x1; r[1] = y1; r[2] = x2; r[3] = y2;
    return true;
}

struct Scan { uint32_t x1, y1, x2, y2, ww, wh, hwin, total; };

// check_region's window k (:367-415) under box s; false = the window is excluded (`continue`)
__device__ bool window_at(const Scan& sc, uint32_t k, uint32_t W, uint32_t H, const Box& s, uint32_t* wx, uint32_t* wy, uint32_t* ww_, uint32_t* wh_) {
    const uint32_t row = k / sc.hwin, col = k - row * sc.hwin;
    uint32_t bx = sc.x1 + (sc.ww - 2u) * col, by = sc.y1 + (sc.wh - 2u) * row;
    uint32_t bw = min(max(3u, sc.x2 - bx), sc.ww), bh = min(max(3u, sc.y2 - by), sc.wh);
    const uint32_t bx2 = bx + bw, by2 = by + bh;
    const bool ex_x = s.min_x < bx && s.max_x > bx2, ex_y = s.min_y < by && s.max_y > by2;
    if (ex_x && ex_y) return false;
    if (ex_y && s.min_x < bx2 && bx2 < s.max_x) bw = max(3u, s.min_x - bx);
    else if (ex_y && s.max_x > bx && bx > s.min_x) { bx = min(bx2 - 3u, s.max_x); bw = bx2 - bx; }
    if (ex_x && s.min_y < by2 && by2 < s.max_y) bh = max(3u, s.min_y - by);
    else if (ex_x && s.max_y > by && by > s.min_y) { by = min(by2 - 3u, s.max_y); bh = by2 - by; }
    if (by + bh > H) { if (bh <= H) by = H - bh; else { by = 0; bh = H; } }
    if (bx + bw > W) { if (bw <= W) bx = W - bw; else { bx = 0; bw = W; } }
    *wx = bx; *wy = by; *ww_ = bw; *wh_ = bh;
    return true;
}

// interior centres of a window, clamped to the frame's interior (a no-op for every window the reference can form; it keeps
// each read inside the code plane whatever the arithmetic above produced)
__device__ __forceinline__ void interior(uint32_t W, uint32_t H, uint32_t bx, uint32_t by, uint32_t bw, uint32_t bh,
                                         uint32_t* cx0, uint32_t* cy0, uint32_t* cx1, uint32_t* cy1) {
    *cx0 = max(bx + 1u, 1u); *cy0 = max(by + 1u, 1u);
    *cx1 = min(bx + bw - 2u, W - 2u); *cy1 = min(by + bh - 2u, H - 2u);            // inclusive
}

__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, static_cast<uint32_t>(__shfl_xor(static_cast<int>(v), o, 64)));
    return v;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, static_cast<uint32_t>(__shfl_xor(static_cast<int>(v), o, 64)));
    return v;
}

// block-wide min of a/b and max of c/d; every lane gets the result
__device__ void block_reduce(uint32_t (*red)[4], uint32_t* a, uint32_t* b, uint32_t* c, uint32_t* d) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t ra = wave_min(*a), rb = wave_min(*b), rc = wave_max(*c), rd = wave_max(*d);
    if (lane == 0) { red[wave][0] = ra; red[wave][1] = rb; red[wave][2] = rc; red[wave][3] = rd; }
    __syncthreads();
    uint32_t oa = red[0][0], ob = red[0][1], oc = red[0][2], od = red[0][3];
#pragma unroll
    for (uint32_t i = 1; i < kThreads / 64; ++i) { oa = min(oa, red[i][0]); ob = min(ob, red[i][1]); oc = max(oc, red[i][2]); od = max(od, red[i][3]); }
    __syncthreads();                                                             // red is reused by the next call
    *a = oa; *b = ob; *c = oc; *d = od;
}

__device__ void check_region(const Region& rg, const Geometry& g, const uint8_t* codes, const uint8_t* flags, Box& s, uint32_t (*red)[4]) {
    const uint32_t W = g.w, H = g.h;
    uint32_t r[4];
    if (!search_rect(rg, W, H, s, r)) return;
    Scan sc;
    sc.x1 = r[0]; sc.y1 = r[1]; sc.x2 = r[2]; sc.y2 = r[3];
    const uint32_t w = sc.x2 - sc.x1, h = sc.y2 - sc.y1;
    sc.ww = min(w, rg.edge == kNonDirectional ? 2048u / 7u : 46u);              // :352-359 (ceil(sqrt(2048f32)) = 46)
    sc.wh = min(h, 2048u / sc.ww);
    const uint32_t vwin = f2u32(ceilf(static_cast<float>(h) / static_cast<float>(sc.wh - 2u)));   // :361-362
    sc.hwin = f2u32(ceilf(static_cast<float>(w) / static_cast<float>(sc.ww - 2u)));
    sc.total = vwin * sc.hwin;
    uint32_t k = 0;
    while (k < sc.total) {
        // speculate: lane t takes window k + t under the current box; a candidate may touch a tile with a hit
        uint32_t cand = UINT_MAX;
        const uint32_t idx = k + threadIdx.x;
        uint32_t bx, by, bw, bh;
        if (idx < sc.total && idx >= k && window_at(sc, idx, W, H, s, &bx, &by, &bw, &bh)) {
            uint32_t cx0, cy0, cx1, cy1;
            interior(W, H, bx, by, bw, bh, &cx0, &cy0, &cx1, &cy1);
            if (cx0 <= cx1 && cy0 <= cy1) {
                bool hit = false;
                for (uint32_t ty = cy0 / kTileH; ty <= cy1 / kTileH && !hit; ++ty)
                    for (uint32_t tx = cx0 / kTileW; tx <= cx1 / kTileW && !hit; ++tx) hit = flags[static_cast<size_t>(ty) * g.tiles_x + tx] != 0;
                if (hit) cand = idx;
            }
        }
        uint32_t dummy0 = UINT_MAX, dummy1 = 0, dummy2 = 0;
        block_reduce(red, &cand, &dummy0, &dummy1, &dummy2);
        if (cand == UINT_MAX) { k = (sc.total - k > kThreads) ? k + kThreads : sc.total; continue; }
        // the first such window, exactly (every lane computes the same geometry: the box is uniform)
        (void)window_at(sc, cand, W, H, s, &bx, &by, &bw, &bh);
        uint32_t cx0, cy0, cx1, cy1;
        interior(W, H, bx, by, bw, bh, &cx0, &cy0, &cx1, &cy1);
        uint32_t mnx = UINT_MAX, mny = UINT_MAX, mxx = 0, mxy = 0;
        const uint32_t iw = cx1 - cx0 + 1u, n = iw * (cy1 - cy0 + 1u);
        for (uint32_t i = threadIdx.x; i < n; i += kThreads) {
            const uint32_t yy = i / iw, cy = cy0 + yy, cx = cx0 + (i - yy * iw);
            const uint32_t c = codes[static_cast<size_t>(cy) * g.code_pitch + cx];
            if (c != kNoHit) {                                                   // :617-633
                mnx = min(mnx, cx - 1u + (c & 3u));
                mxx = max(mxx, cx + ((c >> 2) & 3u));
                mny = min(mny, cy - 1u + ((c >> 4) & 3u));
                mxy = max(mxy, cy + ((c >> 6) & 3u));
            }
        }
        block_reduce(red, &mnx, &mny, &mxx, &mxy);
        if (mnx != UINT_MAX) {
            s.min_x = min(s.min_x, mnx); s.max_x = max(s.max_x, mxx);
            s.min_y = min(s.min_y, mny); s.max_y = max(s.max_y, mxy);
        }
        k = cand + 1u;
    }
}

__global__ void __launch_bounds__(kThreads) replay_kernel(const Geometry g, const uint8_t* __restrict__ codes, const uint8_t* __restrict__ flags,
                                                          uint32_t* __restrict__ rects) {
    __shared__ uint32_t red[kThreads / 64][4];
    const uint32_t img = blockIdx.x, W = g.w, H = g.h;
    uint32_t* out = rects + 4u * img;
    if (W < 3u || H < 3u) {                                                      // :288-290
        if (threadIdx.x == 0) { out[0] = 0; out[1] = 0; out[2] = W; out[3] = H; }
        return;
    }
    const uint8_t* c = codes + img * g.code_plane;
    const uint8_t* f = flags + img * g.flag_plane;
    Box s{W, 0u, H, 0u};
    for (int i = 0; i < kFirstInward; ++i) check_region(kRegions[i], g, c, f, s, red);   // :304-306
    const int64_t area = static_cast<int64_t>(s.min_x) * H + static_cast<int64_t>(s.min_y) * W      // :309-312
                         + (static_cast<int64_t>(W) - s.max_x) * H + (static_cast<int64_t>(H) - s.max_y) * W;
    if (area > static_cast<int64_t>(H) * W) check_region(kRegions[kFull], g, c, f, s, red);
    else for (int i = kFirstInward; i < kFull; ++i) check_region(kRegions[i], g, c, f, s, red);
    if (threadIdx.x == 0) {
        if (s.min_x == W && s.max_x == 0u && s.min_y == H && s.max_y == 0u) { out[0] = 0; out[1] = 0; out[2] = W; out[3] = H; }   // :326-333
        else { out[0] = s.min_x; out[1] = s.min_y; out[2] = s.max_x; out[3] = s.max_y; }
    }
}

}  // namespace
}  // namespace ifhip

using namespace ifhip;

extern "C" {

int ifhip_detect_content_batch_device(const uint8_t* d_bgra, size_t image_bytes, uint32_t n_images, uint32_t w, uint32_t h,
                                      uint32_t stride, int alpha_meaningful, uint32_t threshold, uint32_t* d_rects, void* hip_stream) {
    if (n_images == 0) return IFHIP_OK;
    if (!d_rects) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: null rectangle pointer");
    if (w == 0 || h == 0) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: Bitmap dimensions cannot be zero");
    if (w > static_cast<uint32_t>(INT32_MAX) || h > static_cast<uint32_t>(INT32_MAX))
        return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: Bitmap dimension overflow");                  // :285-287
    int rc = check_frames(d_bgra, image_bytes, w, h, stride, "bitmap");
    if (rc) return rc;
    if (reinterpret_cast<uintptr_t>(d_rects) & 3u) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: rectangles must be 4-byte aligned");
    if (h > 65535u * kTileH || n_images > 65535u) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: more than 65535 images per launch or too tall a bitmap");
    if ((rc = require_gfx950(nullptr))) return rc;
    const hipStream_t st = static_cast<hipStream_t>(hip_stream);
    Geometry g{};
    g.w = w; g.h = h; g.stride = stride; g.image_bytes = image_bytes;
    g.tiles_x = (w + kTileW - 1u) / kTileW; g.tiles_y = (h + kTileH - 1u) / kTileH;
    g.code_pitch = g.tiles_x * kTileW;
    g.code_plane = static_cast<size_t>(g.code_pitch) * h;
    g.flag_plane = (static_cast<size_t>(g.tiles_x) * g.tiles_y + 63u) & ~static_cast<size_t>(63);
    const size_t per_image = g.code_plane + g.flag_plane;
    uint8_t* scratch = nullptr;
    HIP_TRY(static_cast<hipError_t>(cached_malloc_for_stream(reinterpret_cast<void**>(&scratch), per_image * n_images, st, true)));
    uint8_t* codes = scratch;
    uint8_t* flags = scratch + g.code_plane * n_images;
    const int thr = static_cast<int>(threshold);                                 // `search.threshold as i32` (:540)
    const uint32_t vec16 = ((reinterpret_cast<uintptr_t>(d_bgra) | image_bytes | stride) & 15u) == 0 ? 1u : 0u;
    hipLaunchKernelGGL(codes_kernel, dim3(g.tiles_x, g.tiles_y, n_images), dim3(kThreads), 0, st, d_bgra, g, codes, flags,
                       alpha_meaningful ? 1 : 0, thr, vec16);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) {
        hipLaunchKernelGGL(replay_kernel, dim3(n_images), dim3(kThreads), 0, st, g, codes, flags, d_rects);
        e = hipGetLastError();
    }
    const hipError_t fe = static_cast<hipError_t>(cached_free_after(scratch, st));
    HIP_TRY(e);
    HIP_TRY(fe);
    return IFHIP_OK;
}

int ifhip_detect_content(const uint8_t* bgra, uint32_t w, uint32_t h, uint32_t stride, int alpha_meaningful, uint32_t threshold,
                         uint32_t* rect) {
    if (!rect) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: null rectangle pointer");
    HostFrame s;
    int rc = s.up(bgra, w, h, stride, 16u);
    if (rc) return rc;
    if ((rc = ifhip_detect_content_batch_device(s.d, s.image_bytes, 1, w, h, stride, alpha_meaningful, threshold,
                                                reinterpret_cast<uint32_t*>(s.side_output()), nullptr))) return rc;
    return s.down(nullptr, rect);
}

}  // extern "C"
