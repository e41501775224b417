// jpeg_trellis.hip -- gfx950 kernels + C ABI of the mozjpeg preset's trellis quantisation (codecs/mozjpeg.rs:37-59 selects
// mozjpeg's defaults; jcdctmgr.c quantize_trellis is the routine this stands in for).  Input: the raw forward DCT planes of
// ifhip_jpeg_forward_raw_batch_device; output: quantised planes in the layout the entropy coders consume.  The arithmetic is
// csrc/jpeg_trellis_core.hpp, shared with tests/jpeg_trellis_emulate.cpp, which defines the result byte for byte.
//
// Launches per call, all images in each, no host round trip between them:
//   plain   (blocks)  quantise as jcdctmgr.c does, count the sequential AC symbols of the real blocks: LDS histograms of the
//                     two table classes per workgroup, one atomic flush
//   table   (classes) one wave per (image, class): counts + 1 on the legal symbols -> jpeg_gen_optimal_table's lengths
//   search  (blocks)  the dynamic programme per real block; dummy blocks are written as zeros
//   dummy DC          jpeg_dummy_dc_kernel of the forward stage
// Mapping of the block kernels (bound: VALU issue; integer work, no MFMA): 16 lanes per block, four blocks per wave, 16 per
// workgroup.  A block's magnitudes, plain levels and search state sit in LDS; at position i the 16 lanes split the
// predecessor positions j < i, the minimum is taken with 16-lane row DPP steps (64-bit compare, no LDS, no scratch), the
// lanes that hold it name the predecessor with an LDS maximum (ties go to the later one).  The lanes of a block share a
// wave: LDS traffic is ordered with wave-level fences, no s_barrier after the tables are staged.
#include <hip/hip_runtime.h>

#include <cstring>
#include <memory>

#include "hip_entry.hpp"
#include "jpeg_forward_geom.hpp"
#include "jpeg_huff_wave.hpp"
#include "jpeg_trellis_core.hpp"
#include "stage_scratch.hpp"

namespace ifhip {

constexpr uint32_t kTrBlocksPerWg = 16, kTrThreads = kTrBlocksPerWg * kTrLanes;

struct TrArgs {
    FwdGeom g;
    const int16_t* raw[3];          // [n_images][bh][bw][64] jpeg_fdct_islow's outputs (scaled by 8), dummy blocks zero
    int16_t* coef[3];               // the same layout, quantised
    const uint16_t* qt;             // [n_images][3][64]
    uint32_t lambda_scale, n_images;
    uint32_t blocks[3], total;      // blocks per plane (dummy blocks included) and their sum
    uint32_t* hist;                 // [n_images][2][256] zero before the plain pass
    uint8_t* len;                   // [n_images][2][256]
};

struct TrBlock {                    // one block's state in LDS
    uint32_t aq[64];                // zigzag order: |x| | plain level << 16 | sign << 31
    uint32_t Q[64];                 // zigzag order: the table entry | candidate chosen << 16
    int64_t B[64];
    uint32_t pred[64][2];
    int16_t out[64];                // natural order
    uint32_t end;
};

__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the minimum over the 16 lanes of a row, in every lane: quad permutes, then rotations by 4 and 8 inside the row
template <int CTRL>
__device__ __forceinline__ int64_t row_step_min(int64_t v) {
    const int lo = __builtin_amdgcn_update_dpp(0, static_cast<int>(static_cast<uint64_t>(v)), CTRL, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(0, static_cast<int>(static_cast<uint64_t>(v) >> 32), CTRL, 0xF, 0xF, false);
    const int64_t o = static_cast<int64_t>(static_cast<uint64_t>(static_cast<uint32_t>(hi)) << 32 | static_cast<uint32_t>(lo));
    return o < v ? o : v;
}
__device__ __forceinline__ int64_t row_min(int64_t v) {
    v = row_step_min<0xB1>(v);      // quad_perm [1, 0, 3, 2]
    v = row_step_min<0x4E>(v);      // quad_perm [2, 3, 0, 1]
    v = row_step_min<0x124>(v);     // row_ror 4
    return row_step_min<0x128>(v);  // row_ror 8
}

// which block a group of 16 lanes works on: component, offset in blocks inside the plane, is it a real block
struct TrWhere { uint32_t c, off; bool real; };
__device__ __forceinline__ TrWhere locate(const TrArgs& a, uint32_t r) {
    uint32_t c = 0;
    if (r >= a.blocks[0]) { r -= a.blocks[0]; c = 1; if (r >= a.blocks[1]) { r -= a.blocks[1]; c = 2; } }
    const uint32_t bw = c == 0 ? a.g.bw[0] : c == 1 ? a.g.bw[1] : a.g.bw[2];
    const uint32_t rbw = c == 0 ? a.g.rbw[0] : c == 1 ? a.g.rbw[1] : a.g.rbw[2], rbh = c == 0 ? a.g.rbh[0] : c == 1 ? a.g.rbh[1] : a.g.rbh[2];
    const uint32_t by = r / bw, bx = r - by * bw;
    return TrWhere{c, r, bx < rbw && by < rbh};
}

// The block's four coefficients of this lane (natural positions 4 lane .. 4 lane + 3, one 8-byte load) into the zigzag
// ordered state: magnitude, plain level, sign, table entry; B = "no state" where the plain level is zero.  Returns the
// lane's share of the AC energy.
__device__ __forceinline__ uint64_t stage_block(const int16_t* src, const uint16_t* qt, uint32_t lane, TrBlock& s) {
    const uint2 v = *reinterpret_cast<const uint2*>(src + lane * 4u);
    const uint32_t words[2] = {v.x, v.y};
    uint64_t energy = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) {
        const uint32_t n = lane * 4u + k;
        const int32_t x = static_cast<int16_t>(words[k >> 1] >> (16u * (k & 1u)));
        const uint32_t a = static_cast<uint32_t>(x < 0 ? -x : x), Q = qt[n];
        const uint32_t q = trellis_plain_level(a, Q);
        const uint32_t z = static_cast<uint32_t>(enc_zigzag_position(static_cast<int>(n)));
        s.aq[z] = a | q << 16 | (x < 0 ? 0x80000000u : 0u);
        s.Q[z] = Q;
        s.B[z] = z == 0u ? 0 : (q ? 0 : kTrInf);
        s.pred[z][0] = 0; s.pred[z][1] = 0;
        s.out[n] = static_cast<int16_t>(n == 0u ? (x < 0 ? -static_cast<int32_t>(q) : static_cast<int32_t>(q)) : 0);
        if (n) energy += static_cast<uint64_t>(a) * a;
    }
    return energy;
}
__device__ __forceinline__ uint32_t level_of(uint32_t aq) { return (aq >> 16) & 0x7FFFu; }

__global__ void __launch_bounds__(kTrThreads) trellis_plain_kernel(const TrArgs a) {
    __shared__ TrBlock blk[kTrBlocksPerWg];
    __shared__ uint16_t qt[192];
    __shared__ uint32_t hist[2 * 256];
    const uint32_t t = threadIdx.x, img = blockIdx.y, lane = t & (kTrLanes - 1u), grp = t / kTrLanes;
    if (t < 192u) qt[t] = a.qt[static_cast<size_t>(img) * 192u + t];
    for (uint32_t s = t; s < 512u; s += kTrThreads) hist[s] = 0u;
    __syncthreads();
    const uint32_t r = blockIdx.x * kTrBlocksPerWg + grp;
    if (r < a.total) {
        const TrWhere w = locate(a, r);
        if (w.real) {
            TrBlock& s = blk[grp];
            const size_t plane = w.c == 0u ? a.blocks[0] : w.c == 1u ? a.blocks[1] : a.blocks[2];
            const int16_t* raw = w.c == 0u ? a.raw[0] : w.c == 1u ? a.raw[1] : a.raw[2];
            stage_block(raw + (static_cast<size_t>(img) * plane + w.off) * 64u, qt + w.c * 64u, lane, s);
            wave_lds_sync();
            if (lane == 0u) {
                uint32_t* h = hist + (w.c ? 256u : 0u);
                trellis_count_ac([&](uint32_t k) { return static_cast<int32_t>(level_of(s.aq[k])); }, [&](uint32_t sym) { atomicAdd(h + sym, 1u); });
            }
        }
    }
    __syncthreads();
    for (uint32_t s = t; s < 512u; s += kTrThreads)
        if (hist[s]) atomicAdd(a.hist + static_cast<size_t>(img) * 512u + s, hist[s]);
}

// one wave per (image, table class): the model's code lengths
__global__ void __launch_bounds__(64) trellis_table_kernel(const TrArgs a) {
    __shared__ uint32_t counts[256], freq[257], codesize[257], bits[33], codes[256];
    __shared__ int32_t others[257];
    __shared__ uint8_t vals[256], dht[kProgDhtPitch];
    const uint32_t lane = threadIdx.x, cls = blockIdx.x, img = blockIdx.y;
    const size_t at = (static_cast<size_t>(img) * 2u + cls) * 256u;
    for (uint32_t i = lane; i < 256u; i += 64u) { counts[i] = trellis_legal_ac(i) ? a.hist[at + i] + 1u : 0u; codes[i] = 0u; vals[i] = 0; }
    __syncthreads();
    huff_init(counts, lane, freq, codesize, others);
    __syncthreads();
    huff_wave_merge(lane, freq, codesize, others);
    if (lane == 0u) huff_limit(codesize, bits);
    for (uint32_t i = lane; i < 256u; i += 64u) if (codesize[i] && codesize[i] <= 32u) vals[huff_rank(codesize, i)] = static_cast<uint8_t>(i);
    __syncthreads();
    if (lane == 0u) huff_emit(bits, vals, 0x10u, dht, codes);
    __syncthreads();
    for (uint32_t i = lane; i < 256u; i += 64u) a.len[at + i] = static_cast<uint8_t>(codes[i] >> 16);
}

__global__ void __launch_bounds__(kTrThreads) trellis_search_kernel(const TrArgs a) {
    __shared__ TrBlock blk[kTrBlocksPerWg];
    __shared__ uint16_t qt[192];
    __shared__ __attribute__((aligned(4))) uint8_t lens[2 * 256];
    const uint32_t t = threadIdx.x, img = blockIdx.y, lane = t & (kTrLanes - 1u), grp = t / kTrLanes;
    if (t < 192u) qt[t] = a.qt[static_cast<size_t>(img) * 192u + t];
    if (t < 128u) reinterpret_cast<uint32_t*>(lens)[t] = reinterpret_cast<const uint32_t*>(a.len + static_cast<size_t>(img) * 512u)[t];
    __syncthreads();
    const uint32_t r = blockIdx.x * kTrBlocksPerWg + grp;
    if (r >= a.total) return;
    const TrWhere w = locate(a, r);
    TrBlock& s = blk[grp];
    const size_t plane = w.c == 0u ? a.blocks[0] : w.c == 1u ? a.blocks[1] : a.blocks[2];
    const size_t at = (static_cast<size_t>(img) * plane + w.off) * 64u;
    int16_t* dst = (w.c == 0u ? a.coef[0] : w.c == 1u ? a.coef[1] : a.coef[2]) + at;
    if (!w.real) {                                      // (a row of 16 lanes is real or not as a whole)
        *reinterpret_cast<uint2*>(dst + lane * 4u) = make_uint2(0u, 0u);
        return;
    }
    const int16_t* raw = (w.c == 0u ? a.raw[0] : w.c == 1u ? a.raw[1] : a.raw[2]) + at;
    const uint8_t* len = lens + (w.c ? 256u : 0u);
    uint64_t energy = stage_block(raw, qt + w.c * 64u, lane, s);
#pragma unroll
    for (int d = 8; d; d >>= 1) energy += __shfl_xor(static_cast<unsigned long long>(energy), d, 16);
    const uint64_t lambda = trellis_lambda(energy, a.lambda_scale);
    if (lane == 0u) s.end = 0u;
    wave_lds_sync();
    for (uint32_t i = 1; i < 64u; ++i) {
        const uint32_t aq = s.aq[i], q = level_of(aq);
        if (q) {                                        // (uniform in the row)
            const bool two = q >= 2u;
            int64_t cost[2], m[2];
            uint32_t pj[2];
            trellis_lane_scan(s.B, len, lambda, i, trellis_size(q), trellis_size(q - 1u), two, lane, cost, pj);
            m[0] = row_min(cost[0]);
            m[1] = two ? row_min(cost[1]) : INT64_MAX;
            if (cost[0] == m[0]) atomicMax(&s.pred[i][0], pj[0]);
            if (two && cost[1] == m[1]) atomicMax(&s.pred[i][1], pj[1]);
            uint32_t choice;
            const uint32_t Q = s.Q[i];
            const int64_t Bi = trellis_close(aq & 0xFFFFu, q, Q, two, m, &choice);
            if (lane == 0u) { s.B[i] = Bi; s.Q[i] = Q | choice << 16; }
        }
        wave_lds_sync();
    }
    // the best end: position i = lane, lane + 16, ...; ties to the longer block
    int64_t e = INT64_MAX;
    uint32_t ei = 0;
    for (uint32_t i = lane; i < 64u; i += kTrLanes) {
        if (i && !level_of(s.aq[i])) continue;
        const int64_t c = trellis_end_cost(s.B[i], i, len, lambda);
        if (c <= e) { e = c; ei = i; }
    }
    if (e == row_min(e)) atomicMax(&s.end, ei);
    wave_lds_sync();
    if (lane == 0u) {
        for (uint32_t i = s.end; i;) {
            const uint32_t aq = s.aq[i], choice = s.Q[i] >> 16;
            const int32_t l = static_cast<int32_t>(level_of(aq) - choice);
            s.out[enc_zigzag(static_cast<int>(i))] = static_cast<int16_t>((aq >> 31) ? -l : l);
            i = s.pred[i][choice];
        }
    }
    wave_lds_sync();
    *reinterpret_cast<uint2*>(dst + lane * 4u) = *reinterpret_cast<const uint2*>(s.out + lane * 4u);
}

}  // namespace ifhip

using namespace ifhip;

struct ifhip_jpeg_trellis_stage {
    FwdGeom g;
    uint32_t max_images = 0;
    uint32_t* d_hist = nullptr;
    uint8_t* d_len = nullptr;
    StageScratch blocks{&d_hist, &d_len};
};

extern "C" {

int ifhip_jpeg_trellis_stage_create(ifhip_jpeg_trellis_stage** stage, uint32_t width, uint32_t height, const uint8_t* h_samp,
                                    const uint8_t* v_samp, uint32_t max_images) {
    if (!stage) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: null stage out-pointer");
    *stage = nullptr;
    if (max_images == 0 || max_images > 65535u) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: 1..65535 images per stage");
    std::unique_ptr<ifhip_jpeg_trellis_stage> s(new ifhip_jpeg_trellis_stage);
    if (int rc = make_fwd_geom(width, height, h_samp, v_samp, &s->g)) return rc;
    uint64_t total = 0;
    for (int c = 0; c < 3; ++c) total += static_cast<uint64_t>(s->g.bw[c]) * s->g.bh[c];
    if (total > 0x7FFFFFFFull) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: more than 2^31 blocks per image");
    s->max_images = max_images;
    const size_t n = max_images;
    if (int rc = s->blocks.ensure([&]() -> int {
            HIP_TRY(DEV_MALLOC(&s->d_hist, n * 512u * sizeof(uint32_t)));
            HIP_TRY(DEV_MALLOC(&s->d_len, n * 512u));
            return IFHIP_OK;
        })) return rc;
    *stage = s.release();
    return IFHIP_OK;
}

void ifhip_jpeg_trellis_stage_destroy(ifhip_jpeg_trellis_stage* stage) { delete stage; }

int ifhip_jpeg_trellis_batch_device(ifhip_jpeg_trellis_stage* stage, const int16_t* d_raw0, const int16_t* d_raw1, const int16_t* d_raw2,
                                    const uint16_t* d_qt, uint32_t lambda_scale, uint32_t n_images, int16_t* d_coef0, int16_t* d_coef1,
                                    int16_t* d_coef2, void* hip_stream) {
    if (!stage) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: null stage");
    if (n_images == 0) return IFHIP_OK;
    if (n_images > stage->max_images) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: %u images exceed the stage capacity %u", n_images, stage->max_images);
    if (!d_raw0 || !d_raw1 || !d_raw2 || !d_qt || !d_coef0 || !d_coef1 || !d_coef2) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: null pointer");
    if (lambda_scale > kTrLambdaMax) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: lambda_scale %u exceeds %u", lambda_scale, kTrLambdaMax);
    uintptr_t bits = 0;
    for (const int16_t* p : {d_raw0, d_raw1, d_raw2, static_cast<const int16_t*>(d_coef0), static_cast<const int16_t*>(d_coef1), static_cast<const int16_t*>(d_coef2)})
        bits |= reinterpret_cast<uintptr_t>(p);
    if (bits & 15u) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: coefficient planes must be 16-byte aligned");
    if (int rc = stage->blocks.check_device()) return rc;
    TrArgs a;
    std::memset(&a, 0, sizeof a);
    a.g = stage->g;
    a.raw[0] = d_raw0; a.raw[1] = d_raw1; a.raw[2] = d_raw2;
    a.coef[0] = d_coef0; a.coef[1] = d_coef1; a.coef[2] = d_coef2;
    a.qt = d_qt; a.lambda_scale = lambda_scale; a.n_images = n_images;
    for (int c = 0; c < 3; ++c) { a.blocks[c] = a.g.bw[c] * a.g.bh[c]; a.total += a.blocks[c]; }
    a.hist = stage->d_hist; a.len = stage->d_len;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    HIP_TRY(hipMemsetAsync(a.hist, 0, static_cast<size_t>(n_images) * 512u * sizeof(uint32_t), st));
    const dim3 grid((a.total + kTrBlocksPerWg - 1u) / kTrBlocksPerWg, n_images);
    hipLaunchKernelGGL(trellis_plain_kernel, grid, dim3(kTrThreads), 0, st, a);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(trellis_table_kernel, dim3(2, n_images), dim3(64), 0, st, a);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(trellis_search_kernel, grid, dim3(kTrThreads), 0, st, a);
    HIP_TRY(hipGetLastError());
    return launch_dummy_dc(a.g, d_coef0, n_images, hip_stream);
}

int ifhip_jpeg_trellis(const int16_t* raw0, const int16_t* raw1, const int16_t* raw2, uint32_t width, uint32_t height, const uint8_t* h_samp,
                       const uint8_t* v_samp, const uint16_t* qt, uint32_t lambda_scale, int16_t* coef0, int16_t* coef1, int16_t* coef2) {
    if (!raw0 || !raw1 || !raw2 || !qt || !coef0 || !coef1 || !coef2) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: null pointer");
    ifhip_jpeg_trellis_stage* stage = nullptr;
    if (int rc = ifhip_jpeg_trellis_stage_create(&stage, width, height, h_samp, v_samp, 1)) return rc;
    std::unique_ptr<ifhip_jpeg_trellis_stage, void (*)(ifhip_jpeg_trellis_stage*)> guard(stage, ifhip_jpeg_trellis_stage_destroy);
    const int16_t* h_raw[3] = {raw0, raw1, raw2};
    int16_t* h_coef[3] = {coef0, coef1, coef2};
    DeviceBlock d_qt, d_raw[3], d_coef[3];
    HIP_TRY(d_qt.alloc(384));
    HIP_TRY(hipMemcpy(d_qt.p, qt, 384, hipMemcpyHostToDevice));
    size_t cb[3];
    for (int c = 0; c < 3; ++c) {
        cb[c] = static_cast<size_t>(stage->g.bw[c]) * stage->g.bh[c] * 128u;
        HIP_TRY(d_raw[c].alloc(cb[c]));
        HIP_TRY(d_coef[c].alloc(cb[c]));
        HIP_TRY(hipMemcpy(d_raw[c].p, h_raw[c], cb[c], hipMemcpyHostToDevice));
    }
    if (int rc = ifhip_jpeg_trellis_batch_device(stage, d_raw[0].as<int16_t>(), d_raw[1].as<int16_t>(), d_raw[2].as<int16_t>(), d_qt.as<uint16_t>(),
                                                 lambda_scale, 1, d_coef[0].as<int16_t>(), d_coef[1].as<int16_t>(), d_coef[2].as<int16_t>(), nullptr))
        return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    for (int c = 0; c < 3; ++c) HIP_TRY(hipMemcpy(h_coef[c], d_coef[c].p, cb[c], hipMemcpyDeviceToHost));
    return IFHIP_OK;
}

}  // extern "C"
