// jpeg_trellis_core.hpp -- the arithmetic of the mozjpeg preset's rate-distortion optimised ("trellis") quantisation
// (codecs/mozjpeg.rs:37-59 selects mozjpeg's defaults; jcdctmgr.c quantize_trellis is the routine this stands in for), in
// lane-sized pieces that compile for the gfx950 kernels (csrc/jpeg_trellis.hip) AND for a plain host compiler:
// tests/jpeg_trellis_emulate.cpp runs the same routines on the CPU and defines the coder.  This is an integer restatement
// of the published algorithm, not mozjpeg's bytes.  Integers and fixed point only.
//
// Per frame and table class (0 luma, 1 chroma):
//   plain pass   the raw forward DCT outputs (scaled by 8, as jfdctint.c leaves them) are quantised as jcdctmgr.c does;
//                the sequential AC symbols (run/size, ZRL, EOB) of the real blocks are counted
//   rate table   counts + 1 on each of the 162 legal AC symbols -> jpeg_gen_optimal_table's code lengths (the huff_* pieces
//                of jpeg_encode_progressive_core.hpp): len[256], a MODEL of the rate; the file's own tables are built
//                later from the trellis output
//   trellis      per real block, AC only: for zigzag position i with magnitude a_i = |x_i|, step 8 * Q_i and plain level
//                q_i = (a_i + 4 Q_i) / (8 Q_i), the candidate levels are 0, q_i and (where q_i >= 2) q_i - 1, with x_i's sign.
//                    J = sum_i w_i * (a_i - level_i * 8 Q_i)^2 + lambda_b * R
//                R: the run/size code lengths of the sequential coding + magnitude bits; a run of 16 and more pays its
//                ZRLs; EOB is paid unless position 63 is not zero.
//
// Ranges (what rules out overflow; the emulation counts violations of the two guards below and the tests assert 0):
//   a_i <= 32768 (int16); for 8-bit samples the forward stage gives a_i < 2^14 (see csrc/jpeg_forward.hip)
//   w_i = floor(2^22 / Q_i^2): 2^22 at Q = 1, 64 at Q = 255
//   e_i = a_i - level * 8 Q_i: level <= q_i, so -4 Q_i <= e_i <= a_i and e_i^2 <= 2^30; w_i * e_i^2 <= 2^52 (Q = 1: at most
//         2^22 * 2^30; Q = 255: at most 64 * 2^30 = 2^36); 63 of them < 2^58
//   lambda_b = (2^(14.75 + 22) / (2^16.5 + sum a_i^2 / 63)) * lambda_scale / 256 <= 2^20.25 * 2^8 = 2^28.25 for
//         lambda_scale <= 65535 (sum a_i^2 <= 63 * 2^30 < 2^36)
//   R <= 63 * (16 + 10) + 3 * 16 + 16 < 2^11, so lambda_b * R < 2^40 and J < 2^59: int64, with kTrInf = 2^62 for "no
//         such state" (a sum of kTrInf and a rate term stays below 2^63)
#pragma once
#include <cstdint>

#include "jpeg_encode_progressive_core.hpp"

namespace ifhip {

constexpr uint32_t kTrLanes = 16;                    // lanes that share a block
constexpr uint32_t kTrWeightShift = 22;              // w_i = 2^22 / Q_i^2
// mozjpeg's published defaults for the block factor, lambda_log_scale1 = 14.75 and lambda_log_scale2 = 16.5 (its
// HVS-PSNR tuning): lambda = 2^scale1 / (2^scale2 + mean AC energy), here in the units of w (2^22)
constexpr uint64_t kTrLambdaNum = 115571923291ull;   // round(2^(14.75 + 22))
constexpr uint64_t kTrLambdaDen = 92682ull;          // round(2^16.5)
constexpr uint32_t kTrLambdaOne = 256;               // lambda_scale of the tuned default (8 fraction bits)
constexpr uint32_t kTrLambdaMax = 65535;
constexpr uint32_t kTrMaxSize = 10;                  // AC magnitude category of 8-bit JPEG
constexpr int64_t kTrInf = 1ll << 62;

// jcdctmgr.c quantize: round-half-up division of |x| by 8 Q
IFHIP_HD uint32_t trellis_plain_level(uint32_t a, uint32_t Q) { return (a + 4u * Q) / (8u * Q); }
IFHIP_HD int32_t trellis_plain(int32_t x, uint32_t Q) {
    const int32_t q = static_cast<int32_t>(trellis_plain_level(static_cast<uint32_t>(x < 0 ? -x : x), Q));
    return x < 0 ? -q : q;
}
IFHIP_HD uint32_t trellis_weight(uint32_t Q) { return (1u << kTrWeightShift) / (Q * Q); }
IFHIP_HD int64_t trellis_dist(uint32_t a, uint32_t level, uint32_t Q, uint32_t w) {
    const int64_t e = static_cast<int64_t>(a) - static_cast<int64_t>(level * 8u * Q);
    return static_cast<int64_t>(w) * (e * e);
}
// the block factor: falls with the block's AC energy (sum of a_i^2, i = 1..63)
IFHIP_HD uint64_t trellis_lambda(uint64_t energy, uint32_t lambda_scale) {
    return (kTrLambdaNum / (kTrLambdaDen + energy / 63u)) * lambda_scale >> 8;
}
// the magnitude category; the second result says the level is outside 8-bit JPEG (guard: never with the forward stage's planes)
IFHIP_HD uint32_t trellis_size(uint32_t level) {
    const uint32_t n = enc_nbits(level);
    return n > kTrMaxSize ? kTrMaxSize : n;
}
IFHIP_HD bool trellis_legal_ac(uint32_t sym) { return sym == 0u || sym == 0xF0u || ((sym & 15u) >= 1u && (sym & 15u) <= kTrMaxSize); }
// bits of a coefficient of category `size` behind `run` zeros
IFHIP_HD uint32_t trellis_rate(const uint8_t* len, uint32_t run, uint32_t size) {
    return (run >> 4) * len[0xF0] + len[((run & 15u) << 4) | size] + size;
}

// The sequential AC symbols of a block (jchuff.c encode_one_block): level(k), k = 1..63 in zigzag order; add(symbol).
template <class Level, class Add>
IFHIP_HD void trellis_count_ac(const Level& level, Add add) {
    uint32_t run = 0;
    for (uint32_t k = 1; k < 64u; ++k) {
        const int32_t v = level(k);
        if (v == 0) { ++run; continue; }
        for (; run > 15u; run -= 16u) add(0xF0u);
        add((run << 4) | trellis_size(static_cast<uint32_t>(v < 0 ? -v : v)));
        run = 0;
    }
    if (run) add(0u);
}

// J of a block for given level magnitudes -- the stand-alone statement of the cost the search minimises (the tests
// enumerate with it).  a(k), Q(k), level(k): zigzag position k = 1..63.
template <class Mag, class Quant, class Level>
IFHIP_HD int64_t trellis_block_cost(const Mag& a, const Quant& Q, const Level& level, const uint8_t* len, uint64_t lambda) {
    int64_t dist = 0;
    uint32_t bits = 0, run = 0;
    for (uint32_t k = 1; k < 64u; ++k) {
        const uint32_t l = level(k);
        dist += trellis_dist(a(k), l, Q(k), trellis_weight(Q(k)));
        if (!l) { ++run; continue; }
        bits += trellis_rate(len, run, trellis_size(l));
        run = 0;
    }
    if (run) bits += len[0];
    return dist + static_cast<int64_t>(lambda * bits);
}

// ---- the search ---------------------------------------------------------------------------------------------------------
// State (i, c): the block's last coefficient so far that is not zero lies at i, with candidate c (0: q_i, 1: q_i - 1).  With
// Z_t = w_t a_t^2 (what zeroing position t costs) and P its prefix sum, the best cost of (i, c) over every earlier last
// position j (j = 0: none) is
//     D(i, c) + P[i - 1] + min_j ( best[j] - P[j] + lambda * rate(i - j - 1, size_c) )
// so the search carries B[j] = best[j] - P[j] (B[0] = 0) and never needs P itself:
//     B[i] = min_c ( D(i, c) + min_j (B[j] + lambda * rate) ) - Z_i
// and a block that ends at i costs B[i] + P[63] + (i < 63 ? lambda * len[EOB] : 0); i = 0 is the all-zero block.
// Ties go to the plain level (c = 0), to the later predecessor and to the longer block: with lambda = 0 the result is the
// plain quantiser's.
//
// One lane's part of min_j for both candidates: predecessors j = lane, lane + kTrLanes, ... below i.  B[j] = kTrInf where
// q_j = 0 (no state).  cost[c] / pred[c]: the lane's minimum and the LARGEST j that attains it.
IFHIP_HD void trellis_lane_scan(const int64_t* B, const uint8_t* len, uint64_t lambda, uint32_t i, uint32_t size0, uint32_t size1, bool two,
                                uint32_t lane, int64_t (&cost)[2], uint32_t (&pred)[2]) {
    cost[0] = cost[1] = INT64_MAX;
    pred[0] = pred[1] = 0;
    for (uint32_t j = lane; j < i; j += kTrLanes) {
        const int64_t b = B[j];
        const uint32_t run = i - j - 1u;
        const int64_t c0 = b + static_cast<int64_t>(lambda * trellis_rate(len, run, size0));
        if (c0 <= cost[0]) { cost[0] = c0; pred[0] = j; }
        if (two) {
            const int64_t c1 = b + static_cast<int64_t>(lambda * trellis_rate(len, run, size1));
            if (c1 <= cost[1]) { cost[1] = c1; pred[1] = j; }
        }
    }
}
// B[i] and the candidate chosen at i from the reduced minima m[c] (q >= 1; two: q >= 2)
IFHIP_HD int64_t trellis_close(uint32_t a, uint32_t q, uint32_t Q, bool two, const int64_t (&m)[2], uint32_t* choice) {
    const uint32_t w = trellis_weight(Q);
    const int64_t t0 = m[0] + trellis_dist(a, q, Q, w);
    const int64_t t1 = two ? m[1] + trellis_dist(a, q - 1u, Q, w) : INT64_MAX;
    *choice = t1 < t0 ? 1u : 0u;
    return (t1 < t0 ? t1 : t0) - trellis_dist(a, 0u, Q, w);
}
// what ending the block at i adds to B[i] (the common P[63] left out); no state: kTrInf stays far above every real cost
IFHIP_HD int64_t trellis_end_cost(int64_t Bi, uint32_t i, const uint8_t* len, uint64_t lambda) {
    return Bi + (i < 63u ? static_cast<int64_t>(lambda * len[0]) : 0);
}

}  // namespace ifhip
