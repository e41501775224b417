// jpeg_trellis_emulate.cpp -- test infrastructure, not part of the product: the mozjpeg preset's pixel half in plain C++.
// BGRA -> YCbCr (jccolor.c), h2v1 / h2v2 down-sampling with libjpeg's edge expansion (jcsample.c, jcprepct.c), the islow
// forward DCT (jfdctint.c, outputs left scaled by 8), then the three passes of csrc/jpeg_trellis.hip with the SAME routines
// (csrc/jpeg_trellis_core.hpp): the plain quantiser and its AC symbol counts, the rate table (jpeg_gen_optimal_table's
// lengths from the huff_* pieces, its minimum searches lane by lane), and the trellis search with its 16 lanes as a loop.
// This emulation DEFINES the coder: the device planes must equal it byte for byte.  guards[0] counts levels outside the
// 10-bit AC categories, guards[1] costs at or above 2^61.  Built by tests/jpeg_trellis_emu.py with g++.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../imageflow_amd/csrc/jpeg_trellis_core.hpp"

using namespace ifhip;

namespace {

int64_t g_guards[2];

int32_t component(const uint8_t* px, int c) {          // jccolor.c rgb_ycc_convert; px = B, G, R, A
    const int32_t b = px[0], g = px[1], r = px[2];
    if (c == 0) return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
    if (c == 1) return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
    return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}

// jfdctint.c jpeg_fdct_islow: CONST_BITS 13, PASS1_BITS 2; the second pass leaves the outputs scaled by 8
void fdct_islow(int32_t* d) {
    constexpr int32_t F0298 = 2446, F0390 = 3196, F0541 = 4433, F0765 = 6270, F0899 = 7373, F1175 = 9633, F1501 = 12299, F1847 = 15137,
                      F1961 = 16069, F2053 = 16819, F2562 = 20995, F3072 = 25172;
    auto descale = [](int32_t x, int n) { return (x + (1 << (n - 1))) >> n; };
    for (int pass = 0; pass < 2; ++pass) {
        const int step = pass ? 8 : 1, next = pass ? 1 : 8;
        for (int i = 0; i < 8; ++i) {
            int32_t* p = d + i * next;
            const int32_t t0 = p[0] + p[7 * step], t7 = p[0] - p[7 * step], t1 = p[step] + p[6 * step], t6 = p[step] - p[6 * step];
            const int32_t t2 = p[2 * step] + p[5 * step], t5 = p[2 * step] - p[5 * step], t3 = p[3 * step] + p[4 * step], t4 = p[3 * step] - p[4 * step];
            const int32_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
            const int sh = pass ? 15 : 11;
            if (!pass) { p[0] = (t10 + t11) * 4; p[4 * step] = (t10 - t11) * 4; }
            else { p[0] = descale(t10 + t11, 2); p[4 * step] = descale(t10 - t11, 2); }
            int32_t z1 = (t12 + t13) * F0541;
            p[2 * step] = descale(z1 + t13 * F0765, sh);
            p[6 * step] = descale(z1 + t12 * -F1847, sh);
            z1 = t4 + t7;
            int32_t z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
            const int32_t z5 = (z3 + z4) * F1175;
            const int32_t a4 = t4 * F0298, a5 = t5 * F2053, a6 = t6 * F3072, a7 = t7 * F1501;
            z1 *= -F0899; z2 *= -F2562; z3 = z3 * -F1961 + z5; z4 = z4 * -F0390 + z5;
            p[7 * step] = descale(a4 + z1 + z3, sh);
            p[5 * step] = descale(a5 + z2 + z4, sh);
            p[3 * step] = descale(a6 + z2 + z3, sh);
            p[step] = descale(a7 + z1 + z4, sh);
        }
    }
}

struct Geom {
    uint32_t w, h, hs[3], vs[3], hmax, vmax, bw[3], bh[3], rbw[3], rbh[3], dw[3], dh[3];
};
bool make_geom(uint32_t w, uint32_t h, const uint8_t* hs, const uint8_t* vs, Geom* g) {
    if (!w || !h || hs[1] != 1 || vs[1] != 1 || hs[2] != 1 || vs[2] != 1 || hs[0] < 1 || hs[0] > 2 || vs[0] < 1 || vs[0] > 2) return false;
    g->w = w; g->h = h; g->hmax = hs[0]; g->vmax = vs[0];
    const uint32_t mw = (w + 8 * g->hmax - 1) / (8 * g->hmax), mh = (h + 8 * g->vmax - 1) / (8 * g->vmax);
    for (int c = 0; c < 3; ++c) {
        g->hs[c] = hs[c]; g->vs[c] = vs[c];
        g->bw[c] = mw * hs[c]; g->bh[c] = mh * vs[c];
        g->dw[c] = (w * hs[c] + g->hmax - 1) / g->hmax; g->dh[c] = (h * vs[c] + g->vmax - 1) / g->vmax;
        g->rbw[c] = (g->dw[c] + 7) / 8; g->rbh[c] = (g->dh[c] + 7) / 8;
    }
    return true;
}

// one down-sampled sample of component c at (x, y); coordinates past the picture repeat its edge
int32_t sample(const uint8_t* bgra, uint32_t stride, const Geom& g, int c, uint32_t x, uint32_t y) {
    const uint32_t fx = c ? g.hmax : 1, fy = c ? g.vmax : 1;
    y = std::min(y, g.dh[c] - 1);                      // rows behind the last down-sampled row repeat it (jcprepct.c)
    int32_t sum = 0;
    for (uint32_t j = 0; j < fy; ++j)
        for (uint32_t i = 0; i < fx; ++i)
            sum += component(bgra + static_cast<size_t>(std::min(y * fy + j, g.h - 1)) * stride + 4 * static_cast<size_t>(std::min(x * fx + i, g.w - 1)), c);
    if (fx == 1 && fy == 1) return sum;
    if (fy == 1) return (sum + static_cast<int32_t>(x & 1)) >> 1;             // h2v1_downsample: bias 0, 1, 0, 1
    return (sum + 1 + static_cast<int32_t>(x & 1)) >> 2;                      // h2v2_downsample: bias 1, 2, 1, 2
}

struct Searched { int16_t level[64]; int64_t cost; };    // natural order

// the search of one block as the device runs it: sequential over positions, kTrLanes lanes per position
Searched search_block(const int16_t* raw, const uint16_t* Q, const uint8_t* len, uint32_t lambda_scale) {
    uint32_t a[64], Qz[64], q[64], choice[64] = {0}, pred[64][2] = {{0}};
    int64_t B[64];
    uint64_t energy = 0;
    for (int k = 0; k < 64; ++k) {
        const int32_t x = raw[enc_zigzag(k)];
        a[k] = static_cast<uint32_t>(x < 0 ? -x : x); Qz[k] = Q[enc_zigzag(k)];
        q[k] = trellis_plain_level(a[k], Qz[k]);
        if (k) { energy += static_cast<uint64_t>(a[k]) * a[k]; if (enc_nbits(q[k]) > kTrMaxSize) ++g_guards[0]; }
    }
    const uint64_t lambda = trellis_lambda(energy, lambda_scale);
    B[0] = 0;
    for (uint32_t i = 1; i < 64; ++i) {
        if (!q[i]) { B[i] = kTrInf; continue; }
        const bool two = q[i] >= 2;
        int64_t m[2] = {INT64_MAX, INT64_MAX};
        uint32_t p[2] = {0, 0};
        for (uint32_t lane = 0; lane < kTrLanes; ++lane) {
            int64_t c[2]; uint32_t pj[2];
            trellis_lane_scan(B, len, lambda, i, trellis_size(q[i]), trellis_size(q[i] - 1), two, lane, c, pj);
            for (int k = 0; k < 2; ++k) if (c[k] < m[k] || (c[k] == m[k] && pj[k] > p[k])) { m[k] = c[k]; p[k] = pj[k]; }
        }
        B[i] = trellis_close(a[i], q[i], Qz[i], two, m, &choice[i]);
        pred[i][0] = p[0]; pred[i][1] = p[1];
        if (B[i] >= (1ll << 61) || B[i] <= -(1ll << 61)) ++g_guards[1];
    }
    int64_t best = trellis_end_cost(0, 0, len, lambda);
    uint32_t end = 0;
    for (uint32_t i = 1; i < 64; ++i) {
        if (!q[i]) continue;
        const int64_t e = trellis_end_cost(B[i], i, len, lambda);
        if (e <= best) { best = e; end = i; }
    }
    uint32_t lev[64] = {0};
    for (uint32_t i = end; i; ) { lev[i] = q[i] - choice[i]; i = pred[i][choice[i]]; }
    Searched r;
    std::memset(r.level, 0, sizeof r.level);
    r.level[0] = static_cast<int16_t>(trellis_plain(raw[0], Q[0]));
    for (int k = 1; k < 64; ++k) r.level[enc_zigzag(k)] = static_cast<int16_t>(raw[enc_zigzag(k)] < 0 ? -static_cast<int32_t>(lev[k]) : static_cast<int32_t>(lev[k]));
    r.cost = trellis_block_cost([&](uint32_t k) { return a[k]; }, [&](uint32_t k) { return Qz[k]; }, [&](uint32_t k) { return lev[k]; }, len, lambda);
    if (r.cost >= (1ll << 61)) ++g_guards[1];
    return r;
}

// jpeg_gen_optimal_table's lengths for counts + 1 on the legal symbols, the wave's 64 lanes as loops
void rate_table(const uint32_t* hist, uint8_t* len) {
    uint32_t counts[256], freq[257], codesize[257], bits[33], codes[256] = {0};
    int32_t others[257];
    uint8_t vals[256] = {0}, dht[kProgDhtPitch];
    for (uint32_t s = 0; s < 256; ++s) counts[s] = trellis_legal_ac(s) ? hist[s] + 1u : 0u;
    for (uint32_t lane = 0; lane < 64; ++lane) huff_init(counts, lane, freq, codesize, others);
    for (;;) {
        uint64_t k1 = ~0ull, k2 = ~0ull;
        for (uint32_t lane = 0; lane < 64; ++lane) k1 = std::min(k1, huff_lane_key(freq, lane, 0xFFFFFFFFu));
        const uint32_t c1 = huff_key_index(k1);
        for (uint32_t lane = 0; lane < 64; ++lane) k2 = std::min(k2, huff_lane_key(freq, lane, c1));
        if (k2 == ~0ull) break;
        huff_merge(c1, huff_key_index(k2), freq, codesize, others);
    }
    huff_limit(codesize, bits);
    for (uint32_t i = 0; i < 256; ++i) if (codesize[i] && codesize[i] <= 32u) vals[huff_rank(codesize, i)] = static_cast<uint8_t>(i);
    huff_emit(bits, vals, 0x10, dht, codes);
    for (uint32_t s = 0; s < 256; ++s) len[s] = static_cast<uint8_t>(codes[s] >> 16);
}

}  // namespace

extern "C" {

// A whole frame.  qt: [3][64] natural order.  raw* (nullable): the unquantised planes.  len_out (nullable): [2][256].
int jpeg_trellis_emulate(const uint8_t* bgra, uint32_t width, uint32_t height, uint32_t stride, const uint8_t* hs, const uint8_t* vs,
                         const uint16_t* qt, uint32_t lambda_scale, int16_t* coef0, int16_t* coef1, int16_t* coef2, int16_t* raw0, int16_t* raw1,
                         int16_t* raw2, uint8_t* len_out, int64_t* guards) {
    Geom g;
    if (!make_geom(width, height, hs, vs, &g)) return 1;
    g_guards[0] = g_guards[1] = 0;
    int16_t* coef[3] = {coef0, coef1, coef2};
    std::vector<int16_t> raw[3];
    for (int c = 0; c < 3; ++c) {
        raw[c].assign(static_cast<size_t>(g.bw[c]) * g.bh[c] * 64, 0);
        for (uint32_t by = 0; by < g.rbh[c]; ++by)
            for (uint32_t bx = 0; bx < g.rbw[c]; ++bx) {
                int32_t d[64];
                for (uint32_t y = 0; y < 8; ++y)
                    for (uint32_t x = 0; x < 8; ++x) d[y * 8 + x] = sample(bgra, stride, g, c, bx * 8 + x, by * 8 + y) - 128;
                fdct_islow(d);
                int16_t* o = raw[c].data() + (static_cast<size_t>(by) * g.bw[c] + bx) * 64;
                for (int k = 0; k < 64; ++k) o[k] = static_cast<int16_t>(d[k]);
            }
    }
    // plain pass: the symbol counts of the two table classes
    uint32_t hist[2][256] = {{0}};
    for (int c = 0; c < 3; ++c)
        for (uint32_t by = 0; by < g.rbh[c]; ++by)
            for (uint32_t bx = 0; bx < g.rbw[c]; ++bx) {
                const int16_t* x = raw[c].data() + (static_cast<size_t>(by) * g.bw[c] + bx) * 64;
                const uint16_t* Q = qt + c * 64;
                uint32_t* h = hist[c ? 1 : 0];
                trellis_count_ac([&](uint32_t k) { return trellis_plain(x[enc_zigzag(static_cast<int>(k))], Q[enc_zigzag(static_cast<int>(k))]); },
                                 [&](uint32_t s) { h[s]++; });
            }
    uint8_t len[2][256];
    rate_table(hist[0], len[0]);
    rate_table(hist[1], len[1]);
    for (int c = 0; c < 3; ++c) {
        std::memset(coef[c], 0, raw[c].size() * 2);
        for (uint32_t by = 0; by < g.rbh[c]; ++by)
            for (uint32_t bx = 0; bx < g.rbw[c]; ++bx) {
                const size_t at = (static_cast<size_t>(by) * g.bw[c] + bx) * 64;
                const Searched r = search_block(raw[c].data() + at, qt + c * 64, len[c ? 1 : 0], lambda_scale);
                std::memcpy(coef[c] + at, r.level, sizeof r.level);
            }
    }
    // jccoefct.c: the dummy blocks of the last MCU column / row repeat a DC value (luma only: chroma's MCU holds one block)
    for (uint32_t by = 0; by < g.bh[0]; ++by)
        for (uint32_t bx = 0; bx < g.bw[0]; ++bx) {
            if (bx < g.rbw[0] && by < g.rbh[0]) continue;
            uint32_t sy, sx;
            if (by < g.rbh[0]) { sy = by; sx = g.rbw[0] - 1; }
            else { sy = g.rbh[0] - 1; const uint32_t prev = (bx / g.hs[0]) * g.hs[0] + g.hs[0] - 1; sx = std::min(prev, g.rbw[0] - 1); }
            coef[0][(static_cast<size_t>(by) * g.bw[0] + bx) * 64] = coef[0][(static_cast<size_t>(sy) * g.bw[0] + sx) * 64];
        }
    int16_t* raws[3] = {raw0, raw1, raw2};
    for (int c = 0; c < 3; ++c) if (raws[c]) std::memcpy(raws[c], raw[c].data(), raw[c].size() * 2);
    if (len_out) std::memcpy(len_out, len, sizeof len);
    if (guards) { guards[0] = g_guards[0]; guards[1] = g_guards[1]; }
    return 0;
}

// One block (natural order) against a given rate table: the searched levels and their cost.
void jpeg_trellis_search_block(const int16_t* raw, const uint16_t* Q, const uint8_t* len, uint32_t lambda_scale, int16_t* level, int64_t* cost,
                               int64_t* guards) {
    g_guards[0] = g_guards[1] = 0;
    const Searched r = search_block(raw, Q, len, lambda_scale);
    std::memcpy(level, r.level, sizeof r.level);
    *cost = r.cost;
    if (guards) { guards[0] = g_guards[0]; guards[1] = g_guards[1]; }
}

// The stand-alone cost of given levels (natural order; their signs are ignored) for a block.
int64_t jpeg_trellis_block_cost(const int16_t* raw, const uint16_t* Q, const int16_t* level, const uint8_t* len, uint32_t lambda_scale) {
    uint64_t energy = 0;
    auto mag = [&](uint32_t k) { const int32_t x = raw[enc_zigzag(static_cast<int>(k))]; return static_cast<uint32_t>(x < 0 ? -x : x); };
    for (uint32_t k = 1; k < 64; ++k) energy += static_cast<uint64_t>(mag(k)) * mag(k);
    return trellis_block_cost(mag, [&](uint32_t k) { return static_cast<uint32_t>(Q[enc_zigzag(static_cast<int>(k))]); },
                              [&](uint32_t k) { const int32_t l = level[enc_zigzag(static_cast<int>(k))]; return static_cast<uint32_t>(l < 0 ? -l : l); }, len,
                              trellis_lambda(energy, lambda_scale));
}

// the rate table of given symbol counts
void jpeg_trellis_rate_table(const uint32_t* hist, uint8_t* len) { rate_table(hist, len); }

}  // extern "C"
