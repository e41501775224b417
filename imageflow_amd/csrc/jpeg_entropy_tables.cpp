// jpeg_entropy_tables.cpp -- the Huffman decode tables of one baseline JPEG file in the form the entropy kernels read
// (formats: jpeg_entropy_tables.hpp), and a batch's geometry.  Plain host code: no HIP.
#include "jpeg_entropy_tables.hpp"

#include <cstring>
#include <vector>

namespace ifhip {

void derive_search_table(const HuffSpec& h, SearchTab* t) {
    std::memset(t, 0, sizeof *t);
    std::memcpy(t->val, h.vals, 256);
    int32_t code = 0;
    int k = 0;
    for (int l = 1; l <= 16; ++l) {
        t->valoff[l] = k - code;
        k += h.bits[l];
        code += h.bits[l];
        // Largest code of this length.  A length without codes gets the previous bound extended by a 1 bit instead of
        // jdhuff's -1: the serial search "first l with code_l <= maxcode[l]" is unchanged (it only ever reaches l when
        // code_(l-1) > maxcode[l-1], and then code_l > (maxcode[l-1] << 1 | 1) as well), and "code_l > maxcode[l]" becomes
        // monotone in l, which lets the kernel count the lengths in parallel.
        t->maxcode[l] = h.bits[l] ? code - 1 : (l > 1 ? (t->maxcode[l - 1] < 0 ? -1 : ((t->maxcode[l - 1] << 1) | 1)) : -1);
        code <<= 1;
    }
    t->maxcode[17] = 0x7fffffff;
}
void derive_fast_table(const HuffSpec& h, bool ac, FastTabs* F, uint32_t slot, uint32_t* pool_used, uint32_t pool_limit) {
    uint32_t* lut = F->lut[slot];
    for (uint32_t i = 0; i < kLutEntries; ++i) lut[i] = invalid_entry(ac);
    // a DC symbol is a magnitude category, at most 11 in baseline JPEG: larger ones decode as "no such code"
    auto entry = [&](uint32_t l, uint32_t sym) { return (!ac && sym > 11u) ? invalid_entry(ac) : fast_entry(ac, l, sym); };
    struct LongCode { uint32_t code; uint8_t len, sym; };
    std::vector<LongCode> longs;
    uint8_t maxlen[kLutEntries] = {};
    uint32_t code = 0;
    int k = 0;
    for (uint32_t l = 1; l <= 16u; ++l) {
        for (int i = 0; i < h.bits[l]; ++i, ++k, ++code) {
            if (l <= kLutBits) {
                const uint32_t first = code << (kLutBits - l);
                for (uint32_t f = 0; f < (1u << (kLutBits - l)); ++f)
                    if (first + f < kLutEntries) lut[first + f] = entry(l, h.vals[k & 255]);
            } else {
                const uint32_t prefix = code >> (l - kLutBits);
                if (prefix >= kLutEntries) continue;                 // over-subscribed table: the pattern cannot occur
                maxlen[prefix] = static_cast<uint8_t>(l);            // lengths ascend
                longs.push_back(LongCode{code, static_cast<uint8_t>(l), h.vals[k & 255]});
            }
        }
        code <<= 1;
    }
    for (uint32_t prefix = 0; prefix < kLutEntries; ++prefix) {
        if (!maxlen[prefix]) continue;
        const uint32_t n = maxlen[prefix] - kLutBits, size = 1u << n;
        if (*pool_used + size > pool_limit) { lut[prefix] = 0u; continue; }          // left to the serial search
        for (uint32_t i = 0; i < size; ++i) F->pool[*pool_used + i] = invalid_entry(ac);
        lut[prefix] = (*pool_used << 16) | ((32u - n) << 8);
        *pool_used += size;
    }
    for (const LongCode& lc : longs) {
        const uint32_t prefix = lc.code >> (lc.len - kLutBits);
        if (lut[prefix] == 0u) continue;
        const uint32_t n = maxlen[prefix] - kLutBits, rem = lc.len - kLutBits, off = lut[prefix] >> 16;
        const uint32_t sub = (lc.code & ((1u << rem) - 1u)) << (n - rem);
        for (uint32_t f = 0; f < (1u << (n - rem)); ++f) F->pool[off + sub + f] = entry(lc.len, lc.sym);
    }
}
void derive_pair_tables(const FastTabs& F, int ncomp, FastTabs* Pt) {
    for (uint32_t i = 0; i < kPoolEntries; ++i) Pt->pool[i] = pair_entry(F.pool[i], F.pool[i]);
    for (uint32_t slot = 0; slot < 6u; ++slot)
        for (uint32_t i = 0; i < kLutEntries; ++i) {
            const uint32_t e = F.lut[slot][i];
            uint32_t out = (e & 255u) ? pair_entry(e, e) : e;                        // skip 0: pointer into the pool / serial search
            const uint32_t skip1 = e & 255u, adv1 = (e >> 8) & 255u;
            if ((slot & 1u) && slot < 2u * static_cast<uint32_t>(ncomp) && skip1 != 0u && skip1 < kLutBits && adv1 < 64u) {
                const uint32_t e2 = F.lut[slot][(i << skip1) & (kLutEntries - 1u)];   // the window behind the first symbol
                const uint32_t len2 = (e2 >> 16) & 255u;
                if ((e2 & 255u) != 0u && len2 <= kLutBits - skip1)                   // a whole code (never the 32 of "no such code")
                    out = pair_entry(e, (skip1 + (e2 & 255u)) | ((adv1 + ((e2 >> 8) & 255u)) << 8));
            }
            Pt->lut[slot][i] = out;
        }
}
void derive_count_tables(const FastTabs& F, const FastTabs& Pt, FastTabs* Ct) {
    *Ct = Pt;
    for (uint32_t slot = 0; slot < 6u; slot += 2u)
        for (uint32_t i = 0; i < kLutEntries; ++i) {
            const uint32_t e = F.lut[slot][i];
            Ct->lut[slot][i] = e;
            if ((e & 255u) == 0u && e != 0u) {
                const uint32_t off = e >> 16, size = 1u << (32u - ((e >> 8) & 255u));
                for (uint32_t k = 0; k < size && off + k < kPoolEntries; ++k) Ct->pool[off + k] = F.pool[off + k];
            }
        }
}
void derive_image_tables(const ParsedJpeg& P, FastTabs* F, SearchTab* S6, uint32_t pool_limit, uint32_t* pool_used_out) {
    std::memset(F, 0, sizeof *F);
    std::memset(S6, 0, 6u * sizeof *S6);
    uint32_t pool_used = 0;
    for (int c = 0; c < P.ncomp; ++c)
        for (uint32_t ac = 0; ac < 2u; ++ac) {
            const uint32_t slot = 2u * static_cast<uint32_t>(c) + ac;
            const uint8_t id = ac ? P.ta[c] : P.td[c];
            derive_search_table(ac ? P.ac[id] : P.dc[id], &S6[slot]);
            int same = -1;
            for (int o = 0; o < c; ++o) if ((ac ? P.ta[o] : P.td[o]) == id) same = o;
            if (same >= 0) std::memcpy(F->lut[slot], F->lut[2u * static_cast<uint32_t>(same) + ac], sizeof F->lut[slot]);
            else derive_fast_table(ac ? P.ac[id] : P.dc[id], ac != 0u, F, slot, &pool_used, pool_limit);
        }
    if (pool_used_out) *pool_used_out = pool_used;
}

EntropyGeom entropy_geom(const ParsedJpeg& P) {
    EntropyGeom g;
    std::memset(&g, 0, sizeof g);
    g.ncomp = static_cast<uint32_t>(P.ncomp); g.blocks_per_mcu = P.blocks_per_mcu; g.mcus_w = P.mcus_w; g.mcus_h = P.mcus_h;
    uint32_t k = 0;
    for (int c = 0; c < P.ncomp; ++c) {
        g.bw[c] = P.bw[c]; g.bh[c] = P.bh[c]; g.hs[c] = P.hs[c]; g.vs[c] = P.vs[c];
        for (uint32_t dy = 0; dy < P.vs[c]; ++dy)
            for (uint32_t dx = 0; dx < P.hs[c]; ++dx, ++k) {
                g.kcomp[k] = static_cast<uint8_t>(c); g.kdx[k] = static_cast<uint8_t>(dx); g.kdy[k] = static_cast<uint8_t>(dy);
                g.kcomp_packed |= static_cast<uint32_t>(c) << (2u * k);
            }
    }
    return g;
}

}  // namespace ifhip
