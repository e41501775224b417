// jpeg_scan_report.cpp -- diagnostic (host only, no GPU): the tables and the scan layout of one file, checked against each other.
// Everything the kernels of jpeg_entropy.hip rely on that can be checked without them: the two-level tables decode the scan to
// exactly the blocks the geometry asks for (and to the DC values returned in dc_last: the caller compares them with a serial
// decoder's), and a walk with the pair tables / the count tables passes through the same state at every sub-sequence boundary
// as the plain walk -- the property that lets the synchronisation rounds, the count pass and the write pass hand states to
// each other.  A host mirror of walk (same entry formats, same rules, the kernels' long_entry); nothing here produces coefficients.
#include <cstring>
#include <memory>
#include <vector>

#include "jpeg_entropy_tables.hpp"

using namespace ifhip;

namespace {
struct HostStream {
    const std::vector<uint8_t>& b;
    uint32_t peek(uint64_t p) const {                                // 32 bits behind bit position p, zero behind the end
        uint64_t v = 0;
        const size_t at = static_cast<size_t>(p >> 3);
        for (size_t i = 0; i < 5; ++i) v = (v << 8) | (at + i < b.size() ? b[at + i] : 0u);
        return static_cast<uint32_t>((v << (p & 7u)) >> 8);
    }
};
struct HostState { uint64_t p; uint32_t c, z; };
struct HostCounts { uint64_t reads = 0, blocks = 0; int32_t dc[3] = {0, 0, 0}; bool bad = false; };
// mirror of walk(): from state s to the first symbol boundary at or behind `end` (or until `max_blocks` blocks started)
template <int kPairs>
HostState host_walk(const EntropyGeom& g, const HostStream& in, const FastTabs& T, const SearchTab* S6, HostState s, uint64_t end,
                    uint64_t max_blocks, HostCounts* n) {
    while (s.p < end) {
        const uint32_t comp = (g.kcomp_packed >> (2u * s.c)) & 3u, slot = comp * 2u + (s.z ? 1u : 0u);
        if (s.z == 0u && n->blocks >= max_blocks) break;             // pad bits behind the last block
        const uint32_t bits = in.peek(s.p);
        uint32_t e = T.lut[slot][bits >> (32u - kLutBits)];
        if ((e & 255u) == 0u) e = long_entry<kPairs>(&T, S6, slot, e, bits);
        ++n->reads;
        if (s.z == 0u) {
            ++n->blocks;
            if (kPairs != 1) {                                       // DC entries are plain in the plain and the count tables
                const uint32_t len = (e >> 16) & 255u, sz = (e >> 24) & 15u;
                if (len > 16u) n->bad = true;
                else if (sz) {
                    const uint32_t v = (bits << len) >> (32u - sz);
                    n->dc[comp] += static_cast<int32_t>(v) - ((v >> (sz - 1u)) ? 0 : static_cast<int32_t>((1u << sz) - 1u));
                }
            }
        }
        bool both = false;
        if (kPairs == 1 || (kPairs == 2 && s.z != 0u)) both = s.z + ((e >> 8) & 255u) < 64u && s.p + (e & 255u) < end;
        if (kPairs == 0 && ((e >> 21) & 1u)) n->bad = true;
        if (both) e >>= 16;
        s.p += e & 255u;
        s.z += (e >> 8) & 255u;
        if (s.z >= 64u) { s.z = 0u; s.c = s.c + 1u == g.blocks_per_mcu ? 0u : s.c + 1u; }
    }
    return s;
}
}  // namespace

extern "C" int ifhip_jpeg_debug_scan_report(const uint8_t* jpeg, size_t len, ifhip_jpeg_scan_report* out) {
    if (!jpeg || !out) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: null pointer");
    return c_entry("", [&]() -> int {
        std::memset(out, 0, sizeof *out);
        ParsedJpeg P;
        if (int rc = parse_jpeg(jpeg, len, &P)) return rc;
        auto F = std::make_unique<FastTabs>(), Pt = std::make_unique<FastTabs>(), Ct = std::make_unique<FastTabs>();
        SearchTab S6[6];
        const uint32_t pool_limit = test_hook_u32("ent_test_pool", kPoolEntries, kPoolEntries);
        derive_image_tables(P, F.get(), S6, pool_limit, &out->pool_entries_used);
        derive_pair_tables(*F, P.ncomp, Pt.get());
        derive_count_tables(*F, *Pt, Ct.get());
        out->pool_entries = kPoolEntries;
        for (uint32_t slot = 0; slot < 2u * static_cast<uint32_t>(P.ncomp); ++slot)
            for (uint32_t i = 0; i < kLutEntries; ++i) {
                if (F->lut[slot][i] == 0u) ++out->prefixes_left_to_search;
                if ((slot & 1u) && (Pt->lut[slot][i] >> 16) != (Pt->lut[slot][i] & 0xffffu)) ++out->pair_entries;
            }
        const EntropyGeom g = entropy_geom(P);
        std::vector<std::vector<uint8_t>> seg_bytes;
        ScanSegments seg, packed_seg;
        const uint32_t covered = unstuff_scan(jpeg, len, P, &seg_bytes, &seg);
        {   // the product's un-stuffer (straight into the staging block) against the walk above: same segments, same bytes, and
            // -- under the sanitizer build, tools/sanitize -- never a byte beyond the bound the staging block is sized by
            const size_t bound = packed_scan_bound(len, P);
            std::unique_ptr<uint8_t[]> packed(new uint8_t[bound]);
            const uint32_t p_covered = unstuff_scan_packed(jpeg, len, P, packed.get(), bound, &packed_seg);
            bool same = p_covered == covered && packed_seg.mcu0 == seg.mcu0 && packed_seg.mcus == seg.mcus && packed_seg.bits.size() == seg_bytes.size();
            for (size_t k = 0; same && k < seg_bytes.size(); ++k)
                same = packed_seg.bits[k] == seg_bytes[k].size() * 8u &&
                       std::memcmp(packed.get() + static_cast<size_t>(packed_seg.first_word[k]) * 4u, seg_bytes[k].data(), seg_bytes[k].size()) == 0;
            if (!same) return fail(IFHIP_INVALID_STATE, "InvalidState: the packed un-stuffer disagrees with the per-segment walk");
        }
        out->segments = static_cast<uint32_t>(seg_bytes.size());
        out->scan_complete = covered == P.mcus_w * P.mcus_h ? 1u : 0u;
        for (size_t sgi = 0; sgi < seg_bytes.size(); ++sgi) {
            const HostStream in{seg_bytes[sgi]};
            const uint64_t bit_end = static_cast<uint64_t>(seg_bytes[sgi].size()) * 8u, want = static_cast<uint64_t>(seg.mcus[sgi]) * P.blocks_per_mcu;
            const uint64_t n_sub = std::max<uint64_t>(1u, (bit_end + kSubBits - 1u) / kSubBits);
            out->sub_sequences += static_cast<uint32_t>(n_sub);
            HostCounts plain, paired, counted;
            HostState s{0u, 0u, 0u};
            for (uint64_t t = 0; t < n_sub; ++t) {                   // every sub-sequence from its true entry state, three ways
                const uint64_t end = std::min<uint64_t>((t + 1u) * kSubBits, bit_end);
                const HostState a0 = host_walk<0>(g, in, *F, S6, s, end, want, &plain);
                const HostState a1 = host_walk<1>(g, in, *Pt, S6, s, end, want, &paired);
                const HostState a2 = host_walk<2>(g, in, *Ct, S6, s, end, want, &counted);
                if (a1.p != a0.p || a1.c != a0.c || a1.z != a0.z) ++out->pair_walk_mismatches;
                if (a2.p != a0.p || a2.c != a0.c || a2.z != a0.z) ++out->count_walk_mismatches;
                s = a0;
            }
            out->symbols += plain.reads;
            out->table_reads_with_pairs += paired.reads;
            out->blocks += plain.blocks;
            if (plain.blocks != want) ++out->segments_with_wrong_block_count;
            if (plain.bad) ++out->segments_with_invalid_codes;
            for (int c = 0; c < 3; ++c) {
                if (counted.dc[c] != plain.dc[c]) ++out->count_walk_mismatches;
                out->dc_sum[c] += plain.dc[c];                       // (per segment the predictor restarts at 0: sums of the last segment
                if (sgi + 1 == seg_bytes.size()) out->dc_last_segment[c] = plain.dc[c];        // give the last block's DC value)
            }
        }
        return IFHIP_OK;
    });
}
