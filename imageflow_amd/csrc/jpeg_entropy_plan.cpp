// jpeg_entropy_plan.cpp -- see jpeg_entropy_plan.hpp.  Plain host code: no HIP.
#include "jpeg_entropy_plan.hpp"

#include <algorithm>
#include <cstring>

namespace ifhip {

int prepare_tables(PreparedHost* R, const uint8_t* file, size_t len, uint32_t pool_limit) {
    ParsedJpeg& P = R->P;
    P = ParsedJpeg();
    if (int rc = parse_jpeg(file, len, &P)) return rc;
    jpeg::report_quant_tables(P, P, R->qt);
    std::memset(&R->ftabs, 0, sizeof R->ftabs); std::memset(&R->ptabs, 0, sizeof R->ptabs); std::memset(&R->ctabs, 0, sizeof R->ctabs);   // (a recycled handle)
    std::memset(R->stabs, 0, sizeof R->stabs);
    R->pool_limit = pool_limit;
    derive_image_tables(P, &R->ftabs, R->stabs, R->pool_limit);
    derive_pair_tables(R->ftabs, P.ncomp, &R->ptabs);
    derive_count_tables(R->ftabs, R->ptabs, &R->ctabs);
    return IFHIP_OK;
}

int prepare_scan(PreparedHost* R, const uint8_t* file, size_t len, uint32_t* dst, size_t cap, uint32_t index_for_messages, size_t* n_words) {
    const ParsedJpeg& P = R->P;
    const uint32_t total_mcus = P.mcus_w * P.mcus_h;
    const uint32_t mcu0 = unstuff_scan_packed(file, len, P, reinterpret_cast<uint8_t*>(dst), cap, &R->seg);
    const uint64_t subs = R->seg.n_sub;
    if (subs * kSubBits + 4096 >= (1ull << 32)) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: more than 512 MB of scan data");
    if (mcu0 < total_mcus)
        return fail(IFHIP_INVALID_ARGUMENT, "ImageMalformed: scan of image %u ends after %u of %u MCUs", index_for_messages, mcu0, total_mcus);
    *n_words = static_cast<size_t>(subs) * kSubWords;
    for (size_t q = 0; q < *n_words; ++q) dst[q] = __builtin_bswap32(dst[q]);   // stream order bytes -> big-endian words
    return IFHIP_OK;
}

int plan_batch(const PreparedHost* const* prep, uint32_t n_images, BatchPlan* out) {
    BatchPlan& b = *out;
    b = BatchPlan();
    uint64_t subs_in_batch = 0;
    for (uint32_t img = 0; img < n_images; ++img) { b.n_segs += prep[img]->seg.nsub.size(); subs_in_batch += prep[img]->seg.n_sub; }
    if (subs_in_batch * kSubBits + 4096 >= (1ull << 32)) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: batch holds more than 512 MB of scan data");
    const ParsedJpeg& F = prep[0]->P;
    for (uint32_t img = 1; img < n_images; ++img) {
        const ParsedJpeg& P = prep[img]->P;
        bool same = P.width == F.width && P.height == F.height && P.ncomp == F.ncomp;
        for (int c = 0; c < P.ncomp && same; ++c) same = P.hs[c] == F.hs[c] && P.vs[c] == F.vs[c];
        if (!same) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: image %u differs in size or sampling from image 0 (one batch = one geometry)", img);
    }
    b.total_subs = static_cast<uint32_t>(subs_in_batch);
    b.n_wg = static_cast<uint32_t>((subs_in_batch + kOwnSubs - 1u) / kOwnSubs);
    auto aligned = [](size_t v) { return (v + 255u) & ~static_cast<size_t>(255u); };
    b.o_segs = 0;
    b.o_sub = aligned(b.o_segs + std::max<size_t>(b.n_segs, 1) * sizeof(Segment));
    b.o_ftabs = aligned(b.o_sub + std::max<size_t>(subs_in_batch, 1) * sizeof(uint32_t));
    b.o_ptabs = aligned(b.o_ftabs + n_images * sizeof(FastTabs));
    b.o_ctabs = aligned(b.o_ptabs + n_images * sizeof(FastTabs));
    b.o_stabs = aligned(b.o_ctabs + n_images * sizeof(FastTabs));
    b.o_order = aligned(b.o_stabs + static_cast<size_t>(n_images) * 6u * sizeof(SearchTab));
    b.table_bytes = aligned(b.o_order + (static_cast<size_t>(b.n_wg) + 1u) * sizeof(uint32_t));
    b.n_words = static_cast<size_t>(subs_in_batch) * kSubWords + 64u;
    b.first_sub_of.resize(n_images);
    uint32_t first = 0;
    for (uint32_t img = 0; img < n_images; ++img) { b.first_sub_of[img] = first; first += static_cast<uint32_t>(prep[img]->seg.n_sub); }
    b.g = entropy_geom(F);
    b.uniform_tables = 1u;                           // batches of small files put many images into one workgroup: with
    for (uint32_t img = 1; img < n_images && b.uniform_tables; ++img)     // identical tables they all use the LDS copy
        if (std::memcmp(&prep[img]->ftabs, &prep[0]->ftabs, sizeof(FastTabs)) != 0 ||
            std::memcmp(prep[img]->stabs, prep[0]->stabs, 6u * sizeof(SearchTab)) != 0) b.uniform_tables = 0u;
    return IFHIP_OK;
}

void fill_batch_tables(const PreparedHost* const* prep, uint32_t n_images, const BatchPlan& plan, uint8_t* block) {
    Segment* const segs = reinterpret_cast<Segment*>(block + plan.o_segs);
    uint32_t* const sub_seg = reinterpret_cast<uint32_t*>(block + plan.o_sub);
    FastTabs* const ftabs = reinterpret_cast<FastTabs*>(block + plan.o_ftabs);
    FastTabs* const ptabs = reinterpret_cast<FastTabs*>(block + plan.o_ptabs);
    FastTabs* const ctabs = reinterpret_cast<FastTabs*>(block + plan.o_ctabs);
    SearchTab* const stabs = reinterpret_cast<SearchTab*>(block + plan.o_stabs);
    uint32_t* const wg_order = reinterpret_cast<uint32_t*>(block + plan.o_order);
    size_t seg_count = 0;
    for (uint32_t img = 0; img < n_images; ++img) {
        const PreparedHost& R = *prep[img];
        std::memcpy(&ftabs[img], &R.ftabs, sizeof(FastTabs)); std::memcpy(&ptabs[img], &R.ptabs, sizeof(FastTabs)); std::memcpy(&ctabs[img], &R.ctabs, sizeof(FastTabs));
        std::memcpy(&stabs[static_cast<size_t>(img) * 6u], R.stabs, sizeof R.stabs);
        uint64_t sub = plan.first_sub_of[img];
        for (size_t k = 0; k < R.seg.nsub.size(); ++k) {
            Segment sg;
            std::memset(&sg, 0, sizeof sg);
            sg.image = img;
            sg.first_mcu = R.seg.mcu0[k];
            sg.n_blocks = R.seg.mcus[k] * R.P.blocks_per_mcu;
            sg.first_sub = static_cast<uint32_t>(sub);
            sg.n_sub = R.seg.nsub[k];
            sg.bit_end = static_cast<uint32_t>(sub * kSubBits + R.seg.bits[k]);
            for (uint32_t q = 0; q < sg.n_sub; ++q) sub_seg[sub + q] = static_cast<uint32_t>(seg_count);
            sub += sg.n_sub;
            segs[seg_count++] = sg;
        }
    }
    // dispatch order of the synchronisation launch (see entropy_round_kernel): blocks of the smallest scans first, an image's
    // blocks in their own order
    std::vector<uint32_t> key(plan.n_wg);
    uint32_t img = 0;
    for (uint32_t w = 0; w < plan.n_wg; ++w) {
        const uint64_t s0 = static_cast<uint64_t>(w) * kOwnSubs;
        while (img + 1u < n_images && plan.first_sub_of[img + 1u] <= s0) ++img;
        key[w] = static_cast<uint32_t>(prep[img]->seg.n_sub);
        wg_order[w] = w;
    }
    std::stable_sort(wg_order, wg_order + plan.n_wg, [&](uint32_t x, uint32_t y) { return key[x] < key[y]; });
}

}  // namespace ifhip
