// jpeg_entropy_plan_check.cpp -- the host half of the baseline JPEG entropy stage (csrc/jpeg_entropy_tables.cpp,
// csrc/jpeg_entropy_plan.cpp) alone, with its own main, for the host sanitizers: files are prepared without pinned memory,
// batches planned, and their table block filled in a malloc'ed block of exactly table_bytes -- a write outside it is a finding.
// Every batch is held to the properties the kernels rely on; one line per batch goes to stdout for tests/test_jpeg_entropy_plan.py:
//   <batch> ok <fnv-1a digest of the seven regions> <seven offsets> <table_bytes> <n_words> <total_subs> <n_segs> <n_wg> <uniform> <ncomp> <longest segment>
//   <batch> refused <status> <message>
// Input (argv[1]): little-endian u32s -- files, then per file its length and bytes; batches, then per batch its length and file indices.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "jpeg_entropy_plan.hpp"

namespace ifhip {   // the two functions of api.cpp the host files call
static char g_msg[512];
int fail(int status, const char* fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(g_msg, sizeof g_msg, fmt, ap); va_end(ap); return status; }
const char* last_error() { return g_msg; }
}  // namespace ifhip
using namespace ifhip;

#define REQUIRE(cond, ...)                                                      \
    do {                                                                        \
        if (!(cond)) {                                                          \
            std::fprintf(stderr, "batch %zu: %s: ", batch_index, #cond);        \
            std::fprintf(stderr, __VA_ARGS__);                                  \
            std::fprintf(stderr, "\n");                                         \
            return false;                                                       \
        }                                                                       \
    } while (0)

namespace {

struct File {
    std::vector<uint8_t> bytes;
    std::unique_ptr<PreparedHost> host;
    std::unique_ptr<uint32_t, decltype(&std::free)> words{nullptr, &std::free};
    size_t n_words = 0;
};

struct Region { const char* name; size_t offset, bytes; };

uint64_t fnv1a(uint64_t h, const uint8_t* p, size_t n) {
    for (size_t i = 0; i < n; ++i) h = (h ^ p[i]) * 0x100000001b3ull;
    return h;
}

constexpr uint8_t kFill = 0xA5;                      // what the block holds before it is filled: the gaps keep it

bool check_batch(size_t batch_index, const std::vector<const File*>& files) {
    const uint32_t n = static_cast<uint32_t>(files.size());
    std::vector<const PreparedHost*> prep;
    for (const File* f : files) prep.push_back(f->host.get());
    BatchPlan plan;
    if (int rc = plan_batch(prep.data(), n, &plan)) {
        std::printf("%zu refused %d %s\n", batch_index, rc, last_error());
        return true;
    }
    // ---- sizes ----
    uint64_t subs = 0;
    size_t segs_wanted = 0;
    for (const PreparedHost* R : prep) { subs += R->seg.n_sub; segs_wanted += R->seg.nsub.size(); }
    REQUIRE(plan.total_subs == subs && plan.n_segs == segs_wanted, "%u sub-sequences, %zu segments", plan.total_subs, plan.n_segs);
    REQUIRE(plan.n_words == static_cast<size_t>(subs) * 32u + 64u, "n_words %zu", plan.n_words);
    REQUIRE(plan.n_wg == (subs + kOwnSubs - 1u) / kOwnSubs, "n_wg %u", plan.n_wg);
    const Region regions[7] = {{"segs", plan.o_segs, plan.n_segs * sizeof(Segment)},
                               {"sub_seg", plan.o_sub, static_cast<size_t>(subs) * sizeof(uint32_t)},
                               {"ftabs", plan.o_ftabs, n * sizeof(FastTabs)},
                               {"ptabs", plan.o_ptabs, n * sizeof(FastTabs)},
                               {"ctabs", plan.o_ctabs, n * sizeof(FastTabs)},
                               {"stabs", plan.o_stabs, static_cast<size_t>(n) * 6u * sizeof(SearchTab)},
                               {"wg_order", plan.o_order, plan.n_wg * sizeof(uint32_t)}};
    size_t end = 0;
    for (const Region& r : regions) {
        REQUIRE(r.offset % 256u == 0u, "%s at %zu", r.name, r.offset);
        REQUIRE(r.offset >= end, "%s at %zu begins inside the region before it (ends at %zu)", r.name, r.offset, end);
        end = r.offset + r.bytes;
    }
    REQUIRE(end <= plan.table_bytes, "the last region ends at %zu of %zu", end, plan.table_bytes);
    // ---- the block: exactly table_bytes ----
    std::unique_ptr<uint8_t, decltype(&std::free)> block(static_cast<uint8_t*>(std::malloc(plan.table_bytes)), &std::free);
    REQUIRE(block != nullptr, "malloc");
    std::memset(block.get(), kFill, plan.table_bytes);
    fill_batch_tables(prep.data(), n, plan, block.get());
    end = 0;
    for (size_t r = 0; r <= 7; ++r) {                // the gaps are never written
        const size_t gap_end = r < 7 ? regions[r].offset : plan.table_bytes;
        for (size_t i = end; i < gap_end; ++i) REQUIRE(block.get()[i] == kFill, "byte %zu between the regions was written", i);
        if (r < 7) end = regions[r].offset + regions[r].bytes;
    }
    const Segment* segs = reinterpret_cast<const Segment*>(block.get() + plan.o_segs);
    const uint32_t* sub_seg = reinterpret_cast<const uint32_t*>(block.get() + plan.o_sub);
    const uint32_t* wg_order = reinterpret_cast<const uint32_t*>(block.get() + plan.o_order);
    // ---- segments tile [0, total_subs) in image order ----
    uint64_t next_sub = 0;
    uint32_t longest = 0;
    size_t s = 0;
    for (uint32_t img = 0; img < n; ++img) {
        const PreparedHost& R = *prep[img];
        REQUIRE(plan.first_sub_of[img] == next_sub, "image %u starts at %u", img, plan.first_sub_of[img]);
        uint64_t blocks = 0;
        for (size_t k = 0; k < R.seg.nsub.size(); ++k, ++s) {
            const Segment& sg = segs[s];
            REQUIRE(sg.image == img, "segment %zu names image %u, not %u", s, sg.image, img);
            REQUIRE(sg.first_sub == next_sub && sg.n_sub >= 1u, "segment %zu: first_sub %u n_sub %u, %llu expected", s, sg.first_sub, sg.n_sub,
                    static_cast<unsigned long long>(next_sub));
            REQUIRE(static_cast<uint64_t>(sg.first_sub) * 1024u <= sg.bit_end && sg.bit_end <= (static_cast<uint64_t>(sg.first_sub) + sg.n_sub) * 1024u,
                    "segment %zu: bit_end %u outside its sub-sequences", s, sg.bit_end);
            REQUIRE(sg.first_mcu == R.seg.mcu0[k], "segment %zu: first_mcu %u", s, sg.first_mcu);
            for (uint32_t q = 0; q < sg.n_sub; ++q) REQUIRE(sub_seg[next_sub + q] == s, "sub_seg[%llu] = %u, segment %zu holds it",
                                                            static_cast<unsigned long long>(next_sub + q), sub_seg[next_sub + q], s);
            next_sub += sg.n_sub;
            blocks += sg.n_blocks;
            longest = sg.n_sub > longest ? sg.n_sub : longest;
        }
        REQUIRE(blocks == static_cast<uint64_t>(R.P.mcus_w) * R.P.mcus_h * R.P.blocks_per_mcu, "image %u: %llu blocks in its segments", img,
                static_cast<unsigned long long>(blocks));
    }
    REQUIRE(next_sub == subs && s == plan.n_segs, "the segments end at sub-sequence %llu", static_cast<unsigned long long>(next_sub));
    // ---- dispatch order: a permutation, stably sorted by the sub-sequence count of the image each block starts in ----
    std::vector<uint32_t> seen(plan.n_wg, 0u);
    auto key = [&](uint32_t w) { return prep[segs[sub_seg[static_cast<size_t>(w) * kOwnSubs]].image]->seg.n_sub; };
    for (uint32_t i = 0; i < plan.n_wg; ++i) {
        REQUIRE(wg_order[i] < plan.n_wg && !seen[wg_order[i]]++, "wg_order[%u] = %u", i, wg_order[i]);
        if (i) REQUIRE(key(wg_order[i - 1]) < key(wg_order[i]) || (key(wg_order[i - 1]) == key(wg_order[i]) && wg_order[i - 1] < wg_order[i]),
                       "wg_order[%u] = %u behind %u", i, wg_order[i], wg_order[i - 1]);
    }
    // ---- tables: what derive_* gives for each file alone ----
    bool uniform = true;
    auto F = std::make_unique<FastTabs>(), Pt = std::make_unique<FastTabs>(), Ct = std::make_unique<FastTabs>(), F0 = std::make_unique<FastTabs>();
    SearchTab S6[6], S0[6];
    for (uint32_t img = 0; img < n; ++img) {
        ParsedJpeg P;
        REQUIRE(parse_jpeg(files[img]->bytes.data(), files[img]->bytes.size(), &P) == 0, "image %u: %s", img, last_error());
        derive_image_tables(P, F.get(), S6, kPoolEntries);
        derive_pair_tables(*F, P.ncomp, Pt.get());
        derive_count_tables(*F, *Pt, Ct.get());
        const FastTabs* const alone[3] = {F.get(), Pt.get(), Ct.get()};
        for (size_t r = 0; r < 3; ++r)
            REQUIRE(std::memcmp(block.get() + regions[2 + r].offset + img * sizeof(FastTabs), alone[r], sizeof(FastTabs)) == 0, "image %u: %s", img, regions[2 + r].name);
        REQUIRE(std::memcmp(block.get() + plan.o_stabs + static_cast<size_t>(img) * sizeof S6, S6, sizeof S6) == 0, "image %u: stabs", img);
        if (img == 0) { *F0 = *F; std::memcpy(S0, S6, sizeof S0); }
        else if (std::memcmp(F0.get(), F.get(), sizeof(FastTabs)) != 0 || std::memcmp(S0, S6, sizeof S0) != 0) uniform = false;
    }
    REQUIRE(plan.uniform_tables == (uniform ? 1u : 0u), "uniform_tables %u", plan.uniform_tables);
    // ---- geometry ----
    const ParsedJpeg& P0 = prep[0]->P;
    REQUIRE(plan.g.ncomp == static_cast<uint32_t>(P0.ncomp) && plan.g.blocks_per_mcu == P0.blocks_per_mcu && plan.g.mcus_w == P0.mcus_w && plan.g.mcus_h == P0.mcus_h,
            "geometry of image 0");
    uint32_t k = 0;
    for (int c = 0; c < P0.ncomp; ++c)
        for (uint32_t b = 0; b < static_cast<uint32_t>(P0.hs[c]) * P0.vs[c]; ++b, ++k)
            REQUIRE(plan.g.kcomp[k] == c && ((plan.g.kcomp_packed >> (2u * k)) & 3u) == static_cast<uint32_t>(c) && plan.g.kdx[k] == b % P0.hs[c] && plan.g.kdy[k] == b / P0.hs[c],
                    "block %u of the MCU", k);
    REQUIRE(k == P0.blocks_per_mcu, "%u blocks in the MCU", k);

    uint64_t h = 0xcbf29ce484222325ull;
    for (const Region& r : regions) h = fnv1a(h, block.get() + r.offset, r.bytes);
    std::printf("%zu ok %016llx", batch_index, static_cast<unsigned long long>(h));
    for (const Region& r : regions) std::printf(" %zu", r.offset);
    std::printf(" %zu %zu %u %zu %u %u %u %u\n", plan.table_bytes, plan.n_words, plan.total_subs, plan.n_segs, plan.n_wg, plan.uniform_tables, plan.g.ncomp, longest);
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::vector<uint8_t> blob;
    {
        FILE* f = std::fopen(argv[1], "rb");
        if (!f) return 2;
        uint8_t buf[65536];
        for (size_t got; (got = std::fread(buf, 1, sizeof buf, f)) > 0;) blob.insert(blob.end(), buf, buf + got);
        std::fclose(f);
    }
    size_t at = 0;
    auto u32 = [&]() -> uint32_t {
        if (at + 4 > blob.size()) { std::fprintf(stderr, "short input\n"); std::exit(2); }
        uint32_t v;
        std::memcpy(&v, &blob[at], 4);
        at += 4;
        return v;
    };
    std::vector<File> files(u32());
    for (size_t i = 0; i < files.size(); ++i) {
        File& f = files[i];
        const uint32_t len = u32();
        if (at + len > blob.size()) return 2;
        f.bytes.assign(blob.begin() + at, blob.begin() + at + len);
        at += len;
        // prepared as ifhip_jpeg_entropy_prepare does it, the staging block from malloc and of exactly the bound
        f.host = std::make_unique<PreparedHost>();
        if (prepare_tables(f.host.get(), f.bytes.data(), f.bytes.size(), kPoolEntries)) { std::fprintf(stderr, "file %zu: %s\n", i, last_error()); return 1; }
        const size_t bound = packed_scan_bound(f.bytes.size(), f.host->P);
        f.words.reset(static_cast<uint32_t*>(std::malloc(bound)));
        if (!f.words) return 2;
        if (prepare_scan(f.host.get(), f.bytes.data(), f.bytes.size(), f.words.get(), bound, static_cast<uint32_t>(i), &f.n_words)) {
            std::fprintf(stderr, "file %zu: %s\n", i, last_error());
            return 1;
        }
        if (f.n_words != f.host->seg.n_sub * kSubWords || f.n_words * 4u > bound) { std::fprintf(stderr, "file %zu: %zu words\n", i, f.n_words); return 1; }
    }
    const uint32_t n_batches = u32();
    for (size_t b = 0; b < n_batches; ++b) {
        std::vector<const File*> batch(u32());
        for (const File*& f : batch) {
            const uint32_t i = u32();
            if (i >= files.size()) return 2;
            f = &files[i];
        }
        if (batch.empty() || !check_batch(b, batch)) return 1;
    }
    return 0;
}
