// color_link_prefix_sweep.cpp -- a stand-alone program over csrc/color_link.cpp for tests/test_color_link_plan.py, built with
// g++ -fsanitize=address,undefined: every prefix of each profile named on the command line, and seeded single-byte changes of
// it (argv[1]: how many per profile), go through color_link_from_icc -- as a colour frame's and as a grey frame's profile -- in
// a heap block of exactly its length, so that a read past the profile is a sanitizer report.  Prints the number of calls per
// status.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <memory>
#include <vector>

#include "../imageflow_amd/csrc/color_link.hpp"

namespace {
unsigned long g_seen[3] = {0, 0, 0};
void run(const uint8_t* p, size_t n, bool gray) {
    std::unique_ptr<uint8_t[]> exact(new uint8_t[n ? n : 1]);          // no slack behind the last byte
    if (n) std::memcpy(exact.get(), p, n);
    ifhip::ColorLink link;
    const ifhip::ColorPlanResult r = ifhip::color_link_from_icc(exact.get(), n, gray, &link);
    if (r.status < 0 || r.status > 2 || !r.reason) { std::printf("bad status %d\n", r.status); std::exit(2); }
    if (r.status == 0 && link.kind != ifhip::kColorLinkGray && link.nodes.size() != 33u * 33u * 33u) { std::printf("a planned link without its nodes\n"); std::exit(2); }
    ++g_seen[r.status];
}
}  // namespace

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    const int changes = std::atoi(argv[1]);
    uint32_t seed = 12345u;
    const auto next = [&seed]() { seed = seed * 1664525u + 1013904223u; return seed >> 8; };
    for (int a = 2; a < argc; ++a) {
        std::ifstream f(argv[a], std::ios::binary);
        std::vector<uint8_t> icc((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        if (icc.empty()) { std::printf("cannot read %s\n", argv[a]); return 2; }
        const bool gray = icc.size() >= 20 && std::memcmp(&icc[16], "GRAY", 4) == 0;
        for (size_t n = 0; n <= icc.size(); ++n) run(icc.data(), n, gray);
        run(icc.data(), icc.size(), !gray);
        for (int k = 0; k < changes; ++k) {
            std::vector<uint8_t> m = icc;
            // half of the changes in the header, the tag table and the element's own header (the first 256 bytes), half anywhere
            const size_t at = (k & 1) ? next() % m.size() : next() % (m.size() < 256 ? m.size() : 256);
            static const uint8_t hostile[] = {0x00, 0x01, 0x02, 0x7F, 0x80, 0xFF};
            m[at] = hostile[next() % 6u];
            run(m.data(), m.size(), gray);
        }
    }
    std::printf("planned %lu not_convertible %lu malformed %lu\n", g_seen[0], g_seen[1], g_seen[2]);
    return 0;
}
