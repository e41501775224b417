// stage_scratch_check.cpp -- csrc/stage_scratch.hpp without a device: a program of its own (built with g++ and
// -fsanitize=address,undefined by tests/test_stage_scratch.py), which supplies the few ifhip:: functions the header calls
// -- an allocator over malloc that fails on the k-th call and counts what is live -- and walks a stage of N blocks through
// every place an allocation can fail.  Prints one line per finding; exit status 0: none.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>

#include "../imageflow_amd/csrc/stage_scratch.hpp"

namespace {
std::set<void*> g_live;
int g_calls = 0, g_fail_at = 0, g_frees = 0, g_device = 0, g_findings = 0;
char g_message[256];
}  // namespace

namespace ifhip {
int fail(int status, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(g_message, sizeof g_message, fmt, ap);
    va_end(ap);
    return status;
}
int cached_malloc(void** out, size_t bytes) {
    *out = nullptr;
    if (++g_calls == g_fail_at) return 2;                        // (hipErrorOutOfMemory)
    *out = std::malloc(bytes);
    g_live.insert(*out);
    return 0;
}
int cached_free(void* p) {
    if (!p) return 0;
    if (!g_live.erase(p)) { std::printf("a block is freed that is not live\n"); ++g_findings; return 1; }
    std::free(p);
    ++g_frees;
    return 0;
}
int require_gfx950(int* device_out) {
    if (device_out) *device_out = g_device;
    return IFHIP_OK;
}
}  // namespace ifhip

using namespace ifhip;

namespace {
constexpr int N = 5;

// a stage the way the coders write theirs: typed pointers, the owner behind them, one checked allocation per block
struct Stage {
    uint8_t* a = nullptr;
    uint32_t *b = nullptr, *c = nullptr;
    uint64_t* d = nullptr;
    void* e = nullptr;
    StageScratch blocks{&a, &b, &c, &d, &e};
    int allocate() {
        return blocks.ensure([&]() -> int {
            size_t bytes = 16;
            for (void** p : {reinterpret_cast<void**>(&a), reinterpret_cast<void**>(&b), reinterpret_cast<void**>(&c), reinterpret_cast<void**>(&d), &e}) {
                if (cached_malloc(p, bytes)) return fail(IFHIP_GPU_ERROR, "GpuError: DEV_MALLOC(%d bytes) failed", static_cast<int>(bytes));
                bytes *= 3;
            }
            return IFHIP_OK;
        });
    }
    bool empty() const { return !a && !b && !c && !d && !e && !blocks.allocated(); }
    bool full() const { return a && b && c && d && e && blocks.allocated(); }
};

void expect(bool ok, int k, const char* what) {
    if (ok) return;
    std::printf("k = %d: %s\n", k, what);
    ++g_findings;
}
}  // namespace

int main() {
    for (int k = 1; k <= N; ++k) {
        g_device = 0; g_frees = 0;
        {
            Stage s;
            g_calls = 0; g_fail_at = k;
            expect(s.allocate() == IFHIP_GPU_ERROR, k, "the failed allocation is not reported as a GpuError");
            expect(g_live.empty(), k, "a failed call leaves blocks behind");
            expect(g_frees == k - 1, k, "a failed call frees something other than what it took");
            expect(s.empty(), k, "the stage is not as it was before the failed call");
            g_calls = 0; g_fail_at = 0;
            expect(s.allocate() == IFHIP_OK && g_calls == N && g_live.size() == N && s.full(), k, "the retry does not take exactly N blocks");
            expect(s.allocate() == IFHIP_OK && g_calls == N, k, "a call on an allocated stage allocates");
            g_device = 1; g_message[0] = 0;
            expect(s.allocate() == IFHIP_INVALID_STATE && g_calls == N && s.full(), k, "a call on another device is not an InvalidState that leaves the stage alone");
            expect(std::string(g_message) == "InvalidState: stage belongs to device 0, current device is 1", k, g_message);
            expect(s.blocks.check_device() == IFHIP_INVALID_STATE, k, "check_device passes on another device");
            g_device = 0;
            expect(s.blocks.check_device() == IFHIP_OK, k, "check_device fails on the stage's device");
            g_frees = 0;
        }
        expect(g_frees == N && g_live.empty(), k, "destruction does not free N blocks");
    }
    {   // a stage that never allocated frees nothing
        g_frees = 0;
        { Stage s; expect(s.blocks.check_device() == IFHIP_OK && s.empty(), 0, "a fresh stage is not empty"); }
        expect(g_frees == 0, 0, "a fresh stage frees blocks");
    }
    std::printf("%d findings\n", g_findings);
    return g_findings ? 1 : 0;
}
