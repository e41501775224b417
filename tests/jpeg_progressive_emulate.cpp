// jpeg_progressive_emulate.cpp -- csrc/jpeg_progressive_read.cpp and csrc/jpeg_progressive_core.hpp on the CPU: the front end
// as the library runs it, the batch's block laid out by prog_layout_batch with exactly the sizes the device entry allocates,
// and the clear and the launch of every level as loops over workgroups of one 64-lane wave, the workgroup's scratch pre-filled
// with 0xA5 -- an access outside the block, a plane or the scratch is a finding of the sanitizer build.
// Built by tests/test_jpeg_progressive_core.py with g++ (and, with its own main, with ASan + UBSan).
#include <cstdarg>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../imageflow_amd/csrc/jpeg_progressive_read.cpp"

namespace ifhip {
int fail(int status, const char*, ...) { return status; }
}  // namespace ifhip

using namespace ifhip;

extern "C" {

// info: width, height, ncomp, bw[3], bh[3], scans, streams, levels, bits of the longest stream, kProgStageWords
int prog_emu_prepare(const uint8_t* file, size_t len, uint32_t* info, uint16_t* qt3x64) {
    ProgPrepared P;
    if (int rc = prog_prepare(file, len, &P)) return rc;
    info[0] = P.width; info[1] = P.height; info[2] = P.ncomp;
    for (int c = 0; c < 3; ++c) { info[3 + c] = P.bw[c]; info[6 + c] = P.bh[c]; }
    info[9] = static_cast<uint32_t>(P.scans.size()); info[10] = static_cast<uint32_t>(P.streams.size()); info[11] = P.n_levels;
    info[12] = 0;
    for (const ProgStreamRec& st : P.streams) if (st.n_bits > info[12]) info[12] = st.n_bits;
    info[13] = kProgStageWords;
    if (qt3x64) for (uint32_t c = 0; c < P.ncomp; ++c) std::memcpy(qt3x64 + 64 * c, P.qt[c], 128);
    return 0;
}

// n files into their planes (coef[3 * i + c] of plane_bytes[3 * i + c]); rc[i] is prepare's answer, status[i] the status word
// of a file that was prepared.  The prepared files go through ONE batch, as the device entry runs them.
int prog_emu_decode_batch(const uint8_t* const* files, const size_t* lens, uint32_t n, void* const* coef, const size_t* plane_bytes, int* rc, uint32_t* status) {
    std::vector<ProgPrepared> P(n);
    std::vector<const ProgPrepared*> ok;
    std::vector<void*> planes;
    std::vector<size_t> bytes;
    std::vector<uint32_t> at;
    for (uint32_t i = 0; i < n; ++i) {
        rc[i] = prog_prepare(files[i], lens[i], &P[i]);
        if (rc[i]) continue;
        ok.push_back(&P[i]);
        at.push_back(i);
        for (int c = 0; c < 3; ++c) { planes.push_back(coef[3 * i + c]); bytes.push_back(plane_bytes[3 * i + c]); }
    }
    if (ok.empty()) return 0;
    ProgLayout L;
    if (!prog_layout_batch(ok.data(), static_cast<uint32_t>(ok.size()), planes.data(), bytes.data(), &L)) return -1;
    uint8_t* block = static_cast<uint8_t*>(std::malloc(L.blob.size()));      // exactly the device block: nothing behind the blob
    std::memcpy(block, L.blob.data(), L.blob.size());
    std::vector<uint32_t> words(ok.size(), 0xA5A5A5A5u);
    const ProgArgs a = L.args(block, words.data());
    jpeg_progressive_decode_batch_cpu(a, L.level_first.data(), static_cast<uint32_t>(L.level_first.size()) - 1u, 3u);
    std::free(block);
    for (size_t k = 0; k < ok.size(); ++k) status[at[k]] = words[k];
    return 0;
}

}  // extern "C"

#ifdef JPEG_PROG_EMU_MAIN
// The sanitizer build: cases from a file (u32 len, bytes), a line "rc status sum" per case; the planes are sized exactly.
#include <cstdio>
int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t head;
    while (std::fread(&head, 4, 1, f) == 1) {
        std::vector<uint8_t> src(head ? head : 1);
        if (head && std::fread(src.data(), 1, head, f) != head) return 3;
        uint32_t info[14] = {0};
        int rc = prog_emu_prepare(src.data(), head, info, nullptr);
        uint32_t status = 0, sum = 0;
        if (!rc) {
            std::vector<int16_t> plane[3];
            void* coef[3];
            size_t bytes[3];
            for (int c = 0; c < 3; ++c) {
                plane[c].assign(static_cast<size_t>(info[3 + c]) * info[6 + c] * 64u, static_cast<int16_t>(0x5A5A));
                coef[c] = plane[c].empty() ? nullptr : plane[c].data();
                bytes[c] = plane[c].size() * 2u;
            }
            const uint8_t* file = src.data();
            const size_t len = head;
            if (prog_emu_decode_batch(&file, &len, 1, coef, bytes, &rc, &status)) return 4;
            if (!status) for (int c = 0; c < 3; ++c) for (int16_t v : plane[c]) sum = sum * 0x01000193u ^ static_cast<uint16_t>(v);
        }
        std::printf("%d %u %u\n", rc, status, sum);
    }
    std::fclose(f);
    return 0;
}
#endif
