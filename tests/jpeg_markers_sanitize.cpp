// jpeg_markers_sanitize.cpp -- csrc/jpeg_markers.hpp alone, in a program of its own, for the host sanitizers
// (tests/test_jpeg_marker_walk.py builds it with -fsanitize=address,undefined).  Reads one file of cases, each behind a 4-byte
// little-endian length (tests/golden/make_jpeg_marker_golden.py write_sanitizer_corpus), copies every case into a heap block
// of exactly its size and drives the stepper and every segment reader over it the way the library's walks do: strictly up to
// the first scan header, as parse_jpeg and as read_jpeg ask their questions, and leniently, as the EXIF and ICC readers go.
// Prints: cases, frames the parse_jpeg walk takes, frames the read_jpeg walk takes, segments the lenient walk saw and the sum of
// their bytes.
#include <cstdio>
#include <memory>
#include <vector>

#include "jpeg_markers.hpp"

using namespace ifhip::jpeg;

// every byte of a segment is read: a payload that runs over the block is the sanitizer's to find
static unsigned touch(const Segment& s) {
    unsigned sum = 0;
    for (size_t k = 0; k < s.size; ++k) sum += s.data[k];
    return sum;
}

static bool frame_checks_as_read_jpeg(FrameHeader* f, Geometry* g, int adobe) {
    for (int c = 0; c < f->ncomp; ++c) if (!factors_in_range(*f, c)) return false;
    frame_geometry(f, g);
    return chroma_is_1x1(*f, *g) && !rgb_coded(*f, adobe);
}

// read_jpeg without planes: one frame header, judged at the SOF and again at an Adobe marker behind it; the first SOS ends it
static bool walk_as_read_jpeg(const uint8_t* d, size_t len) {
    if (!has_soi(d, len)) return false;
    Tables T;
    FrameHeader f;
    Geometry g;
    bool have_sof = false;
    size_t at = 2;
    Segment s;
    for (Step step; (step = next_segment(d, len, &at, &s)) != Step::End;) {
        if (step != Step::Segment) return false;
        uint32_t defined = 0;
        if (s.marker == kDQT) { if (!read_dqt(s, T.qt, T.qt_present)) return false; }
        else if (s.marker == kDHT) { if (!read_dht(s, T.dc, T.ac, &defined)) return false; }
        else if (s.marker == 0xC0 || s.marker == 0xC1 || s.marker == 0xC2) {
            if (have_sof || read_sof(s, &f) != Sof::Ok || f.width == 0 || f.height == 0 || !frame_checks_as_read_jpeg(&f, &g, T.adobe_transform)) return false;
            have_sof = true;
        }
        else if (is_sof(s.marker)) return false;
        else if (s.marker == kDRI) read_dri(s, &T.restart_interval);
        else if (read_adobe(s, &T.adobe_transform)) { if (have_sof && !frame_checks_as_read_jpeg(&f, &g, T.adobe_transform)) return false; }
        else if (s.marker == kSOS) return have_sof;
    }
    return have_sof;
}

// parse_jpeg: SOF0 / SOF1, a later one overwrites; the first SOS must name every component in order; the frame is judged behind it
static bool walk_as_parse_jpeg(const uint8_t* d, size_t len) {
    if (!has_soi(d, len)) return false;
    Tables T;
    FrameHeader f;
    Geometry g;
    uint8_t td[3] = {0, 0, 0}, ta[3] = {0, 0, 0};
    bool have_sof = false, have_scan = false;
    size_t at = 2;
    Segment s;
    for (Step step; !have_scan && (step = next_segment(d, len, &at, &s)) != Step::End;) {
        if (step != Step::Segment) return false;
        uint32_t defined = 0;
        if (s.marker == kDQT) { if (!read_dqt(s, T.qt, T.qt_present)) return false; }
        else if (s.marker == kDHT) { if (!read_dht(s, T.dc, T.ac, &defined)) return false; }
        else if (s.marker == 0xC0 || s.marker == 0xC1) { if (read_sof(s, &f) != Sof::Ok) return false; have_sof = true; }
        else if (is_sof(s.marker)) return false;
        else if (s.marker == kDRI) read_dri(s, &T.restart_interval);
        else if (s.marker == kSOS) {
            if (!have_sof || s.size < 1 || s.data[0] != f.ncomp || s.size < 4u + 2u * f.ncomp) return false;
            for (int c = 0; c < f.ncomp; ++c) {
                int named = -1;
                for (int k = 0; k < f.ncomp; ++k) if (f.comp_id[k] == s.data[1 + 2 * c]) named = k;
                td[c] = s.data[2 + 2 * c] >> 4; ta[c] = s.data[2 + 2 * c] & 15;
                if (named != c || td[c] > 3 || ta[c] > 3) return false;
            }
            have_scan = true;
        }
        else read_adobe(s, &T.adobe_transform);
    }
    if (!have_sof || !have_scan || f.width == 0 || f.height == 0 || rgb_coded(f, T.adobe_transform)) return false;
    for (int c = 0; c < f.ncomp; ++c)
        if (!factors_in_range(f, c) || !T.qt_present[f.tq[c]] || !T.dc[td[c]].present || !T.ac[ta[c]].present) return false;
    frame_geometry(&f, &g);
    return chroma_is_1x1(f, g) && within_block_limit(g);
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* in = std::fopen(argv[1], "rb");
    if (!in) return 2;
    unsigned long cases = 0, parse_ok = 0, read_ok = 0, lenient = 0, sum = 0;
    uint8_t n4[4];
    while (std::fread(n4, 1, 4, in) == 4) {
        const size_t len = n4[0] | (n4[1] << 8) | (n4[2] << 16) | (static_cast<size_t>(n4[3]) << 24);
        std::unique_ptr<uint8_t[]> d(new uint8_t[len]);                 // exactly `len` bytes: one past the end is a finding
        if (std::fread(d.get(), 1, len, in) != len) return 2;
        ++cases;
        parse_ok += walk_as_parse_jpeg(d.get(), len);
        read_ok += walk_as_read_jpeg(d.get(), len);
        if (has_soi(d.get(), len)) {
            size_t at = 2;
            for (Segment s; next_segment(d.get(), len, &at, &s) == Step::Segment && s.marker != kSOS; ++lenient) sum += touch(s);
        }
    }
    std::fclose(in);
    std::printf("%lu %lu %lu %lu %lu\n", cases, parse_ok, read_ok, lenient, sum);
    return 0;
}
