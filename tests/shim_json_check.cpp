// shim_json_check.cpp -- the ABI shim's JSON reader and parameter readers (csrc/shim_json.hpp, shim_json.cpp) in a program of
// their own, for the host sanitizers (tests/test_shim_json.py builds it with ASan + UBSan; nothing of the GPU runtime is in it).
//
//   shim_json_check <case file>
//
// The file holds cases: one kind byte, a u32le length, that many bytes.  One line of output per case.
//   'J'  a document for parse_json:  "S <to_json text>" when it parses and its text reads back to the same text,
//                                    "U <text> | <text of the text read back>" when it does not (never, the test says),
//                                    "E <category> <message>" for a FlowErr.
//   'P'  a call of a parameter reader, itself a JSON object {"fn": name, "arg": value}:  "V <integer>", or "E ..." as above.
//        parse_color, parse_filter (default -1), keyword_transparent and encode_coder get the value of "arg" (absent: a null
//        pointer); want_int and want_u32 read the key "arg" of the object.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "shim_json.hpp"

using namespace ifshim;

static void put(const std::string& line) {
    std::fwrite(line.data(), 1, line.size(), stdout);
    std::fputc('\n', stdout);
}

static void document(const uint8_t* p, size_t n) {
    std::string first, second;
    to_json(parse_json(p, n), &first);
    to_json(parse_json(reinterpret_cast<const uint8_t*>(first.data()), first.size()), &second);
    put(first == second ? "S " + first : "U " + first + " | " + second);
}

static void parameter(const uint8_t* p, size_t n) {
    const JVal call = parse_json(p, n);
    const JVal* fn = call.get("fn");
    const JVal* arg = call.get("arg");
    if (!fn || fn->t != JVal::Str) raise(kInternalError, "the case names no reader");
    int64_t v = 0;
    if (fn->s == "parse_color") v = parse_color(arg, "node");
    else if (fn->s == "parse_filter") v = parse_filter(arg, -1);
    else if (fn->s == "keyword_transparent") v = keyword_transparent(arg) ? 1 : 0;
    else if (fn->s == "encode_coder") v = encode_coder(arg);
    else if (fn->s == "want_int") v = want_int(call, "arg", "node");
    else if (fn->s == "want_u32") v = want_u32(call, "arg", "node");
    else raise(kInternalError, "the case names an unknown reader");
    char buf[32];
    std::snprintf(buf, sizeof buf, "V %" PRId64, v);
    put(buf);
}

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: %s <case file>\n", argv[0]); return 2; }
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 2; }
    std::vector<uint8_t> blob;
    uint8_t chunk[65536];
    for (size_t got; (got = std::fread(chunk, 1, sizeof chunk, f)) > 0;) blob.insert(blob.end(), chunk, chunk + got);
    std::fclose(f);
    size_t at = 0;
    while (at < blob.size()) {
        if (blob.size() - at < 5) { std::fprintf(stderr, "a case header is cut short at byte %zu\n", at); return 2; }
        const uint8_t kind = blob[at];
        const size_t n = static_cast<size_t>(blob[at + 1]) | static_cast<size_t>(blob[at + 2]) << 8 | static_cast<size_t>(blob[at + 3]) << 16 | static_cast<size_t>(blob[at + 4]) << 24;
        at += 5;
        if (blob.size() - at < n || (kind != 'J' && kind != 'P')) { std::fprintf(stderr, "a bad case at byte %zu\n", at - 5); return 2; }
        // a copy of exactly the case's size, so that a read past its end is a read past an allocation
        const std::vector<uint8_t> bytes(blob.begin() + static_cast<std::ptrdiff_t>(at), blob.begin() + static_cast<std::ptrdiff_t>(at + n));
        at += n;
        try {
            if (kind == 'J') document(bytes.data(), bytes.size());
            else parameter(bytes.data(), bytes.size());
        } catch (const FlowErr& e) {
            put("E " + std::to_string(e.cat) + " " + e.msg);
        }
    }
    return 0;
}
