// shim_errors.hpp -- the error categories of the ABI shim (abi_shim.cpp, shim_*.cpp): imageflow's ErrorCategory with its exit and HTTP maps, and
// the exception every refusal of a job travels in.  Standard library only, so that the JSON reader (shim_json.hpp) builds
// without the GPU runtime.
#pragma once
#include <cstdarg>
#include <cstdio>
#include <string>

namespace ifshim {

// ---- errors: ErrorCategory (imageflow_core/src/errors.rs:779-838) with its exit / HTTP maps (:849-902) -----------
enum Cat { kOk = 0, kOutOfMemory = 1, kArgumentInvalid = 2, kInvalidJson = 3, kImageMalformed = 4, kImageTypeNotSupported = 5,
           kNodeArgumentInvalid = 6, kGraphInvalid = 7, kActionNotSupported = 8, kIoError = 16, kInternalError = 18,
           kOperationCancelled = 21 };
// (ErrorKind::ColorProfileError, a profile the CMS cannot read, is of category ImageMalformed: errors.rs:241 -- code 4, HTTP 400, exit 65)
inline int http_code(int c) {
    switch (c) {
    case kOk: return 200;
    case kArgumentInvalid: case kGraphInvalid: case kNodeArgumentInvalid: case kActionNotSupported: case kInvalidJson:
    case kImageMalformed: case kImageTypeNotSupported: return 400;
    case kOutOfMemory: return 503;
    case kOperationCancelled: return 499;
    default: return 500;
    }
}
inline int exit_code(int c) {
    switch (c) {
    case kOk: return 0;
    case kArgumentInvalid: case kGraphInvalid: case kActionNotSupported: case kNodeArgumentInvalid: return 64;
    case kInvalidJson: case kImageMalformed: case kImageTypeNotSupported: return 65;
    case kOutOfMemory: return 71;
    case kIoError: return 74;
    case kOperationCancelled: return 130;
    default: return 70;
    }
}
struct FlowErr {
    int cat;
    std::string msg;
};
[[noreturn]] inline void raise(int cat, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
inline void raise(int cat, const char* fmt, ...) {
    char buf[768];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    throw FlowErr{cat, buf};
}

}  // namespace ifshim
