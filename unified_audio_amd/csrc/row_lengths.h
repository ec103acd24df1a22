// row_lengths.h - the host-side check of the length vector of a call with per-row lengths.  Plain C++ with no
// device code and no error text, so tools/row_lengths_selftest.cpp runs it under the host sanitizers; the caller words the refusal.
#pragma once
#include <cstdint>
#include <vector>

namespace qa {

// v: HOST memory, int64 [B], each entry in lo .. hi (lo and hi within int).  Returns the first row outside the range, or -1 when there is
// none; then out [B] holds the values as the kernels read them and *full whether every entry equals hi (the call is the rectangular one).
// Reads v[0 .. B) and nothing else; with B <= 0 it reads nothing, *out is empty and *full is true.
inline int64_t check_row_lengths(const int64_t* v, int64_t B, int64_t lo, int64_t hi, std::vector<int>* out, bool* full) {
    out->assign((size_t)(B > 0 ? B : 0), 0);
    *full = true;
    for (int64_t b = 0; b < B; ++b) {
        if (v[b] < lo || v[b] > hi) {
            *full = false;
            return b;
        }
        (*out)[(size_t)b] = (int)v[b];
        *full = *full && v[b] == hi;
    }
    return -1;
}

}  // namespace qa
