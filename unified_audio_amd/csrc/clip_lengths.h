// clip_lengths.h - the length vector of a per-clip BiCodec / resample / wav_normalize call: check_row_lengths
// (row_lengths.h) with the refusal worded.  Host code without a HIP dependency, so that it also compiles into a stand-alone program under
// the host sanitizers (tools/clip_lengths_selftest.cpp).
#pragma once
#include <cstdint>
#include <vector>

#include "quarkaudio.h"
#include "row_lengths.h"

namespace qa {

void set_error(const char* fmt, ...);

// lengths: HOST memory, int64 [B], each in lo .. hi (`unit` names what they count, `hi_name` the call's own extent).  Fills out [B]
// (the values as the kernels read them) and *full (every entry equals hi: the call is the rectangular one).  The first entry outside
// the range fails the call with QA_ERR_INVALID and a message naming the entry point, the row and its value; nothing is launched
// before this returns.
inline int check_clip_lengths(const char* fn, int64_t B, const int64_t* lengths, int64_t lo, int64_t hi, const char* unit,
                              const char* hi_name, std::vector<int>* out, bool* full) {
    if (!lengths || !out || !full) {
        set_error("%s: null length vector", fn);
        return QA_ERR_INVALID;
    }
    if (B <= 0 || B >= (1 << 20) || hi < lo || hi > INT32_MAX) {
        set_error("%s: %lld clips of up to %lld %s", fn, (long long)B, (long long)hi, unit);
        return QA_ERR_INVALID;
    }
    const int64_t bad = check_row_lengths(lengths, B, lo, hi, out, full);
    if (bad >= 0) {
        set_error("%s: lengths[%lld] = %lld is outside %lld .. %s = %lld (%s)", fn, (long long)bad, (long long)lengths[bad], (long long)lo,
                  hi_name, (long long)hi, unit);
        return QA_ERR_INVALID;
    }
    return QA_OK;
}

}  // namespace qa
