// conv_offsets.h - the host-side check behind the 32-bit entries of conv_gemm's source-frame table.  An entry is a
// float offset relative to the FIRST clip a row tile touches: (clip - clip0) * T_in * ldx + frame * ldx.  Plain C++ with no device code and
// no error text, so tools/conv_offsets_selftest.cpp runs it under the host sanitizers; the caller words the refusal.
#pragma once
#include <cstdint>

namespace qa {

constexpr int64_t CONV_OFFSET_LIMIT = INT64_C(1) << 31;  // a table entry is an int, -1 = zero padding

// The bound on every entry of a tile of `bm` rows of a [B, t_out] row grid whose clips are t_in frames of ldx floats apart:
// rows m0 .. m0 + bm - 1 lie in the clips m0 / t_out .. (m0 + bm - 1) / t_out, at most ceil(bm / t_out) + 1 of them for any m0, and an
// entry stays below (that many clips) * t_in * ldx.  Saturates at INT64_MAX instead of overflowing; 0 for an empty grid or clip.
inline int64_t conv_tile_offset_span(int64_t bm, int64_t t_out, int64_t t_in, int64_t ldx) {
    if (bm <= 0 || t_out <= 0 || t_in <= 0 || ldx <= 0) return 0;
    const int64_t clips = bm / t_out + (bm % t_out != 0) + 1;  // no bm + t_out: t_out may be anything up to INT64_MAX
    if (t_in > INT64_MAX / ldx) return INT64_MAX;
    const int64_t clip = t_in * ldx;
    if (clip > INT64_MAX / clips) return INT64_MAX;
    return clips * clip;
}

// whether the table of such a tile fits its 32-bit entries; *span (may be null) receives the bound for the caller's message
inline bool conv_tile_offsets_fit(int64_t bm, int64_t t_out, int64_t t_in, int64_t ldx, int64_t* span) {
    const int64_t s = conv_tile_offset_span(bm, t_out, t_in, ldx);
    if (span) *span = s;
    return s < CONV_OFFSET_LIMIT;
}

}  // namespace qa
