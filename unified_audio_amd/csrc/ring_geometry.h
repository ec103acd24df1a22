// ring_geometry.h - the arithmetic of a ring K/V cache under a sliding window.  Host-only C++ with no HIP types:
// the launchers, the host checks of a ring stream and tools/ring_geometry_selftest.cpp all call these functions, and the kernels of
// stream_attn.hip call the constexpr ones, so one statement of the geometry is what the tests exercise.
//
// A ring of `cap` rows holds position p of a sequence in row p mod cap.  A step appends the nq positions pos0 .. e - 1 (e = pos0 + nq,
// the item's own end) FIRST and attends afterwards, so at attention time row s holds
//     p(s) = e - 1 - ((e - 1 - s) mod cap)
// and p(s) < 0 means the row was never written for this sequence (it may hold anything, NaN included).  The query at position P sees
// the key of row s iff 0 <= p(s) <= P and P - p(s) < context.
#pragma once
#include <cstdint>

namespace qa {
namespace ring {

constexpr int64_t MAX_POSITIONS = (int64_t)1 << 24;  // positions are exact as fp32 up to here: fr = (float)p * inv_freq
constexpr int ROW_ALIGN = 32;                        // the key tile of both attention kernels

// Rows of the ring for a window of left_context keys and chunks of up to max_chunk frames; 0 for arguments that have no ring.
// left_context - 1 + max_chunk rows are what the appends of a chunk need so that they never overwrite a key its first query still sees.
// One row more is kept: attention_kernel's ring mode follows RingKVCache.complete(), which counts the row under the write cursor (the
// oldest one, position e - cap) as not written, and a long chunk at the tight capacity would lose that key.  Rounded up to whole tiles.
constexpr int64_t capacity(int64_t left_context, int64_t max_chunk) {
    if (left_context < 1 || max_chunk < 1) return 0;
    const int64_t need = left_context + max_chunk;
    return (need + ROW_ALIGN - 1) / ROW_ALIGN * ROW_ALIGN;
}
// the fewest rows a ring may have for steps of n frames under `context` (the short kernel's own requirement; capacity() is above it)
constexpr int64_t min_rows(int64_t context, int64_t n) { return context - 1 + n; }

constexpr int row_of(int64_t p, int cap) { return (int)(p % cap); }  // p >= 0

// p(s) from the row of the last position, without a division: rows up to it hold the positions down from `last_pos`, the rows behind
// it the ones a full turn earlier
constexpr int64_t pos_at(int s, int64_t last_pos, int last_row, int cap) {
    return s <= last_row ? last_pos - (last_row - s) : last_pos - (last_row - s) - cap;
}
constexpr int64_t pos_of_row(int s, int64_t e, int cap) { return pos_at(s, e - 1, row_of(e - 1, cap), cap); }  // e >= 1, 0 <= s < cap

constexpr bool visible(int64_t p, int64_t P, int context) { return p >= 0 && p <= P && P - p < context; }

// The physical rows some query of a step (positions pos0 .. pos0 + nq - 1, window `context`) can see: at most two half-open intervals
// [lo[i], hi[i]), in row order.  n = 0: nothing (nq = 0).
struct Intervals {
    int n;
    int lo[2], hi[2];
};
constexpr Intervals visible_rows(int64_t pos0, int nq, int context, int cap) {
    Intervals iv = {0, {0, 0}, {0, 0}};
    if (nq <= 0) return iv;
    const int64_t e = pos0 + nq;
    int64_t first = pos0 - context + 1;  // the oldest key query pos0 sees
    if (first < 0) first = 0;
    if (first < e - cap) first = e - cap;  // older ones are overwritten (only below min_rows)
    const int64_t count = e - first;     // 1 .. cap
    const int r0 = row_of(first, cap);
    if (r0 + count <= cap) {
        iv.n = 1;
        iv.lo[0] = r0; iv.hi[0] = (int)(r0 + count);
    } else {
        iv.n = 2;
        iv.lo[0] = 0; iv.hi[0] = (int)(r0 + count - cap);
        iv.lo[1] = r0; iv.hi[1] = cap;
    }
    return iv;
}
// whether rows [a, b) hold a visible row
constexpr bool intersects(const Intervals& iv, int a, int b) {
    return (iv.n > 0 && a < iv.hi[0] && iv.lo[0] < b) || (iv.n > 1 && a < iv.hi[1] && iv.lo[1] < b);
}

// a row at `offset` positions may take `n` more: every position stays below 2^24
constexpr bool positions_fit(int64_t offset, int64_t n) { return offset >= 0 && n >= 0 && offset + n <= MAX_POSITIONS; }

}  // namespace ring
}  // namespace qa
