// stream_step.h - the host plan of one step of a stream: whether the step is legal and, if it is, what its kernels
// read.  The streaming H-Codec encoder and the stand-alone codec Transformer both step through plan_step; they differ in the numbers of
// StreamView alone.  Plain C++ with no device code, no knobs and no error text, so tools/stream_step_selftest.cpp runs it under the host
// sanitizers; hcodec.cpp words the refusal.
#pragma once
#include <algorithm>

#include "ring_geometry.h"
#include "row_lengths.h"

namespace qa {

// The stream as the planner sees it.  A unit is what the caller counts: code frames of the H-Codec stream (rate 2), frames of a
// Transformer stream (rate 1).
//   off [B]            units of every row since begin / its reset; not read for B = 0
//   rate               Transformer frames per unit
//   cap                units a row of a linear stream holds
//   first_min          the fewest units of a row's first chunk (1: no minimum)
//   window, max_chunk  ring stream: the sliding window and the most a step may take, in Transformer frames; window 0: a linear stream
struct StreamView {
    const int* off;
    int64_t B;
    int rate, cap, first_min, window, max_chunk;
};

// Why a step is refused: frames[row] outside 0 .. n | ring: the row's chunk is above max_chunk | ring: the row would pass 2^24 Transformer
// positions | a row at offset 0 takes fewer than first_min units | linear: the row would end behind cap | every row takes 0
enum StepFault { STEP_OK = 0, STEP_COUNT_RANGE, STEP_RING_CHUNK, STEP_RING_POSITIONS, STEP_FIRST_SHORT, STEP_OVER_CAPACITY, STEP_ALL_IDLE };

// What a legal step carries to its kernels (section 45): per row the count in the caller's unit, whether the row starts a sequence in this
// step, and its Transformer position and query count - the four vectors a step with per-row lengths uploads, in this order.
struct StepPlan {
    std::vector<int> cnt, first, pos0, nq;
    int max_keys = 0;      // max_b(pos0[b] + nq[b]): the split count of the short attention, the key walk of the long one
    bool together = true;  // every row is at one offset and takes all n: the rectangular step, which needs no row arrays
    int64_t row = -1;      // of a refusal: the first offending row (-1 for STEP_ALL_IDLE)
};

// One step of n >= 1 units per row, or of frames[b] <= n units of row b (frames: the caller's HOST vector [B]; null: every row takes n).
// n is any value without lengths and within int with them (check_row_lengths).  STEP_OK: *p is the plan.  Otherwise the fault, p->row
// and p->together (false when the lengths are out of range); the other fields hold nothing.  Of several faults the one reported is the
// first in this order:
//   1. the first row with frames[b] outside 0 .. n
//   2. ring stream: the first row whose chunk is above max_chunk or whose positions pass 2^24; of one row, the chunk first
//   3. row by row: the first-chunk minimum of a row that starts (offset 0, 0 < count < first_min), then (linear) its capacity; behind all
//      rows, that every row idles
// The rectangular step (`together`) is step 3 on rows that are alike - its first row speaks for all, and the largest offset is every
// row's - and a step without lengths on rows at different offsets is one with per-row lengths of n each.  No sum is formed that could
// overflow: offsets go up to 2^24 / rate.
inline StepFault plan_step(const StreamView& s, const int64_t* frames, int64_t n, StepPlan* p) {
    const size_t B = (size_t)(s.B > 0 ? s.B : 0);
    p->row = -1;
    p->max_keys = 0;
    p->together = false;
    bool full = true;
    if (frames) {
        p->row = check_row_lengths(frames, s.B, 0, n, &p->cnt, &full);
        if (p->row >= 0) return STEP_COUNT_RANGE;
    }
    p->together = full;
    for (size_t b = 1; b < B; ++b) p->together = p->together && s.off[b] == s.off[0];
    auto count = [&](size_t b) { return frames ? frames[b] : n; };
    if (s.window > 0)
        for (size_t b = 0; b < B; ++b) {
            p->row = (int64_t)b;
            if (count(b) > s.max_chunk / s.rate) return STEP_RING_CHUNK;  // rate * count > max_chunk, without the product
            if (!ring::positions_fit((int64_t)s.rate * s.off[b], s.rate * count(b))) return STEP_RING_POSITIONS;
        }
    bool live = B == 0;
    for (size_t b = 0; b < B; ++b) {
        const int64_t f = count(b);
        p->row = (int64_t)b;
        live = live || f > 0;
        if (s.off[b] == 0 && f > 0 && f < s.first_min) return STEP_FIRST_SHORT;
        if (s.window <= 0 && f > (int64_t)s.cap - s.off[b]) return STEP_OVER_CAPACITY;  // off + f > cap, without the sum
    }
    p->row = -1;
    if (!live) return STEP_ALL_IDLE;
    if (!frames) p->cnt.assign(B, (int)n);
    p->first.resize(B); p->pos0.resize(B); p->nq.resize(B);
    for (size_t b = 0; b < B; ++b) {
        p->first[b] = s.off[b] == 0 && p->cnt[b] > 0;
        p->pos0[b] = s.rate * s.off[b];
        p->nq[b] = s.rate * p->cnt[b];
        p->max_keys = std::max(p->max_keys, p->pos0[b] + p->nq[b]);
    }
    return STEP_OK;
}

}  // namespace qa
