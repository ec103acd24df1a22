// stream_step_selftest.cpp - the host plan of a stream step (unified_audio_amd/csrc/stream_step.h) against a naive
// restatement of its rules, as a stand-alone host program for the host sanitizers.  The restatement is straight-line, one block per
// fault, in plain 64-bit sums; the offsets and the length vector of every case live in exact-size heap blocks, so a read past either end
// is a report, and with B = 0 the planner gets pointers it must not read at all.  A case is one check: fault, row, `together` and, for a
// legal step, the five plan fields.  Every case is run; the program prints how many failed.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer -I unified_audio_amd/csrc
//       tools/stream_step_selftest.cpp -o stream_step_selftest && ./stream_step_selftest
#include <cstdio>
#include <cstring>
#include <memory>
#include <set>

#include "stream_step.h"

using namespace qa;

static long long g_checks = 0, g_failed = 0;

struct Stream {
    int rate, cap, first_min, window, max_chunk;
};
struct Want {
    StepFault fault = STEP_OK;
    int64_t row = -1;
    bool together = false;
    std::vector<int> cnt, first, pos0, nq;
    int max_keys = 0;
};

// the rules, restated.  frames null: every row takes n
static Want naive(const Stream& s, const std::vector<int>& off, const std::vector<int64_t>* frames, int64_t n) {
    const size_t B = off.size();
    const int64_t P = (int64_t)1 << 24;
    Want w;
    // 1. the length vector's range
    if (frames)
        for (size_t b = 0; b < B; ++b)
            if ((*frames)[b] < 0 || (*frames)[b] > n) {
                w.fault = STEP_COUNT_RANGE;
                w.row = (int64_t)b;
                return w;
            }
    std::vector<int64_t> cnt(B, n);
    if (frames) cnt = *frames;
    w.together = true;
    for (size_t b = 0; b < B; ++b)
        if (cnt[b] != n || off[b] != off[0]) w.together = false;
    // 2. a ring stream: per row, the chunk and then the positions
    if (s.window > 0)
        for (size_t b = 0; b < B; ++b) {
            if (s.rate * cnt[b] > s.max_chunk) {
                w.fault = STEP_RING_CHUNK;
                w.row = (int64_t)b;
                return w;
            }
            if ((int64_t)s.rate * off[b] + s.rate * cnt[b] > P) {
                w.fault = STEP_RING_POSITIONS;
                w.row = (int64_t)b;
                return w;
            }
        }
    int64_t largest = 0;
    bool all_zero = true;
    for (size_t b = 0; b < B; ++b) {
        if (off[b] > largest) largest = off[b];
        if (off[b] != 0) all_zero = false;
    }
    if (w.together) {
        // 3. the rectangular step
        if (all_zero && n < s.first_min) {
            w.fault = STEP_FIRST_SHORT;
            w.row = 0;
            return w;
        }
        if (s.window == 0 && largest + n > s.cap) {
            w.fault = STEP_OVER_CAPACITY;
            w.row = 0;
            return w;
        }
    } else {
        // 4. the step with per-row lengths
        bool idle = true;
        for (size_t b = 0; b < B; ++b) {
            if (off[b] == 0 && cnt[b] > 0 && cnt[b] < s.first_min) {
                w.fault = STEP_FIRST_SHORT;
                w.row = (int64_t)b;
                return w;
            }
            if (s.window == 0 && off[b] + cnt[b] > s.cap) {
                w.fault = STEP_OVER_CAPACITY;
                w.row = (int64_t)b;
                return w;
            }
            if (cnt[b] > 0) idle = false;
        }
        if (idle) {
            w.fault = STEP_ALL_IDLE;
            return w;
        }
    }
    for (size_t b = 0; b < B; ++b) {
        w.cnt.push_back((int)cnt[b]);
        w.first.push_back(off[b] == 0 && cnt[b] > 0 ? 1 : 0);
        w.pos0.push_back(s.rate * off[b]);
        w.nq.push_back((int)(s.rate * cnt[b]));
        if (w.pos0[b] + w.nq[b] > w.max_keys) w.max_keys = w.pos0[b] + w.nq[b];
    }
    return w;
}

static StepPlan g_plan;  // kept across cases, as a stream keeps it across steps: stale contents the call has to replace

// plan_step on exact-size copies of off and frames
static StepFault run(const Stream& s, const std::vector<int>& off, const std::vector<int64_t>* frames, int64_t n) {
    const size_t B = off.size();
    std::unique_ptr<int[]> po(B ? new int[B] : nullptr);  // B entries and not one more; none at all for B = 0
    std::unique_ptr<int64_t[]> pf(frames && B ? new int64_t[B] : nullptr);
    if (B) std::memcpy(po.get(), off.data(), sizeof(int) * B);
    if (frames && B) std::memcpy(pf.get(), frames->data(), sizeof(int64_t) * B);
    static int64_t none;  // B = 0 with lengths: a pointer that is not null and holds no entry to read
    const int64_t* f = !frames ? nullptr : B ? pf.get() : &none + 1;
    return plan_step(StreamView{po.get(), (int64_t)B, s.rate, s.cap, s.first_min, s.window, s.max_chunk}, f, n, &g_plan);
}

static void fail(const char* what, const Stream& s, const std::vector<int>& off, const std::vector<int64_t>* frames, int64_t n, StepFault got) {
    if (++g_failed > 12) return;
    std::fprintf(stderr, "FAILED %s: rate %d cap %d first_min %d window %d max_chunk %d n %lld, got fault %d row %lld together %d; rows (off",
                 what, s.rate, s.cap, s.first_min, s.window, s.max_chunk, (long long)n, (int)got, (long long)g_plan.row, (int)g_plan.together);
    for (size_t b = 0; b < off.size(); ++b) std::fprintf(stderr, " %d", off[b]);
    std::fprintf(stderr, ") (frames");
    for (size_t b = 0; frames && b < frames->size(); ++b) std::fprintf(stderr, " %lld", (long long)(*frames)[b]);
    std::fprintf(stderr, ")\n");
}

// one check: the planner against the restatement
static void check(const Stream& s, const std::vector<int>& off, const std::vector<int64_t>* frames, int64_t n, bool plan_only = false) {
    ++g_checks;
    const Want w = naive(s, off, frames, n);
    const StepFault got = run(s, off, frames, n);
    bool ok = got == w.fault && g_plan.row == w.row && g_plan.together == w.together;
    if (plan_only) ok = ok && got == STEP_OK;
    if (ok && got == STEP_OK)
        ok = g_plan.cnt == w.cnt && g_plan.first == w.first && g_plan.pos0 == w.pos0 && g_plan.nq == w.nq && g_plan.max_keys == w.max_keys;
    if (!ok) fail("against the restatement", s, off, frames, n, got);
}

// one check: the planner against a fault and a row written down here
static void expect(const Stream& s, const std::vector<int>& off, const std::vector<int64_t>* frames, int64_t n, StepFault fault, int64_t row) {
    ++g_checks;
    const StepFault got = run(s, off, frames, n);
    if (got != fault || g_plan.row != row) fail("against the stated fault", s, off, frames, n, got);
}

// every vector of B entries over `values`, in turn
template <typename T, typename F>
static void product(const std::vector<T>& values, size_t B, F&& each) {
    std::vector<T> v(B, values[0]);
    std::vector<size_t> i(B, 0);
    for (;;) {
        each(v);
        size_t k = 0;
        while (k < B && ++i[k] == values.size()) {
            i[k] = 0;
            v[k] = values[0];
            ++k;
        }
        if (k == B) return;
        v[k] = values[i[k]];
    }
}

template <typename T>
static std::vector<T> distinct(std::initializer_list<T> v) {
    const std::set<T> s(v);
    return std::vector<T>(s.begin(), s.end());
}

int main() {
    const int64_t P = (int64_t)1 << 24;
    // B = 1 .. 4, exhaustively, on a linear stream of 5 units: the Transformer's numbers (rate 1, no first-chunk minimum) and the codec's
    for (const Stream& s : {Stream{1, 5, 1, 0, 0}, Stream{2, 5, 3, 0, 0}})
        for (const int64_t n : {(int64_t)2, (int64_t)4}) {
            const std::vector<int> offsets = distinct<int>({0, 1, s.cap - 1, s.cap});
            const std::vector<int64_t> counts = distinct<int64_t>({-1, 0, 1, s.first_min - 1, s.first_min, n, n + 1});
            for (size_t B = 1; B <= 4; ++B)
                product(offsets, B, [&](const std::vector<int>& off) {
                    check(s, off, nullptr, n);
                    product(counts, B, [&](const std::vector<int64_t>& fr) { check(s, off, &fr, n); });
                });
        }
    // ring streams: window 5, max_chunk 4 Transformer frames, both rates; counts at max_chunk and one unit above, offsets around 2^24
    // positions (a row at P / rate with a chunk above max_chunk has both ring faults)
    for (const Stream& s : {Stream{1, 32, 1, 5, 4}, Stream{2, 16, 3, 5, 4}}) {
        const int64_t mc = s.max_chunk / s.rate, top = P / s.rate;
        const std::vector<int> offsets = distinct<int>({0, 1, (int)top - 1, (int)top, (int)top + 1});
        const std::vector<int64_t> counts = distinct<int64_t>({0, 1, mc, mc + 1});
        for (const int64_t n : {mc, mc + 1})
            for (size_t B = 1; B <= 3; ++B)
                product(offsets, B, [&](const std::vector<int>& off) {
                    check(s, off, nullptr, n);
                    product(counts, B, [&](const std::vector<int64_t>& fr) { check(s, off, &fr, n); });
                });
    }
    // precedence, one case per adjacent pair of the order, the two faults in different rows and in one row; fault and row written down
    {
        const Stream ring2{2, 16, 3, 5, 4}, ring2_short{2, 16, 3, 5, 2}, lin2{2, 5, 3, 0, 0}, lin2_tiny{2, 1, 3, 0, 0};
        std::vector<int64_t> fr;
        // range before the ring: a later row out of range wins over an earlier row's chunk; one row with both (3 > n = 2 = max_chunk)
        fr = {3, 4};
        expect(ring2, {4, 4}, &fr, 3, STEP_COUNT_RANGE, 1);
        fr = {3, 2};
        expect(ring2, {4, 4}, &fr, 2, STEP_COUNT_RANGE, 0);
        // within the ring check rows ascend, and of one row the chunk comes first
        fr = {1, 3};
        expect(ring2, {(int)(P / 2), 4}, &fr, 3, STEP_RING_POSITIONS, 0);
        fr = {3, 1};
        expect(ring2, {4, (int)(P / 2)}, &fr, 3, STEP_RING_CHUNK, 0);
        fr = {3, 1};
        expect(ring2, {(int)(P / 2), 4}, &fr, 3, STEP_RING_CHUNK, 0);
        // the ring before the rectangular step's first-chunk minimum (2 code frames: above a max_chunk of 1, below first_min = 3)
        expect(ring2_short, {0, 0}, nullptr, 2, STEP_RING_CHUNK, 0);
        expect(ring2, {0, 0}, nullptr, 2, STEP_FIRST_SHORT, 0);
        // the ring before the rows' first-chunk minimum: a later row's chunk wins over an earlier row's short start; one row with both
        fr = {1, 3};
        expect(ring2, {0, 4}, &fr, 3, STEP_RING_CHUNK, 1);
        fr = {2, 0};
        expect(ring2_short, {0, 4}, &fr, 2, STEP_RING_CHUNK, 0);
        // rectangular: the first-chunk minimum before the capacity
        expect(lin2_tiny, {0, 0}, nullptr, 2, STEP_FIRST_SHORT, 0);
        expect(lin2_tiny, {1, 1}, nullptr, 2, STEP_OVER_CAPACITY, 0);
        // per row: rows ascend whichever fault, and of one row the first-chunk minimum comes first
        fr = {3, 1};
        expect(lin2, {4, 0}, &fr, 3, STEP_OVER_CAPACITY, 0);
        fr = {1, 3};
        expect(lin2, {0, 4}, &fr, 3, STEP_FIRST_SHORT, 0);
        fr = {2, 0};
        expect(lin2_tiny, {0, 0}, &fr, 2, STEP_FIRST_SHORT, 0);
        // a row's capacity before "every row idles" is even asked; idle rows alone
        fr = {0, 1};
        expect(lin2, {0, 5}, &fr, 3, STEP_OVER_CAPACITY, 1);
        fr = {0, 0};
        expect(lin2, {0, 5}, &fr, 3, STEP_ALL_IDLE, -1);
        // no lengths on rows at different offsets: per-row rules with n everywhere (row 1 is refused as a row, not as the rectangle)
        expect(lin2, {0, 3}, nullptr, 3, STEP_OVER_CAPACITY, 1);
        // a ring has no capacity to exceed, at any offset
        expect(ring2, {1000, 1000}, nullptr, 2, STEP_OK, -1);
        // the compares form no sum: the ends of int64 as n, offsets at the top of a linear stream of 2^24 Transformer frames
        const Stream big{2, (int)(P / 2), 3, 0, 0};
        expect(big, {(int)(P / 2), (int)(P / 2)}, nullptr, INT64_MAX, STEP_OVER_CAPACITY, 0);
        expect(big, {(int)(P / 2), 0}, nullptr, INT64_MAX, STEP_OVER_CAPACITY, 0);
        expect(ring2, {0, 0}, nullptr, INT64_MAX, STEP_RING_CHUNK, 0);
        fr = {INT32_MAX, INT64_MIN};
        expect(big, {0, 0}, &fr, INT32_MAX, STEP_COUNT_RANGE, 1);
        fr = {INT32_MAX, INT64_MAX};
        expect(big, {0, 0}, &fr, INT32_MAX, STEP_COUNT_RANGE, 1);
        fr = {INT32_MAX, INT32_MAX};
        expect(big, {1, 1}, &fr, INT32_MAX, STEP_OVER_CAPACITY, 0);
    }
    // size: B = 129, legal vectors from a fixed seed, for the plan fields alone
    {
        uint64_t seed = 0x9E3779B97F4A7C15ull;
        auto next = [&](uint64_t m) {
            seed = seed * 6364136223846793005ull + 1442695040888963407ull;
            return (int64_t)((seed >> 33) % m);
        };
        for (const Stream& s : {Stream{1, 4000, 1, 0, 0}, Stream{2, 2000, 3, 0, 0}, Stream{2, 288, 3, 250, 32}})
            for (int rep = 0; rep < 64; ++rep) {
                const int64_t n = s.window ? s.max_chunk / s.rate : 40;
                std::vector<int> off(129);
                std::vector<int64_t> fr(129);
                for (size_t b = 0; b < off.size(); ++b) {
                    off[b] = next(3) == 0 ? 0 : (int)next(s.window ? P / s.rate - n : s.cap - n);
                    fr[b] = next(4) == 0 ? 0 : s.first_min + next(n - s.first_min + 1);
                }
                fr[(size_t)next(129)] = n;  // at least one row is live
                check(s, off, &fr, n, true);
            }
    }
    // empty: B = 0 reads nothing, with and without lengths, and there is no row to refuse (no stream is begun with B = 0)
    check(Stream{1, 5, 1, 0, 0}, {}, nullptr, 2);
    {
        const std::vector<int64_t> fr;
        check(Stream{2, 5, 3, 0, 0}, {}, &fr, 4);
        check(Stream{2, 16, 3, 5, 4}, {}, &fr, 3);
    }
    if (g_failed) {
        std::fprintf(stderr, "stream_step_selftest: %lld of %lld checks FAILED\n", g_failed, g_checks);
        return 1;
    }
    std::printf("stream_step_selftest: ok (%lld checks)\n", g_checks);
    return 0;
}
