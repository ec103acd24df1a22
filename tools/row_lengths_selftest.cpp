// row_lengths_selftest.cpp - the host check of the length vector of a call with per-row lengths (csrc/row_lengths.h)
// as a stand-alone host program for the host sanitizers.  Every vector lives in an exact-size heap block, so a read past either end is a
// report; with B <= 0 the function gets a pointer it must not read at all.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer \
//       -I unified_audio_amd/csrc tools/row_lengths_selftest.cpp -o /tmp/row_lengths_selftest && /tmp/row_lengths_selftest
#include <cstdio>
#include <cstring>
#include <memory>

#include "row_lengths.h"

#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            return 1;                                                    \
        }                                                                \
    } while (0)

static std::vector<int> g_out;
static bool g_full;

// check_row_lengths on an exact-size copy of v
static int64_t run(const std::vector<int64_t>& v, int64_t lo, int64_t hi) {
    const size_t B = v.size();
    std::unique_ptr<int64_t[]> p(B ? new int64_t[B] : nullptr);  // B entries and not one more; none at all for B = 0
    if (B) std::memcpy(p.get(), v.data(), sizeof(int64_t) * B);
    g_out.assign(3, -7);  // stale contents the call has to replace
    g_full = false;
    return qa::check_row_lengths(p.get(), (int64_t)B, lo, hi, &g_out, &g_full);
}

int main() {
    const int64_t lo = 3, hi = 11;
    // B = 0 (and below): nothing is read - not even a null pointer - nothing is wrong, the output is empty
    CHECK(run({}, lo, hi) == -1 && g_out.empty() && g_full);
    g_full = false;
    CHECK(qa::check_row_lengths(nullptr, -4, lo, hi, &g_out, &g_full) == -1 && g_out.empty() && g_full);
    for (const int B : {1, 2, 257}) {
        const int rows[3] = {0, B / 2, B - 1};  // the first, a middle and the last row (they coincide for small B)
        // every row at hi: full
        std::vector<int64_t> v((size_t)B, hi);
        CHECK(run(v, lo, hi) == -1 && g_full && (int)g_out.size() == B);
        for (int b = 0; b < B; ++b) CHECK(g_out[(size_t)b] == (int)hi);
        for (const int r : rows) {
            // lo and an inner value are accepted and copied; the call is no longer full
            for (const int64_t ok : {lo, lo + 1, hi - 1}) {
                v.assign((size_t)B, hi);
                v[(size_t)r] = ok;
                CHECK(run(v, lo, hi) == -1 && !g_full && (int)g_out.size() == B && g_out[(size_t)r] == (int)ok);
                for (int b = 0; b < B; ++b) CHECK(b == r || g_out[(size_t)b] == (int)hi);
            }
            // one step outside either end, and the ends of int64, are refused with the row
            for (const int64_t bad : {lo - 1, hi + 1, INT64_MIN, INT64_MAX}) {
                v.assign((size_t)B, hi);
                v[(size_t)r] = bad;
                CHECK(run(v, lo, hi) == r && !g_full);
            }
        }
        if (B >= 2) {  // of two bad rows the first is reported, whatever the second holds
            v.assign((size_t)B, lo);
            v[(size_t)(B / 2)] = hi + 1;
            v[(size_t)(B - 1)] = lo - 1;
            CHECK(run(v, lo, hi) == B / 2);
            v[0] = INT64_MIN;
            CHECK(run(v, lo, hi) == 0);
        }
    }
    // a range of one value: every accepted vector is full
    CHECK(run({5, 5, 5}, 5, 5) == -1 && g_full);
    CHECK(run({5, 4, 5}, 5, 5) == 1 && run({5, 5, 6}, 5, 5) == 2);
    // lo = 0 (idle rows of a session call) and the whole int range as hi
    CHECK(run({0, 2, 0}, 0, 2) == -1 && !g_full && g_out == std::vector<int>({0, 2, 0}));
    CHECK(run({INT32_MAX, 1}, 1, INT32_MAX) == -1 && !g_full && g_out[0] == INT32_MAX);
    CHECK(run({INT32_MAX, (int64_t)INT32_MAX + 1}, 1, INT32_MAX) == 1);
    std::puts("row_lengths_selftest: ok");
    return 0;
}
