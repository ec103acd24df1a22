// ring_geometry_selftest.cpp - unified_audio_amd/csrc/ring_geometry.h against a brute-force list of positions.
// A ring is simulated literally: an array of cap rows, every position 0 .. e - 1 written to row p mod cap in turn.  For small cap,
// window, step and offset - and for offsets near 2^24 - the header's p(s), the visibility rule, the visible intervals and the capacity
// rule must agree with what that array holds.  Build with -fsanitize=address,undefined; prints "ring_geometry_selftest: ok".
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ring_geometry.h"

using namespace qa::ring;

static long long g_checks = 0;
#define CHECK(cond, ...)                                 \
    do {                                                 \
        ++g_checks;                                      \
        if (!(cond)) {                                   \
            std::fprintf(stderr, "FAILED %s: ", #cond);  \
            std::fprintf(stderr, __VA_ARGS__);           \
            std::fprintf(stderr, "\n");                  \
            std::exit(1);                                \
        }                                                \
    } while (0)

// the rows of a ring after positions 0 .. e - 1 were appended (-1: never written); for e beyond cap only the last cap matter
static std::vector<int64_t> brute_rows(int64_t e, int cap) {
    std::vector<int64_t> rows((size_t)cap, -1);
    for (int64_t p = e > cap ? e - cap : 0; p < e; ++p) rows[(size_t)(p % cap)] = p;
    return rows;
}

static void check_step(int cap, int context, int n, int64_t pos0) {
    const int64_t e = pos0 + n;
    const std::vector<int64_t> rows = brute_rows(e, cap);
    const int last_row = row_of(e - 1, cap);
    CHECK(rows[(size_t)last_row] == e - 1, "row_of cap %d e %lld", cap, (long long)e);
    std::vector<char> seen((size_t)cap, 0);
    for (int s = 0; s < cap; ++s) {
        const int64_t p = pos_of_row(s, e, cap);
        CHECK((p < 0) == (rows[(size_t)s] < 0) && (p < 0 || p == rows[(size_t)s]), "p(%d) = %lld, the ring holds %lld (cap %d, e %lld)", s,
              (long long)p, (long long)rows[(size_t)s], cap, (long long)e);
        CHECK(p == pos_at(s, e - 1, last_row, cap), "pos_at row %d", s);
        for (int i = 0; i < n; ++i) {
            const int64_t P = pos0 + i;
            const bool want = rows[(size_t)s] >= 0 && rows[(size_t)s] <= P && P - rows[(size_t)s] < context;
            CHECK(visible(p, P, context) == want, "visible row %d query %lld cap %d W %d", s, (long long)P, cap, context);
            seen[(size_t)s] = seen[(size_t)s] || want;
        }
    }
    // the intervals hold exactly the rows some query sees, when the ring is large enough for the step
    const Intervals iv = visible_rows(pos0, n, context, cap);
    CHECK(iv.n >= 1 && iv.n <= 2, "intervals %d", iv.n);
    for (int i = 0; i < iv.n; ++i) CHECK(0 <= iv.lo[i] && iv.lo[i] < iv.hi[i] && iv.hi[i] <= cap, "interval %d = [%d, %d)", i, iv.lo[i], iv.hi[i]);
    if (iv.n == 2) CHECK(iv.hi[0] <= iv.lo[1], "intervals overlap");
    for (int s = 0; s < cap; ++s) {
        const bool in = intersects(iv, s, s + 1);
        if (cap >= min_rows(context, n)) CHECK(in == (seen[(size_t)s] != 0), "row %d: interval %d, seen %d (cap %d W %d n %d pos0 %lld)", s, in,
                                               seen[(size_t)s], cap, context, n, (long long)pos0);
        else CHECK(in || !seen[(size_t)s], "row %d seen outside the intervals", s);
    }
    // ranges of rows, the way a split or a tile asks
    for (int a = 0; a < cap; a += 3)
        for (int b = a + 1; b <= cap; b += 2) {
            bool any = false;
            for (int s = a; s < b; ++s) any = any || intersects(iv, s, s + 1);
            CHECK(intersects(iv, a, b) == any, "range [%d, %d)", a, b);
        }
    // with min_rows rows no key that the first query sees was overwritten by the chunk's own appends
    if (cap >= min_rows(context, n)) {
        for (int64_t p = pos0 - context + 1 < 0 ? 0 : pos0 - context + 1; p <= pos0; ++p)
            CHECK(rows[(size_t)(p % cap)] == p, "position %lld lost (cap %d W %d n %d pos0 %lld)", (long long)p, cap, context, n, (long long)pos0);
    }
}

int main() {
    // capacity rule
    for (int W = 1; W <= 70; ++W)
        for (int n = 1; n <= 70; ++n) {
            const int64_t c = capacity(W, n);
            CHECK(c % ROW_ALIGN == 0 && c >= min_rows(W, n) + 1 && c < W + n + ROW_ALIGN, "capacity(%d, %d) = %lld", W, n, (long long)c);
        }
    CHECK(capacity(0, 4) == 0 && capacity(4, 0) == 0 && capacity(-1, 1) == 0, "capacity of no ring");
    CHECK(capacity(250, 16) == 288 && capacity(1500, 16) == 1536 && capacity(40, 512) == 576, "capacity examples");
    // small rings, every offset through several turns
    for (int cap = 1; cap <= 12; ++cap)
        for (int W = 1; W <= 13; ++W)
            for (int n = 1; n <= 5; ++n)
                for (int64_t pos0 = 0; pos0 <= 4 * cap + 3; ++pos0) check_step(cap, W, n, pos0);
    // tile-sized rings at offsets near the static table's end and near 2^24
    const int caps[] = {32, 64, 96};
    const int64_t bases[] = {8192 - 40, (1 << 20) - 17, MAX_POSITIONS - 140};
    for (int cap : caps)
        for (int W : {5, 33, cap - 15})
            for (int n : {1, 4, 16})
                for (int64_t base : bases)
                    for (int64_t pos0 = base; pos0 + n <= base + 130 && pos0 + n <= MAX_POSITIONS; pos0 += 7) check_step(cap, W, n, pos0);
    check_step(64, 49, 16, MAX_POSITIONS - 16);
    // the 2^24 check
    CHECK(positions_fit(0, 1) && positions_fit(MAX_POSITIONS - 16, 16) && !positions_fit(MAX_POSITIONS - 15, 16) && !positions_fit(-1, 1) &&
              positions_fit(MAX_POSITIONS, 0),
          "positions_fit");
    // every position below 2^24 is exact as a float
    CHECK((int64_t)(float)(MAX_POSITIONS - 1) == MAX_POSITIONS - 1 && (int64_t)(float)(MAX_POSITIONS + 1) != MAX_POSITIONS + 1, "fp32 exactness");
    std::printf("%lld checks\nring_geometry_selftest: ok\n", g_checks);
    return 0;
}
