// lm_session_rows_selftest.cpp - the host side of per-row lengths on a qa_lm_cache session (csrc/lm_session_rows.h)
// as a stand-alone host program for the host sanitizers: the checks of a length vector, and the move plan of qa_lm_cache_select replayed
// on a host model of the cache.  Every vector lives in an exact-size heap block, so a read past either end is a report.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer \
//       -I unified_audio_amd/csrc tools/lm_session_rows_selftest.cpp -o /tmp/lm_session_rows_selftest && /tmp/lm_session_rows_selftest
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>

#include "lm_session_rows.h"

#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            return 1;                                                    \
        }                                                                \
    } while (0)

template <typename T>
static std::unique_ptr<T[]> exact(const std::vector<T>& v) {  // exact size: v.size() entries and not one more
    std::unique_ptr<T[]> p(new T[v.size() ? v.size() : 1]);
    if (!v.empty()) std::memcpy(p.get(), v.data(), sizeof(T) * v.size());
    return p;
}

static int check_rows() {
    using namespace qa;
    std::vector<int> out;
    int64_t row = -1;
    int active = -1;
    bool uniform = false;
    auto run = [&](std::vector<int64_t> n, std::vector<int> len, int64_t n_max, int max_len) {
        auto pn = exact(n);
        auto pl = exact(len);
        return check_session_rows(pn.get(), pl.get(), (int64_t)n.size(), n_max, max_len, &row, &out, &active, &uniform);
    };
    CHECK(run({5, 31, 32, 33}, {0, 0, 0, 0}, 33, 96) == SR_OK && active == 4 && !uniform && out == std::vector<int>({5, 31, 32, 33}));
    CHECK(run({7, 7, 7}, {4, 4, 4}, 7, 11) == SR_OK && uniform && active == 3);
    CHECK(run({7, 7, 7}, {4, 5, 4}, 7, 12) == SR_OK && !uniform);
    CHECK(run({0, 0}, {40, 3}, 8, 40) == SR_OK && active == 0 && !uniform);        // idle at max_len
    CHECK(run({3, 8}, {37, 20}, 8, 40) == SR_OK && active == 2);                   // ends exactly at max_len with n < n_max
    CHECK(run({1, 9, 1}, {0, 0, 0}, 8, 40) == SR_COUNT_RANGE && row == 1);
    CHECK(run({1, 1, -1}, {0, 0, 0}, 8, 40) == SR_COUNT_RANGE && row == 2);
    CHECK(run({1, 1, 3}, {4, 2, 6}, 4, 8) == SR_OVER_CAPACITY && row == 2);
    CHECK(run({INT64_MAX}, {1}, INT64_MAX, 8) == SR_OVER_CAPACITY && row == 0);    // no overflow in len + n
    auto crop = [&](std::vector<int64_t> lens, std::vector<int> len) {
        auto pc = exact(lens);
        auto pl = exact(len);
        return check_crop_rows(pc.get(), pl.get(), (int64_t)lens.size());
    };
    CHECK(crop({4, 2, 0}, {9, 2, 6}) == -1);
    CHECK(crop({4, 3, 6}, {4, 2, 6}) == 1);
    CHECK(crop({-1, 0}, {4, 2}) == 0);
    CHECK(crop({}, {}) == -1);
    return 0;
}

// a cache of `rows` rows x max_len positions of one int, plus the spare row; position p of old row r holds r * 1000 + p
static int check_moves(std::mt19937& rng, int B, int n, int max_batch, int max_len) {
    using namespace qa;
    const int rows = std::max(B, n);
    std::vector<int> len(max_batch, 0);
    std::vector<int64_t> idx(n);
    for (int r = 0; r < B; ++r) len[r] = (int)(rng() % (max_len + 1));
    for (int j = 0; j < n; ++j) idx[j] = (int64_t)(rng() % B);
    std::vector<int> cache((size_t)(max_batch + 1) * max_len, -7);  // row max_batch: the spare row; -7: never written
    for (int r = 0; r < B; ++r)
        for (int p = 0; p < len[r]; ++p) cache[(size_t)r * max_len + p] = r * 1000 + p;
    const std::vector<int> before = cache;
    auto pi = exact(idx);
    auto pl = exact(len);
    std::vector<KvMoves> waves;
    plan_cache_moves(pi.get(), pl.get(), n, rows, &waves);
    for (const KvMoves& w : waves) {
        CHECK(w.n >= 1 && w.n <= KV_MOVES_MAX);
        const std::vector<int> snap = cache;  // a launch reads the state the previous launch left
        for (int i = 0; i < w.n; ++i) {
            CHECK(w.dst[i] >= -1 && w.dst[i] < max_batch && w.src[i] >= -1 && w.src[i] < max_batch && w.dst[i] != w.src[i]);
            CHECK(w.len[i] >= 0 && w.len[i] <= max_len);
            for (int k = 0; k < w.n; ++k) CHECK(k == i || (w.dst[k] != w.src[i] && w.dst[k] != w.dst[i]));  // in-place safe inside a launch
            const size_t from = (size_t)(w.src[i] < 0 ? max_batch : w.src[i]) * max_len, to = (size_t)(w.dst[i] < 0 ? max_batch : w.dst[i]) * max_len;
            for (int p = 0; p < w.len[i]; ++p) cache[to + p] = snap[from + p];
        }
    }
    for (int j = 0; j < n; ++j) {
        const int src = (int)idx[j];
        for (int p = 0; p < len[src]; ++p) CHECK(cache[(size_t)j * max_len + p] == src * 1000 + p);
        // behind the new length nothing was written: a row is the destination of one move, which carries len[src] positions
        for (int p = len[src]; p < max_len; ++p) CHECK(cache[(size_t)j * max_len + p] == before[(size_t)j * max_len + p]);
    }
    for (int r = n; r < max_batch; ++r)  // rows outside the new batch are never written
        for (int p = 0; p < max_len; ++p) CHECK(cache[(size_t)r * max_len + p] == before[(size_t)r * max_len + p]);
    return 0;
}

int main() {
    if (check_rows()) return 1;
    std::mt19937 rng(1234);
    for (int it = 0; it < 4000; ++it) {
        const int max_batch = 1 + (int)(rng() % 40), max_len = 1 + (int)(rng() % 6);
        const int B = 1 + (int)(rng() % max_batch), n = 1 + (int)(rng() % max_batch);
        if (check_moves(rng, B, n, max_batch, max_len)) {
            std::fprintf(stderr, "iteration %d: B %d n %d max_batch %d max_len %d\n", it, B, n, max_batch, max_len);
            return 1;
        }
    }
    // 70 rows: maps with cycles through the spare row, and more than one wave of KV_MOVES_MAX moves
    for (int it = 0; it < 200; ++it)
        if (check_moves(rng, 70, 70, 70, 3)) return 1;
    std::puts("lm_session_rows_selftest: ok");
    return 0;
}
