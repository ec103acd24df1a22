// lm_session_rows.h - the host side of per-row lengths on a qa_lm_cache session: the checks of a length vector and
// the move plan of qa_lm_cache_select.  Plain C++ with no device code, so tools/lm_session_rows_selftest.cpp runs it under the host
// sanitizers; lm.cpp turns a refusal into the library's error message.
#pragma once
#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

namespace qa {

// one wave of independent row moves of a KV cache (qa_lm_cache_select), passed by value to the kernel: row src[i] -> row dst[i],
// -1 = the spare row
constexpr int KV_MOVES_MAX = 32;
struct KvMoves {
    int n;
    int dst[KV_MOVES_MAX], src[KV_MOVES_MAX];
    int len[KV_MOVES_MAX];  // positions move i copies: the length of the row it carries (0: nothing to copy)
};

// why a length vector of a session call is refused
enum SessionRowsFault { SR_OK = 0, SR_COUNT_RANGE = 1, SR_OVER_CAPACITY = 2 };

// n [B] (the caller's HOST vector) against the rows' lengths len [B]: every n[b] in 0 .. n_max and len[b] + n[b] <= max_len.  The first
// offending row goes to *row.  On SR_OK: *n_out [B] holds the counts as ints, *active the rows with n[b] > 0, *uniform whether the call is
// rectangular (every row at one length and every n[b] == n_max).
inline SessionRowsFault check_session_rows(const int64_t* n, const int* len, int64_t B, int64_t n_max, int max_len, int64_t* row,
                                           std::vector<int>* n_out, int* active, bool* uniform) {
    n_out->assign((size_t)B, 0);
    *active = 0;
    *uniform = true;
    for (int64_t b = 0; b < B; ++b) {
        *row = b;
        if (n[b] < 0 || n[b] > n_max) return SR_COUNT_RANGE;
        if (n[b] > (int64_t)max_len - len[b]) return SR_OVER_CAPACITY;  // len[b] + n[b] > max_len, without the sum
        (*n_out)[(size_t)b] = (int)n[b];
        if (n[b] > 0) ++*active;
        if (n[b] != n_max || len[b] != len[0]) *uniform = false;
    }
    return SR_OK;
}

// lens [B] of qa_lm_cache_crop_rows against the rows' lengths: the first row with lens[b] outside 0 .. len[b], or -1
inline int64_t check_crop_rows(const int64_t* lens, const int* len, int64_t B) {
    for (int64_t b = 0; b < B; ++b)
        if (lens[b] < 0 || lens[b] > len[b]) return b;
    return -1;
}

// qa_lm_cache_select as waves of row moves.  Row j must become old row idx[j], contents and length (len_old [rows]: the lengths before the
// call).  A move may run once nothing still pending reads its destination, so the moves are emitted leaves first; what is left then is
// disjoint cycles, each opened by parking one row in the cache's spare row (-1).  Consecutive moves that neither read nor overwrite one
// another's rows share a launch.  Every move carries the length of the row it moves (a parked row its own), so rows of different lengths
// share a wave and a row of length 0 costs nothing.
inline void plan_cache_moves(const int64_t* idx, const int* len_old, int n, int rows, std::vector<KvMoves>* waves) {
    std::vector<int> src(n), readers(rows + 1, 0);  // readers[r + 1]: pending moves that read row r (r = -1: the spare row)
    std::vector<char> pending(n, 0);
    int left = 0;
    for (int j = 0; j < n; ++j) {
        src[j] = (int)idx[j];
        if (src[j] != j) {
            pending[j] = 1;
            ++readers[src[j] + 1];
            ++left;
        }
    }
    struct Move {
        int dst, src, len;
    };
    std::vector<Move> order;
    auto emit_free = [&] {
        for (bool progress = true; progress;) {
            progress = false;
            for (int j = 0; j < n; ++j)
                if (pending[j] && readers[j + 1] == 0) {
                    order.push_back({j, src[j], len_old[idx[j]]});  // from the spare row too: it holds old row idx[j]
                    --readers[src[j] + 1];
                    pending[j] = 0;
                    --left;
                    progress = true;
                }
        }
    };
    emit_free();
    while (left > 0) {  // only cycles are left: park one row of a cycle, let its reader take the spare row instead
        int j = 0;
        while (!pending[j]) ++j;
        order.push_back({-1, j, len_old[j]});
        for (int k = 0; k < n; ++k)
            if (pending[k] && src[k] == j) {
                src[k] = -1;
                ++readers[0];
            }
        readers[j + 1] = 0;
        emit_free();
    }
    KvMoves w{};
    std::vector<char> rd(rows + 1, 0), wr(rows + 1, 0);
    auto flush = [&] {
        if (w.n) waves->push_back(w);
        w = KvMoves{};
        std::fill(rd.begin(), rd.end(), 0);
        std::fill(wr.begin(), wr.end(), 0);
    };
    for (const Move& m : order) {
        if (w.n == KV_MOVES_MAX || wr[m.src + 1] || rd[m.dst + 1] || wr[m.dst + 1]) flush();
        w.dst[w.n] = m.dst;
        w.src[w.n] = m.src;
        w.len[w.n] = m.len;
        ++w.n;
        wr[m.dst + 1] = 1;
        rd[m.src + 1] = 1;
    }
    flush();
}

}  // namespace qa
