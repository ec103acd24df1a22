// lm_cond_rows_selftest.cpp - the condition form of the host plan of a scoring call with per-row lengths (csrc/lm_score_rows.h,
// ScoreRowsShape::cond_form) as a stand-alone host program for the host sanitizers.  The form of
// CustomLlamaModel.forward: prompt [mix_sos, cond[b, :n_cond[b]]] or none, no enrollment, the last position of a row's OWN stream dropped
// (Lt_b = G + n_semantic[b] + 1).  Every vector lives in an exact-size heap block, so a read past either end is a report.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I unified_audio_amd/csrc \
//       tools/lm_cond_rows_selftest.cpp -o /tmp/lm_cond_rows_selftest && /tmp/lm_cond_rows_selftest
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "lm_score_rows.h"

#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            return 1;                                                    \
        }                                                                \
    } while (0)

using namespace qa;
typedef std::vector<int64_t> Vec;

static std::unique_ptr<int64_t[]> exact(const Vec& v) {  // exact size: v.size() entries and not one more
    std::unique_ptr<int64_t[]> p(new int64_t[v.size() ? v.size() : 1]);
    if (!v.empty()) std::memcpy(p.get(), v.data(), sizeof(int64_t) * v.size());
    return p;
}

static ScoreRowsShape shape(int64_t B, int64_t Tc_max, int64_t T_max, int G) {
    ScoreRowsShape s;
    s.B = B; s.cond_form = true; s.nm_max = Tc_max; s.T_max = T_max; s.G = G;
    return s;
}

struct Run {
    ScoreRows R;
    int64_t row = -1, value = -1;
    ScoreRowsFault f = SCR_OK;
};

static Run run(const ScoreRowsShape& s, const Vec* nc, const Vec* T) {
    Run r;
    auto pc = nc ? exact(*nc) : nullptr;
    auto pt = T ? exact(*T) : nullptr;
    r.f = plan_score_rows(nullptr, pc.get(), pt.get(), s, &r.R, &r.row, &r.value);
    return r;
}

// the plan against a naive recount of the condition form
static int check_plan(const ScoreRowsShape& s, const Vec* nc, const Vec* T) {
    const Run r = run(s, nc, T);
    CHECK(r.f == SCR_OK);
    const ScoreRows& R = r.R;
    const size_t B = (size_t)s.B;
    CHECK(R.Lp.size() == B && R.Lt.size() == B && R.L.size() == B && R.off.size() == B && R.nm.size() == B && R.T.size() == B && R.ne.size() == B);
    CHECK(R.Lp_max == (s.nm_max > 0 ? 1 + (int)s.nm_max : 0));
    long long total = 0;
    bool uniform = true;
    for (size_t b = 0; b < B; ++b) {
        const int64_t c = s.nm_max > 0 ? (nc ? (*nc)[b] : s.nm_max) : 0, t = T ? (*T)[b] : s.T_max;
        CHECK(R.ne[b] == 0 && R.nm[b] == c && R.T[b] == t);
        CHECK(R.Lp[b] == (s.nm_max > 0 ? 1 + c : 0));
        CHECK(R.Lt[b] == s.G + t + 1);  // the last position of the row's own stream is dropped
        CHECK(R.L[b] == R.Lp[b] + R.Lt[b] && R.L[b] <= s.max_pos);
        CHECK(R.off[b] == total);
        total += R.Lt[b];
        uniform = uniform && c == (s.nm_max > 0 ? s.nm_max : 0) && t == s.T_max;
    }
    CHECK(R.total_rows == total && R.uniform == uniform);
    CHECK(R.groups.size() == (B + 63) / 64);
    size_t b0 = 0;
    long long body = 0, packed = 0;
    for (const ScoreGroup& g : R.groups) {
        CHECK((size_t)g.b0 == b0 && g.gb == (int)std::min<size_t>(64, B - b0) && g.row0 == R.off[b0]);
        int n = 0, lt = 0;
        long long rows = 0;
        for (int i = 0; i < g.gb; ++i) {
            n = std::max(n, R.L[b0 + i]);
            lt = std::max(lt, R.Lt[b0 + i]);
            rows += R.Lt[b0 + i];
        }
        CHECK(g.n == n && g.Lt_max == lt && g.rows == rows);
        body = std::max(body, (long long)g.gb * n);
        packed = std::max(packed, rows);
        b0 += (size_t)g.gb;
    }
    CHECK(b0 == B && R.body_rows_max == body && R.packed_rows_max == packed);
    return 0;
}

// B rows with `first`, `middle`, `last` at rows 0, B / 2 and B - 1 and `fill` elsewhere
static Vec spread(int64_t B, int64_t fill, int64_t first, int64_t middle, int64_t last) {
    Vec v((size_t)B, fill);
    v[(size_t)(B / 2)] = middle;
    v[(size_t)(B - 1)] = last;
    v[0] = first;
    return v;
}

static int check_batches() {
    const int64_t Tc = 18, T = 11;
    const int G = 6;
    for (int64_t B : {(int64_t)1, (int64_t)2, (int64_t)65}) {
        const ScoreRowsShape s = shape(B, Tc, T, G);
        // both ends of each range in the first, a middle and the last row
        for (int64_t edge_c : {(int64_t)1, Tc})
            for (int64_t edge_t : {(int64_t)0, T})
                for (int where = 0; where < 3; ++where) {
                    const int64_t other_c = edge_c == 1 ? Tc : 1, other_t = edge_t == 0 ? T : 0;
                    Vec nc = spread(B, 9, where == 0 ? edge_c : other_c, where == 1 ? edge_c : other_c, where == 2 ? edge_c : other_c);
                    Vec ts = spread(B, 5, where == 0 ? edge_t : other_t, where == 1 ? edge_t : other_t, where == 2 ? edge_t : other_t);
                    if (check_plan(s, &nc, &ts)) return 1;
                    if (check_plan(s, &nc, nullptr)) return 1;
                    if (check_plan(s, nullptr, &ts)) return 1;
                    // one step outside either end, in the same row: refused, naming that row and value
                    const size_t at = where == 0 ? 0 : where == 1 ? (size_t)(B / 2) : (size_t)(B - 1);
                    for (int64_t bad : {(int64_t)0, Tc + 1, (int64_t)-3}) {
                        Vec v = nc;
                        for (size_t b = 0; b < at; ++b) v[b] = 9;
                        v[at] = bad;
                        const Run r = run(s, &v, &ts);
                        CHECK(r.f == SCR_MIX_RANGE && r.row == (int64_t)at && r.value == bad);
                    }
                    for (int64_t bad : {(int64_t)-1, T + 1}) {
                        Vec v = ts;
                        for (size_t b = 0; b < at; ++b) v[b] = 5;
                        v[at] = bad;
                        const Run r = run(s, &nc, &v);
                        CHECK(r.f == SCR_SEMANTIC_RANGE && r.row == (int64_t)at && r.value == bad);
                    }
                }
        // n_semantic = 0 in every row: Lt = G + 1
        {
            Vec ts((size_t)B, 0);
            const Run r = run(s, nullptr, &ts);
            CHECK(r.f == SCR_OK && !r.R.uniform && r.R.total_rows == (long long)B * (G + 1));
            if (check_plan(s, nullptr, &ts)) return 1;
        }
        // every vector uniform -> uniform, whichever of them is given
        {
            Vec nc((size_t)B, Tc), ts((size_t)B, T);
            CHECK(run(s, &nc, &ts).R.uniform && run(s, &nc, nullptr).R.uniform && run(s, nullptr, &ts).R.uniform && run(s, nullptr, nullptr).R.uniform);
            nc[(size_t)(B - 1)] = Tc - 1;
            CHECK(!run(s, &nc, &ts).R.uniform);
            if (check_plan(s, &nc, &ts)) return 1;
        }
    }
    return 0;
}

static int check_too_long_and_no_condition() {
    // 1 + 3000 + (6 + 1090 + 1) = 4098 positions at full width; row 1 alone holds 4097: refused with its count
    const ScoreRowsShape s = shape(3, 3000, 1090, 6);
    {
        Vec nc = {10, 2999, 3000}, ts = {1090, 1090, 0};
        const Run r = run(s, &nc, &ts);
        CHECK(r.f == SCR_TOO_LONG && r.row == 1 && r.value == 4097);
        nc[1] = 2998;  // 4096: the longest row the model takes
        const Run ok = run(s, &nc, &ts);
        CHECK(ok.f == SCR_OK && ok.R.L[1] == 4096 && ok.R.L[2] == 1 + 3000 + 6 + 0 + 1);
        const Run full = run(s, nullptr, nullptr);
        CHECK(full.f == SCR_TOO_LONG && full.row == 0 && full.value == 4098);
    }
    // no condition: n_cond is refused with row 0 and its value, n_semantic alone is planned with an empty prompt
    {
        const ScoreRowsShape none = shape(2, 0, 7, 4);
        Vec nc = {5, 1}, ts = {0, 7};
        const Run r = run(none, &nc, &ts);
        CHECK(r.f == SCR_COND_WITHOUT && r.row == 0 && r.value == 5);
        const Run ok = run(none, nullptr, &ts);
        CHECK(ok.f == SCR_OK && ok.R.Lp_max == 0 && ok.R.Lp[0] == 0 && ok.R.Lp[1] == 0 && ok.R.Lt[0] == 5 && ok.R.Lt[1] == 12 && !ok.R.uniform);
        if (check_plan(none, nullptr, &ts)) return 1;
    }
    // the speech form is what it was: the field defaults to it
    {
        ScoreRowsShape sp;
        sp.B = 1; sp.nm_max = 4; sp.T_max = 3; sp.G = 2;
        Run r;
        r.f = plan_score_rows(nullptr, nullptr, nullptr, sp, &r.R, &r.row, &r.value);
        CHECK(!sp.cond_form && r.f == SCR_OK && r.R.Lp[0] == 1 + 1 + 4 && r.R.Lt[0] == 2 + 3 + 2);
    }
    return 0;
}

int main() {
    if (check_batches() || check_too_long_and_no_condition()) return 1;
    std::printf("lm_cond_rows_selftest: ok\n");
    return 0;
}
