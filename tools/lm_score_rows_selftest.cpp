// lm_score_rows_selftest.cpp - the host side of per-row lengths on the teacher-forced scoring path (csrc/lm_score_rows.h, DESIGN.md
// section 35) as a stand-alone host program for the host sanitizers: every refusal with the row it names, offsets / maxima / groups
// against a naive recount, and the "is this rectangular" decision.  Every vector lives in an exact-size heap block, so a read past
// either end is a report.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I unified_audio_amd/csrc \
//       tools/lm_score_rows_selftest.cpp -o /tmp/lm_score_rows_selftest && /tmp/lm_score_rows_selftest
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>

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

static ScoreRowsShape shape(int64_t B, bool enroll, int64_t ne_max, int64_t nm_max, int64_t T_max, int G, bool targets = true) {
    ScoreRowsShape s;
    s.B = B; s.has_enroll = enroll; s.ne_max = ne_max; s.nm_max = nm_max; s.T_max = T_max; s.G = G; s.targets = targets;
    return s;
}

struct Run {
    ScoreRows R;
    int64_t row = -1, value = -1;
    ScoreRowsFault f = SCR_OK;
};

// nullptr for an absent vector (`has_*` false), else an exact-size copy
static Run run(const ScoreRowsShape& s, const Vec* ne, const Vec* nm, const Vec* T) {
    Run r;
    auto pe = ne ? exact(*ne) : nullptr;
    auto pm = nm ? exact(*nm) : nullptr;
    auto pt = T ? exact(*T) : nullptr;
    r.f = plan_score_rows(pe.get(), pm.get(), pt.get(), s, &r.R, &r.row, &r.value);
    return r;
}

static int check_refusals() {
    const Vec ne = {3, 5, 1}, nm = {6, 1, 9}, T = {0, 7, 4};
    const ScoreRowsShape s = shape(3, true, 5, 9, 7, 4);
    CHECK(run(s, &ne, &nm, &T).f == SCR_OK);
    {  // n_enroll without an enrollment
        Run r = run(shape(3, false, 0, 9, 7, 4), &ne, &nm, &T);
        CHECK(r.f == SCR_ENROLL_WITHOUT && r.row == 0 && r.value == 3);
    }
    for (int64_t bad : {(int64_t)0, (int64_t)6, (int64_t)-2, INT64_MAX, INT64_MIN}) {
        Vec v = ne;
        v[1] = bad;
        Run r = run(s, &v, &nm, &T);
        CHECK(r.f == SCR_ENROLL_RANGE && r.row == 1 && r.value == bad);
    }
    for (int64_t bad : {(int64_t)0, (int64_t)10, (int64_t)-1, INT64_MAX}) {
        Vec v = nm;
        v[2] = bad;
        Run r = run(s, &ne, &v, &T);
        CHECK(r.f == SCR_MIX_RANGE && r.row == 2 && r.value == bad);
        Run q = run(shape(3, false, 0, 9, 7, 4), nullptr, &v, nullptr);  // the same without the other vectors
        CHECK(q.f == SCR_MIX_RANGE && q.row == 2 && q.value == bad);
    }
    for (int64_t bad : {(int64_t)-1, (int64_t)8, INT64_MAX, INT64_MIN}) {
        Vec v = T;
        v[0] = bad;
        Run r = run(s, &ne, &nm, &v);
        CHECK(r.f == SCR_SEMANTIC_RANGE && r.row == 0 && r.value == bad);
    }
    {  // the first offending row is the one named, whatever follows
        Vec v = {9, 0, 0};
        Run r = run(s, &ne, &v, &T);
        CHECK(r.f == SCR_MIX_RANGE && r.row == 1 && r.value == 0);
    }
    {  // the longest row above max_pos: 1 + (1 + 100) + 1 + 2000 + 32 + 1961 + 2 = 4098 > 4096; one id fewer twice fits
        const Vec e = {100, 100}, m = {2000, 2000}, t = {1959, 1961};
        Run r = run(shape(2, true, 100, 2000, 1961, 32), &e, &m, &t);
        CHECK(r.f == SCR_TOO_LONG && r.row == 1 && r.value == 4098);
        const Vec t2 = {1959, 1959};
        Run ok = run(shape(2, true, 100, 2000, 1961, 32), &e, &m, &t2);
        CHECK(ok.f == SCR_OK && ok.R.L[1] == 4096);
        Run full = run(shape(2, true, 100, 2000, 1961, 32), nullptr, nullptr, nullptr);  // the maxima themselves are checked too
        CHECK(full.f == SCR_TOO_LONG && full.row == 0 && full.value == 4098);
    }
    return 0;
}

static int check_uniform() {
    const Vec ne = {5, 5}, nm = {9, 9}, T = {7, 7};
    const ScoreRowsShape s = shape(2, true, 5, 9, 7, 4);
    CHECK(run(s, &ne, &nm, &T).R.uniform);
    CHECK(run(s, nullptr, &nm, nullptr).R.uniform);
    CHECK(run(s, nullptr, nullptr, nullptr).R.uniform);
    const Vec ne2 = {5, 4}, nm2 = {8, 9}, T2 = {7, 0};
    CHECK(!run(s, &ne2, &nm, &T).R.uniform);
    CHECK(!run(s, &ne, &nm2, &T).R.uniform);
    CHECK(!run(s, &ne, &nm, &T2).R.uniform);
    CHECK(!run(s, nullptr, nullptr, &T2).R.uniform);
    // a prompt-only call ignores the semantic vector's width
    CHECK(run(shape(2, true, 5, 9, 0, 0, false), &ne, &nm, nullptr).R.uniform);
    CHECK(!run(shape(2, true, 5, 9, 0, 0, false), &ne2, &nm, nullptr).R.uniform);
    return 0;
}

// offsets, counts, maxima and groups against a naive recount
static int check_plan(std::mt19937& rng, int B, bool enroll, bool targets, int group_rows) {
    const int ne_max = 1 + (int)(rng() % 40), nm_max = 1 + (int)(rng() % 130), T_max = (int)(rng() % 130), G = (int)(rng() % 6);
    Vec ne(B), nm(B), T(B);
    for (int b = 0; b < B; ++b) {
        ne[b] = 1 + (int64_t)(rng() % ne_max);
        nm[b] = 1 + (int64_t)(rng() % nm_max);
        T[b] = (int64_t)(rng() % (T_max + 1));
    }
    ScoreRowsShape s = shape(B, enroll, enroll ? ne_max : 0, nm_max, T_max, G, targets);
    s.group_rows = group_rows;
    const bool give_T = targets && (rng() & 1);
    Run r = run(s, enroll ? &ne : nullptr, &nm, give_T ? &T : nullptr);
    CHECK(r.f == SCR_OK);
    const ScoreRows& R = r.R;
    CHECK((int)R.L.size() == B && (int)R.off.size() == B);
    CHECK(R.Lp_max == 1 + (enroll ? 1 + ne_max : 0) + 1 + nm_max);
    long long total = 0;
    for (int b = 0; b < B; ++b) {
        const int Tb = targets ? (give_T ? (int)T[b] : T_max) : 0;
        const int Lp = 1 + (enroll ? 1 + (int)ne[b] : 0) + 1 + (int)nm[b];
        const int Lt = targets ? G + Tb + 2 : 0;
        CHECK(R.ne[b] == (enroll ? (int)ne[b] : 0) && R.nm[b] == (int)nm[b] && R.T[b] == Tb);
        CHECK(R.Lp[b] == Lp && R.Lt[b] == Lt && R.L[b] == Lp + Lt);
        CHECK(R.off[b] == total);
        total += Lt;
    }
    CHECK(R.total_rows == total);
    CHECK((int)R.groups.size() == (B + group_rows - 1) / group_rows);
    long long body_max = 0, packed_max = 0;
    int next = 0;
    for (const ScoreGroup& g : R.groups) {
        CHECK(g.b0 == next && g.gb >= 1 && g.gb <= group_rows);
        next += g.gb;
        int n = 0, lt = 0;
        long long rows = 0;
        for (int b = g.b0; b < g.b0 + g.gb; ++b) {
            n = std::max(n, R.L[b]);
            lt = std::max(lt, R.Lt[b]);
            rows += R.Lt[b];
        }
        CHECK(g.n == n && g.Lt_max == lt && g.rows == rows && g.row0 == R.off[g.b0]);
        body_max = std::max(body_max, (long long)g.gb * n);
        packed_max = std::max(packed_max, rows);
    }
    CHECK(next == B);
    CHECK(R.body_rows_max == body_max && R.packed_rows_max == packed_max);
    return 0;
}

int main() {
    if (check_refusals()) return 1;
    if (check_uniform()) return 1;
    std::mt19937 rng(20260);
    for (int it = 0; it < 200; ++it) {
        const int Bs[] = {1, 2, 63, 64, 65, 70, 129};
        const int B = Bs[it % 7];
        if (check_plan(rng, B, (it & 1) != 0, (it % 5) != 0, 64)) return 1;
    }
    if (check_plan(rng, 70, true, true, 64) || check_plan(rng, 1, false, true, 64) || check_plan(rng, 9, true, true, 4)) return 1;
    {  // B = 70: rows 0 .. 63 and 64 .. 69, the second group at its OWN longest row
        Vec nm(70, 5), T(70, 3);
        nm[3] = 100;
        nm[66] = 20;
        Run r = run(shape(70, false, 0, 100, 3, 4), nullptr, &nm, &T);
        CHECK(r.f == SCR_OK && r.R.groups.size() == 2 && r.R.groups[0].gb == 64 && r.R.groups[1].b0 == 64 && r.R.groups[1].gb == 6);
        CHECK(r.R.groups[0].n == 2 + 100 + 9 && r.R.groups[1].n == 2 + 20 + 9 && r.R.groups[1].row0 == 64 * 9 && r.R.groups[1].rows == 6 * 9);
    }
    std::puts("lm_score_rows_selftest: ok");
    return 0;
}
