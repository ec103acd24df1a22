// lm_score_rows.h - the host side of per-row lengths on the teacher-forced scoring path (qa_lm_score_ragged / qa_lm_prompt_ragged,
// DESIGN.md section 35): the checks of the three length vectors, every row's prompt / target / position counts, the packed target-row
// offsets, the groups' own widths and the "is this the rectangular call" decision.  Plain C++ with no device code, so
// tools/lm_score_rows_selftest.cpp runs it under the host sanitizers; lm.cpp turns a refusal into the library's error message.
#pragma once
#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

namespace qa {

// why the length vectors of a score / prompt call are refused (the first offending row and its value go with it)
enum ScoreRowsFault {
    SCR_OK = 0,
    SCR_ENROLL_WITHOUT = 1,  // n_enroll given, but the call has no enrollment
    SCR_ENROLL_RANGE = 2,    // n_enroll[b] outside 1 .. n_enroll_max
    SCR_MIX_RANGE = 3,       // n_mix[b] outside 1 .. n_mix_max
    SCR_SEMANTIC_RANGE = 4,  // n_semantic[b] outside 0 .. semantic_length_max
    SCR_TOO_LONG = 5,        // the row's prompt + target positions exceed max_pos
    SCR_COND_WITHOUT = 6,    // condition form: n_cond given, but the call has no condition
};

// what a call looks like before its vectors are read: the maxima are the strides of the caller's tensors
struct ScoreRowsShape {
    int64_t B = 0;
    bool has_enroll = false;
    int64_t ne_max = 0, nm_max = 0, T_max = 0;
    int G = 0;
    bool targets = true;  // false: a prompt-only call (qa_lm_prompt_ragged) - no target rows, T is ignored
    int group_rows = 64;  // sequences per pass of the body (LM_MAX_ROWS)
    int max_pos = 4096;   // max_position_embeddings
    // CustomLlamaModel.forward (qa_lm_score_cond_ragged): the prompt is [mix_sos, cond[b, :n]] - n_mix / nm_max carry the
    // rows' condition frames and T_max their width - or NOTHING (nm_max = 0), there is no enrollment, and the last position of a row's OWN
    // stream is dropped: Lt = G + T + 1, no eos target
    bool cond_form = false;
};

// sequences [b0, b0 + gb) go through the body together, laid out at the group's OWN longest row
struct ScoreGroup {
    int b0 = 0, gb = 0;
    int n = 0;           // positions of the group's longest row: the group's width
    int Lt_max = 0;      // target rows of the group's longest target stream
    long long row0 = 0;  // packed target rows in front of the group (in the call)
    long long rows = 0;  // packed target rows of the group: the sum of its Lt
};

struct ScoreRows {
    std::vector<int> ne, nm, T;       // [B] the rows' own counts (ne all 0 without an enrollment, T all 0 without targets)
    std::vector<int> Lp, Lt, L;       // [B] prompt positions, target rows, Lp + Lt
    std::vector<long long> off;       // [B] packed target-row offset: the exclusive prefix sum of Lt over the call
    long long total_rows = 0;         // the sum of Lt
    int Lp_max = 0;                   // the prompt at the tensors' widths: the row stride of qa_lm_prompt_ragged's output
    std::vector<ScoreGroup> groups;
    long long body_rows_max = 0;      // max over the groups of gb * n: the rows the body's buffers must hold
    long long packed_rows_max = 0;    // max over the groups of `rows`
    bool uniform = true;              // every given vector is at full width: the call IS the rectangular one
};

// The three HOST vectors (each nullptr = every row at full width) against the shape.  On a fault *row / *value name the first offending
// row and what it holds (SCR_TOO_LONG: its position count; SCR_ENROLL_WITHOUT: row 0 and n_enroll[0]).  On SCR_OK *out is filled.
inline ScoreRowsFault plan_score_rows(const int64_t* n_enroll, const int64_t* n_mix, const int64_t* n_semantic, const ScoreRowsShape& s,
                                      ScoreRows* out, int64_t* row, int64_t* value) {
    *row = 0;
    *value = 0;
    if (n_enroll && !s.has_enroll) {
        *value = s.B > 0 ? n_enroll[0] : 0;
        return SCR_ENROLL_WITHOUT;
    }
    const bool no_cond = s.cond_form && s.nm_max <= 0;
    if (n_mix && no_cond) {
        *value = s.B > 0 ? n_mix[0] : 0;
        return SCR_COND_WITHOUT;
    }
    const size_t B = (size_t)std::max<int64_t>(s.B, 0);
    ScoreRows r;
    r.ne.assign(B, 0);
    r.nm.assign(B, 0);
    r.T.assign(B, 0);
    r.Lp.assign(B, 0);
    r.Lt.assign(B, 0);
    r.L.assign(B, 0);
    r.off.assign(B, 0);
    r.Lp_max = s.cond_form ? (int)(no_cond ? 0 : 1 + s.nm_max) : (int)(1 + (s.has_enroll ? 1 + s.ne_max : 0) + 1 + s.nm_max);
    for (size_t b = 0; b < B; ++b) {
        *row = (int64_t)b;
        const int64_t ne = s.has_enroll ? (n_enroll ? n_enroll[b] : s.ne_max) : 0;
        const int64_t nm = no_cond ? 0 : n_mix ? n_mix[b] : s.nm_max;
        const int64_t T = s.targets ? (n_semantic ? n_semantic[b] : s.T_max) : 0;
        if (s.has_enroll && (ne < 1 || ne > s.ne_max)) {
            *value = ne;
            return SCR_ENROLL_RANGE;
        }
        if (!no_cond && (nm < 1 || nm > s.nm_max)) {
            *value = nm;
            return SCR_MIX_RANGE;
        }
        if (T < 0 || T > s.T_max) {
            *value = T;
            return SCR_SEMANTIC_RANGE;
        }
        // every term is bounded by its checked maximum, so the sum cannot overflow once the maxima are sane (lm.cpp checks them)
        const int64_t Lp = s.cond_form ? (no_cond ? 0 : 1 + nm) : 1 + (s.has_enroll ? 1 + ne : 0) + 1 + nm;
        const int64_t Lt = s.targets ? (int64_t)s.G + T + (s.cond_form ? 1 : 2) : 0;
        if (Lp + Lt > s.max_pos) {
            *value = Lp + Lt;
            return SCR_TOO_LONG;
        }
        r.ne[b] = (int)ne;
        r.nm[b] = (int)nm;
        r.T[b] = (int)T;
        r.Lp[b] = (int)Lp;
        r.Lt[b] = (int)Lt;
        r.L[b] = (int)(Lp + Lt);
        r.off[b] = r.total_rows;
        r.total_rows += Lt;
        if ((s.has_enroll && ne != s.ne_max) || nm != s.nm_max || (s.targets && T != s.T_max)) r.uniform = false;
    }
    *row = 0;
    const int step = std::max(1, s.group_rows);
    for (size_t b0 = 0; b0 < B; b0 += (size_t)step) {
        ScoreGroup g;
        g.b0 = (int)b0;
        g.gb = (int)std::min<size_t>((size_t)step, B - b0);
        g.row0 = r.off[b0];
        for (int i = 0; i < g.gb; ++i) {
            g.n = std::max(g.n, r.L[b0 + i]);
            g.Lt_max = std::max(g.Lt_max, r.Lt[b0 + i]);
            g.rows += r.Lt[b0 + i];
        }
        r.body_rows_max = std::max(r.body_rows_max, (long long)g.gb * g.n);
        r.packed_rows_max = std::max(r.packed_rows_max, g.rows);
        r.groups.push_back(g);
    }
    *out = std::move(r);
    return SCR_OK;
}

}  // namespace qa
