"""TEST INFRASTRUCTURE ONLY - the truth of a teacher-forced score call with per-row lengths (qa_lm_score_ragged):
row b is tests/lm_score_ref.score on that sequence ALONE, on its trimmed inputs - never the ragged code itself.  `padded_logits` is an
independent second formulation (one zero-padded, left-aligned causal batch), which tests/test_lm_score_ragged_cpu.py holds against the
first in float64: the "a causal body needs no mask for left-aligned rows" argument, pinned on the oracle.

THE CASE: R.SMALL, weight seed 91, 'tse', G = 4, eps 0.1, seeded random targets; rows of 133 / 50 / 90 / 265 / 49 / 139 positions - one
that crosses a 128-query block, one that crosses two, rows that end inside the first 32-key tile region of a block, T_b = 0, nm_b = 1
and ne_b = 1."""
from __future__ import annotations

import functools

import torch
import torch.nn.functional as F

from oracle import llm_ref as L
from tests import lm_score_ref as R

CASE_SEED, CASE_G, CASE_EPS = 91, 4, 0.1
CASE_NE = [3, 40, 17, 1, 25, 9]
CASE_NM = [60, 1, 33, 129, 7, 64]
CASE_T = [61, 0, 31, 126, 8, 57]
CASE_POSITIONS = [133, 50, 90, 265, 49, 139]


def positions(ne, nm, T, G, enroll=True):
    """Row b's prompt positions, target rows and their sum."""
    lp = [1 + (1 + e if enroll else 0) + 1 + m for e, m in zip(ne, nm)]
    lt = [G + t + 2 for t in T]
    return lp, lt, [a + b for a, b in zip(lp, lt)]


def case_inputs(spec=R.SMALL, seed=CASE_SEED, ne=CASE_NE, nm=CASE_NM, T=CASE_T, G=CASE_G):
    """(enr [B, max ne, F], mix [B, max nm, F], g int32 [B, G], s int64 [B, max T]) of a case, seeded; padded at the maxima."""
    B = len(nm)
    mix = L.synth_feats(seed + 100, B, max(nm), spec.feats_dim)
    enr = L.synth_feats(seed + 101, B, max(ne), spec.feats_dim)
    gen = torch.Generator().manual_seed(seed + 102)
    g = torch.randint(0, spec.global_size, (B, G), generator=gen, dtype=torch.int32)
    s = torch.randint(0, spec.semantic_size, (B, max(max(T), 1)), generator=gen, dtype=torch.int64)[:, :max(T)]
    return enr, mix, g, s


def score_ragged(sd, spec, task, enr, mix, g, s, ne, nm, T, eps, dtype=torch.float32) -> dict:
    """R.score row by row on trimmed inputs, plus the pooled scalars.  rows: the per-row dicts of R.score (logits [1, Lt_b, V], ...);
    loss_seq / correct [B]; loss = sum of all row KLs / sum Lt_b, acc = sum correct / sum Lt_b (float64 scalars)."""
    rows = []
    for b in range(mix.shape[0]):
        e = None if enr is None else enr[b:b + 1, :ne[b]]
        rows.append(R.score(sd, spec, task, e, mix[b:b + 1, :nm[b]], g[b:b + 1], s[b:b + 1, :T[b]], eps, dtype))
    total = sum(o["targets"].shape[1] for o in rows)
    return dict(rows=rows, loss_seq=torch.cat([o["loss_seq"] for o in rows]), correct=torch.cat([o["correct"] for o in rows]),
                loss=float(sum(o["row_kl"].sum() for o in rows) / total), acc=float(sum(int(o["correct"]) for o in rows)) / total,
                Lt=[o["targets"].shape[1] for o in rows])


@torch.no_grad()
def padded_logits(sd, spec, task, enr, mix, g, s, ne, nm, T, dtype=torch.float64):
    """The second formulation: every row's [prompt, input embeddings] left-aligned in ONE zero-padded batch through the causal body, and
    each row's last Lt_b live rows through the head.  Returns the list of logits [Lt_b, V]."""
    sd = {k: v.to(dtype) for k, v in sd.items()}
    B = mix.shape[0]
    seqs = []
    for b in range(B):
        e = None if enr is None else enr[b:b + 1, :ne[b]].to(dtype)
        inp, _ = R.token_ids(g[b:b + 1], s[b:b + 1, :T[b]], spec)
        seqs.append(torch.cat([L.build_prompt(sd, L.TASK_MAP[task], e, mix[b:b + 1, :nm[b]].to(dtype)), sd["codec_embedding.weight"][inp]], dim=1)[0])
    n = max(x.shape[0] for x in seqs)
    x = torch.zeros(B, n, spec.hidden, dtype=dtype)
    for b, q in enumerate(seqs):
        x[b, :q.shape[0]] = q
    hs = L.llm_forward(sd, x, L.KVCache(spec.n_layers), spec, dtype)
    out = []
    for b, q in enumerate(seqs):
        lt = g.shape[1] + T[b] + 2
        out.append(F.linear(hs[b, q.shape[0] - lt:q.shape[0]], sd["output_head.weight"]))
    return out


@functools.lru_cache(maxsize=None)
def case_oracle(task: str = "tse"):
    """THE CASE's weights, inputs and per-row oracle in fp64 and fp32, computed once and shared (read-only) by the tests that need it."""
    sd = L.lm_state_dict(CASE_SEED, R.SMALL)
    enr, mix, g, s = case_inputs()
    e = enr if task != "se" else None
    o64 = score_ragged(sd, R.SMALL, task, e, mix, g, s, CASE_NE, CASE_NM, CASE_T, CASE_EPS, torch.float64)
    o32 = score_ragged(sd, R.SMALL, task, e, mix, g, s, CASE_NE, CASE_NM, CASE_T, CASE_EPS, torch.float32)
    return sd, (e, mix, g, s), o64, o32
