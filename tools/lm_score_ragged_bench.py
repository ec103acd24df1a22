#!/usr/bin/env python
"""UniSE LM teacher-forced scoring over rows of different lengths, at the UniSE width: N TSE rows whose mixtures last 2 - 5 s (seeded,
100 - 250 feature frames; T_b = nm_b semantic targets, 32 global ids) with enrollments of 100 - 250 frames.

  ragged    ONE LLM_SFT.score(..., mix_lengths=, semantic_lengths=, enroll_lengths=) over all N rows (qa_lm_score_ragged)
  grouped   one rectangular score call per DISTINCT length triple, on the trimmed rows (what a caller did before per-row lengths existed)
  padded    the ONE rectangular call over the padded tensors (what the reference's forward does: the padding is scored like any frame)

for N = 16 and N = 64 (argument 1: a comma list of N).  Each figure is the median (min - max) of REPS runs (argument 2, default 5) after
one warm-up run, HIP events around the calls.  While timing, every row's loss and correct count of `ragged` must equal `grouped`'s bit for
bit (asserted).  One JSON line per figure is appended to profiles/lm_score_ragged_bench.jsonl (argument 3: another path)."""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import unified_audio_amd as qa  # noqa: E402
from unified_audio_amd import synth as L  # noqa: E402  (seeded weights / features: data generation only)

SIZES = [int(v) for v in sys.argv[1].split(",")] if len(sys.argv) > 1 else [16, 64]
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
OUT = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "lm_score_ragged_bench.jsonl")
G = 32
FRAMES = (100, 250)  # 2 s .. 5 s at 50 frames per second
dev = torch.device("cuda:0")
lm = qa.LLM_SFT(device=dev).load_state_dict(L.lm_state_dict(4321))
rows = []


def timed(fn):
    ms, out = [], None
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for _ in range(REPS + 1):
        torch.cuda.synchronize()
        ev[0].record()
        out = fn()
        ev[1].record()
        torch.cuda.synchronize()
        ms.append(ev[0].elapsed_time(ev[1]))
    return (statistics.median(ms[1:]), min(ms[1:]), max(ms[1:])), out


def report(name, n, ms, **kw):
    row = dict(bench="lm_score_ragged", name=name, rows=n, ms_median=round(ms[0], 3), ms_min=round(ms[1], 3), ms_max=round(ms[2], 3), reps=REPS, **kw)
    rows.append(row)
    print(json.dumps(row), flush=True)


for n in SIZES:
    gen = torch.Generator().manual_seed(2000 + n)
    nm = torch.randint(FRAMES[0], FRAMES[1] + 1, (n,), generator=gen).tolist()
    ne = torch.randint(FRAMES[0], FRAMES[1] + 1, (n,), generator=gen).tolist()
    T = list(nm)
    mix = L.synth_feats(60, n, max(nm)).to(dev)
    enr = L.synth_feats(61, n, max(ne)).to(dev)
    g = torch.randint(0, 4096, (n, G), generator=gen).to(dev)
    s = torch.randint(0, 8192, (n, max(T)), generator=gen).to(dev)
    mel = torch.zeros(n, 1, 80)
    triples = {}
    for b in range(n):
        triples.setdefault((ne[b], nm[b], T[b]), []).append(b)

    def ragged():
        return lm.score("tse", mel, enr, mel, mix, g, s, mix_lengths=nm, semantic_lengths=T, enroll_lengths=ne)

    def grouped():
        loss = torch.empty(n, dtype=torch.float32, device=dev)
        acc = torch.empty(n, dtype=torch.float32, device=dev)
        for (e, m, t), idx in triples.items():
            i = torch.tensor(idx, device=dev)
            one = torch.zeros(len(idx), 1, 80)
            lo, ac = lm.score("tse", one, enr[i, :e].contiguous(), one, mix[i, :m].contiguous(), g[i], s[i, :t].contiguous())
            loss[i], acc[i] = lo, ac
        return loss, acc

    def padded():
        return lm.score("tse", mel, enr, mel, mix, g, s)

    t_r, out_r = timed(ragged)
    t_g, out_g = timed(grouped)
    t_p, _ = timed(padded)
    assert torch.equal(out_r[0], out_g[0]) and torch.equal(out_r[1], out_g[1]), "a row of the ragged call differs from its rectangular call"
    lt = [G + t + 2 for t in T]
    pos = [1 + 1 + e + 1 + m + k for e, m, k in zip(ne, nm, lt)]
    lt_max, pos_max = G + max(T) + 2, 3 + max(ne) + max(nm) + G + max(T) + 2
    common = dict(distinct_triples=len(triples), target_rows=sum(lt), target_rows_padded=n * lt_max, positions=sum(pos),
                  positions_padded=n * pos_max)
    report("ragged", n, t_r, rows_equal_grouped=True, **common)
    report("grouped", n, t_g, calls=len(triples), **common)
    report("padded", n, t_p, **common)

with open(OUT, "a") as f:
    for row in rows:
        f.write(json.dumps(row) + "\n")
