#!/usr/bin/env python
"""UniSE LM ragged-batch micro-benchmark at the UniSE width: N TSE segments from N utterances whose enrollments differ in length
(seeded, 2 - 5 s = 100 - 250 feature frames), mix prompt 250 frames, 33 + 250 greedy steps.

  ragged    ONE LLM_SFT.generate(..., enroll_lengths=...) over all N segments
  grouped   one generate per DISTINCT enrollment length (what the driver did before per-row lengths existed)

for N = 16 and N = 64 (arguments 1: a comma list of N).  Each figure is the median (min - max) of REPS runs after one warm-up run, wall
clock around a device synchronisation; the two forms must give the same tokens (reported as tokens_equal).  One JSON line per figure is
appended to profiles/lm_ragged_bench.jsonl (argument 3: another path)."""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import unified_audio_amd as qa  # noqa: E402
from unified_audio_amd import synth as L  # noqa: E402  (seeded weights / features: data generation only)

SIZES = [int(v) for v in sys.argv[1].split(",")] if len(sys.argv) > 1 else [16, 64]
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
OUT = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "lm_ragged_bench.jsonl")
N_MIX, G, S = 250, 32, 250
FRAMES = (100, 250)  # 2 s .. 5 s of enrollment at 50 frames per second
dev = torch.device("cuda:0")
lm = qa.LLM_SFT(device=dev).load_state_dict(L.lm_state_dict(4321))
rows = []


def timed(fn):
    ts, out = [], None
    for _ in range(REPS + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return (statistics.median(ts[1:]), min(ts[1:]), max(ts[1:])), out


def report(name, n, ms, **kw):
    row = dict(bench="lm_ragged", name=name, segments=n, ms_median=round(ms[0], 3), ms_min=round(ms[1], 3), ms_max=round(ms[2], 3), reps=REPS, **kw)
    rows.append(row)
    print(json.dumps(row), flush=True)


for n in SIZES:
    gen = torch.Generator().manual_seed(1000 + n)
    lens = torch.randint(FRAMES[0], FRAMES[1] + 1, (n,), generator=gen).tolist()
    distinct = sorted(set(lens))
    mix = L.synth_feats(50, n, N_MIX).to(dev)
    enr = L.synth_feats(51, n, max(lens)).to(dev)
    for b, v in enumerate(lens):
        enr[b, v:] = 0.0
    mel = torch.zeros(n, S, 80)

    def ragged():
        return lm.generate("tse", mel, enr, mel, mix, do_sample=False, enroll_lengths=lens)

    def grouped():
        g = torch.empty((n, G), dtype=torch.int64, device=dev)
        s = torch.empty((n, S), dtype=torch.int64, device=dev)
        for v in distinct:
            idx = torch.tensor([b for b, x in enumerate(lens) if x == v], device=dev)
            m = torch.zeros(len(idx), S, 80)
            g[idx], s[idx] = lm.generate("tse", m, enr[idx, :v].contiguous(), m, mix[idx].contiguous(), do_sample=False)
        return g, s

    ms_r, (gr, sr) = timed(ragged)
    ms_g, (gg, sg) = timed(grouped)
    same = bool(torch.equal(gr, gg) and torch.equal(sr, sg))
    tok = n * (G + 1 + S)
    report("ragged", n, ms_r, distinct_lengths=len(distinct), frames_min=min(lens), frames_max=max(lens), tok_per_s=round(tok / ms_r[0] * 1e3))
    report("grouped", n, ms_g, distinct_lengths=len(distinct), calls=len(distinct), tok_per_s=round(tok / ms_g[0] * 1e3))
    row = dict(bench="lm_ragged", name="grouped_over_ragged", segments=n, ratio_of_medians=round(ms_g[0] / ms_r[0], 2),
               distinct_lengths=len(distinct), tokens_equal=same,
               note="the launch-bound decode step predicts a ratio near the number of distinct lengths")
    rows.append(row)
    print(json.dumps(row), flush=True)
os.makedirs(os.path.dirname(OUT), exist_ok=True)
with open(OUT, "a") as f:
    for row in rows:
        f.write(json.dumps(row) + "\n")
