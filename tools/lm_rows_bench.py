#!/usr/bin/env python
"""UniSE LM with per-row mixture and semantic lengths, at the UniSE width, SE prompt, 33 global steps: N segments
whose mixtures last 1 - 5 s (seeded, in steps of 0.5 s: 50 .. 250 feature frames and as many semantic steps).

  ragged    ONE LLM_SFT.generate(..., mix_lengths=, semantic_lengths=) over all N segments
  padded    the rectangle: every row at 5 s (250 frames, 250 steps) - what the driver's wrap-padding pays today
  grouped   one rectangular generate per DISTINCT length

for N = 16 and N = 64 (argument 1: a comma list of N), then UniSE.enhance with tail="trim" against tail="wrap" on 64 utterances of 1 - 7 s
(seeded weights at the published sizes; argument 4 = 0 skips it).  Every comparison runs in this one process with its forms ALTERNATED
run by run (ragged, padded, grouped, ragged, ...), REPS runs each (argument 2) after one warm-up round, wall clock around a device
synchronisation.  Figures: ms per call as median (min - max) and USEFUL tokens per second - the 33 + n_semantic[b] steps a row asked for,
whatever the form computed.  ragged and grouped must give the same tokens over every row's own columns (tokens_equal).  One JSON line per
figure is appended to profiles/lm_rows_bench.jsonl (argument 3: another path)."""
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
from unified_audio_amd import unise as U  # noqa: E402

SIZES = [int(v) for v in sys.argv[1].split(",")] if len(sys.argv) > 1 else [16, 64]
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
OUT = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "lm_rows_bench.jsonl")
DRIVER = (int(sys.argv[4]) if len(sys.argv) > 4 else 1) != 0
G, FULL = 32, 250
dev = torch.device("cuda:0")
lm = qa.LLM_SFT(device=dev).load_state_dict(L.lm_state_dict(4321))
rows = []


def alternated(forms):
    """{name: fn} -> {name: ((median, min, max) ms, last output)}: one warm-up round, then REPS rounds, the forms in turn inside a round"""
    ts, out = {k: [] for k in forms}, {}
    for it in range(REPS + 1):
        for name, fn in forms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out[name] = fn()
            torch.cuda.synchronize()
            if it:
                ts[name].append((time.perf_counter() - t0) * 1e3)
    return {k: ((statistics.median(v), min(v), max(v)), out[k]) for k, v in ts.items()}


def report(bench, name, n, ms, **kw):
    row = dict(bench=bench, name=name, rows=n, ms_median=round(ms[0], 3), ms_min=round(ms[1], 3), ms_max=round(ms[2], 3), reps=REPS, **kw)
    rows.append(row)
    print(json.dumps(row), flush=True)


for n in SIZES:
    gen = torch.Generator().manual_seed(2000 + n)
    lens = (torch.randint(2, 11, (n,), generator=gen) * 25).tolist()  # 1.0 .. 5.0 s in steps of 0.5 s, 50 frames and 50 steps per second
    lens[0] = FULL  # the tensors' widths are the rectangle's whatever the draw
    distinct = sorted(set(lens))
    mix = L.synth_feats(50, n, FULL).to(dev)
    mel = torch.zeros(n, FULL, 80)

    def ragged():
        return lm.generate("se", None, None, mel, mix, do_sample=False, mix_lengths=lens, semantic_lengths=lens)

    def padded():
        return lm.generate("se", None, None, mel, mix, do_sample=False)

    def grouped():
        g = torch.empty((n, G), dtype=torch.int64, device=dev)
        s = torch.full((n, FULL), -1, dtype=torch.int64, device=dev)
        for v in distinct:
            idx = torch.tensor([b for b, x in enumerate(lens) if x == v], device=dev)
            g[idx], s[idx, :v] = lm.generate("se", None, None, torch.zeros(len(idx), v, 80), mix[idx, :v].contiguous(), do_sample=False)
        return g, s

    res = alternated(dict(ragged=ragged, padded=padded, grouped=grouped))
    useful = sum(G + 1 + v for v in lens)
    (gr, sr), (gg, sg) = res["ragged"][1], res["grouped"][1]
    same = bool(torch.equal(gr, gg) and torch.equal(sr, sg))
    steps_saved = 1.0 - (G + 1 + max(lens)) / (G + 1 + FULL)
    for name in ("ragged", "padded", "grouped"):
        ms = res[name][0]
        report("lm_rows", name, n, ms, useful_tokens=useful, useful_tok_per_s=round(useful / ms[0] * 1e3), distinct_lengths=len(distinct),
               frames_min=min(lens), frames_mean=round(sum(lens) / n, 1), calls=len(distinct) if name == "grouped" else 1)
    row = dict(bench="lm_rows", name="ratios", rows=n, padded_over_ragged=round(res["padded"][0][0] / res["ragged"][0][0], 3),
               grouped_over_ragged=round(res["grouped"][0][0] / res["ragged"][0][0], 3), tokens_equal=same,
               useful_over_padded_tokens=round(useful / (n * (G + 1 + FULL)), 3), chain_steps_saved=round(steps_saved, 3),
               note="one chain of <= 64 rows runs for its LONGEST row: a batch holding one 5 s row saves K/V traffic and no step")
    rows.append(row)
    print(json.dumps(row), flush=True)

if DRIVER:
    fx = qa.SSLFeatureExtractor(qa.SPEC_WAVLM_BASE_PLUS, device=dev).load_state_dict(L.ssl_state_dict(qa.SPEC_WAVLM_BASE_PLUS))
    bic = qa.BiCodec(device=dev).load_state_dict(L.bicodec_state_dict(77))
    tok = qa.BiCodecTokenizer(model=bic)
    drivers = {t: U.UniSE(lm, fx, tokenizer=tok, tail=t) for t in ("wrap", "trim")}
    gen = torch.Generator().manual_seed(3000)
    n_utt = 64
    samples = torch.randint(16000, 7 * 16000 + 1, (n_utt,), generator=gen).tolist()
    srcs = [(torch.randn(1, t, generator=gen) * 0.1).to(dev) for t in samples]
    res = alternated({t: (lambda d=d: d.enhance("se", srcs)) for t, d in drivers.items()})
    audio_s = sum(samples) / 16000
    for t in ("wrap", "trim"):
        ms = res[t][0]
        segs = sum(len(U.trim_samples(v)) if t == "trim" else -(-v // U.SEG_LEN) for v in samples)
        steps = sum(U.mel_frames(v) for u in samples for v in U.trim_samples(u)) if t == "trim" else segs * FULL
        report("unise_tail", t, n_utt, ms, segments=segs, semantic_steps=steps, audio_s=round(audio_s, 1),
               audio_s_per_s=round(audio_s / ms[0] * 1e3, 1), lengths_ok=all(o.numel() == v for o, v in zip(res[t][1], samples)))
    row = dict(bench="unise_tail", name="ratios", rows=n_utt, wrap_over_trim=round(res["wrap"][0][0] / res["trim"][0][0], 3))
    rows.append(row)
    print(json.dumps(row), flush=True)

os.makedirs(os.path.dirname(OUT), exist_ok=True)
with open(OUT, "a") as f:
    for row in rows:
        f.write(json.dumps(row) + "\n")
