#!/usr/bin/env python
"""SSL front-end ragged-batch micro-benchmark at the HuBERT-base size (SPEC_HUBERT_BASE, seeded weights): N clips (seeded) whose lengths
are spread over 2 - 10 s (50 - 250 code frames of 640 samples, every length distinct up to N = 201), resident on the device.

  ssl ragged / grouped        ONE SSLFeatureExtractor(wav, lengths=...) over all N clips, against one call per DISTINCT length scattered
                              into one zero-padded batch (what a caller did before per-clip lengths existed)
  tokenize ragged / grouped   HCodecTokenizer.tokenize(wav, lengths=...) without feats at the SPEC_10 size: one front-end call in front
                              of the ragged encode, against the loop over distinct lengths in front of the same encode

Argument 1: N (default 32).  Each figure is the median (min - max) of REPS runs (argument 2, default 5) after one warm-up run, wall clock
around a device synchronisation.  The two forms are compared with torch.equal (features: on every clip's valid frames and the zeros behind
them; codes: whole tensors).  One JSON line per figure is appended to profiles/ssl_ragged_bench.jsonl (argument 3: another path)."""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import unified_audio_amd as qa  # noqa: E402
from unified_audio_amd import synth  # noqa: E402  (seeded weights / inputs: data generation only)

N_CLIPS = int(sys.argv[1]) if len(sys.argv) > 1 else 32
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
OUT = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "ssl_ragged_bench.jsonl")
FRAMES = (50, 250)  # 2 s .. 10 s at 25 code frames per second
HOP = 640
dev = torch.device("cuda:0")
fx = qa.SSLFeatureExtractor(qa.SPEC_HUBERT_BASE, device=dev).load_state_dict(synth.ssl_state_dict(qa.SPEC_HUBERT_BASE, 21))
tok = qa.HCodecTokenizer(state_dict=synth.hcodec10_state_dict(1234), feature_extractor=fx, device=dev, spec=qa.SPEC_10)
tok.model.check_codes = False
frames = [round(FRAMES[0] + (FRAMES[1] - FRAMES[0]) * i / max(N_CLIPS - 1, 1)) for i in range(N_CLIPS)]
frames = [frames[i] for i in torch.randperm(N_CLIPS, generator=torch.Generator().manual_seed(7)).tolist()]  # a file list is not sorted
lens = [f * HOP for f in frames]
distinct = sorted(set(lens))
wav = synth.synth_wav(11, N_CLIPS, max(lens)).to(dev)
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


def report(name, ms, **kw):
    row = dict(bench="ssl_ragged", name=name, clips=N_CLIPS, ms_median=round(ms[0], 3), ms_min=round(ms[1], 3), ms_max=round(ms[2], 3),
               reps=REPS, **kw)
    rows.append(row)
    print(json.dumps(row), flush=True)


def ratio(name, ms_g, ms_r, **kw):
    row = dict(bench="ssl_ragged", name=name, clips=N_CLIPS, ratio_of_medians=round(ms_g[0] / ms_r[0], 2), ratio_min=round(ms_g[1] / ms_r[2], 2),
               ratio_max=round(ms_g[2] / ms_r[1], 2), distinct_lengths=len(distinct), **kw)
    rows.append(row)
    print(json.dumps(row), flush=True)


def ssl_ragged():
    return fx(wav, lengths=lens)


def ssl_grouped():
    out = torch.zeros((N_CLIPS, fx.frames(max(lens)), fx.spec.hidden_size), device=dev)
    for n in distinct:
        idx = torch.tensor([b for b, x in enumerate(lens) if x == n], device=dev)
        part = fx(wav[idx, :n].contiguous())
        out[idx, :part.shape[1]] = part
    return out


def tokenize_ragged():
    return tok.tokenize(wav, lengths=lens)


def tokenize_grouped():
    tok._ragged_front_end = lambda: False  # the loop over distinct lengths, as for any other front-end
    try:
        return tok.tokenize(wav, lengths=lens)
    finally:
        del tok._ragged_front_end


audio_s = sum(lens) / 16000.0
ms_r, fr = timed(ssl_ragged)
ms_g, fg = timed(ssl_grouped)
report("ssl_ragged", ms_r, distinct_lengths=len(distinct), seconds_min=min(lens) / 16000, seconds_max=max(lens) / 16000,
       audio_s_per_s=round(audio_s / ms_r[0] * 1e3, 1))
report("ssl_grouped", ms_g, distinct_lengths=len(distinct), calls=len(distinct), audio_s_per_s=round(audio_s / ms_g[0] * 1e3, 1))
ratio("ssl_grouped_over_ragged", ms_g, ms_r, feats_equal=bool(torch.equal(fr, fg)))
ms_tr, (ar, sr) = timed(tokenize_ragged)
ms_tg, (ag, sg) = timed(tokenize_grouped)
report("tokenize_ragged", ms_tr, distinct_lengths=len(distinct), front_end_calls=1, audio_s_per_s=round(audio_s / ms_tr[0] * 1e3, 1))
report("tokenize_grouped", ms_tg, distinct_lengths=len(distinct), front_end_calls=len(distinct), audio_s_per_s=round(audio_s / ms_tg[0] * 1e3, 1))
ratio("tokenize_grouped_over_ragged", ms_tg, ms_tr, codes_equal=bool(torch.equal(ar, ag) and torch.equal(sr, sg)))
with open(OUT, "a") as f:
    f.write("== python tools/ssl_ragged_bench.py " + " ".join(sys.argv[1:]) + "\n")
    for r in rows:
        f.write(json.dumps(r) + "\n")
