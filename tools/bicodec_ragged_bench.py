#!/usr/bin/env python
"""BiCodec ragged-batch micro-benchmark at the published size (SPEC_BICODEC / SPEC_BICODEC_ENCODER behind the XLSR-53 front-end
SPEC_XLSR53_BICODEC, seeded weights): N clips (seeded) whose lengths are spread over 2 - 10 s (100 - 500 semantic tokens of 320 samples,
every length distinct up to N = 401), resident on the device.

  ragged     ONE BiCodecTokenizer.tokenize(wav, lengths=...) - one normalisation, one front-end call, one codec call - and ONE
             detokenize(global, semantic, lengths=token_frames(lengths)) over all N clips
  grouped    one tokenize + one detokenize per DISTINCT length (what a caller did before per-clip lengths existed)

Argument 1: N (default 32).  Each figure is the median (min - max) of REPS runs (argument 2, default 5) after one warm-up run, wall clock
around a device synchronisation.  The two forms are compared with torch.equal on every clip's valid part (tokens, waveform) and on what
lies behind it (-1, zeros).  `padded_share` is the part of the ragged call's rows that lie behind a clip's end: every launch of a ragged
call is rectangular at the longest length.  One JSON line per figure is appended to profiles/bicodec_ragged_bench.jsonl (argument 3:
another path)."""
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
from unified_audio_amd.ssl import SPEC_XLSR53_BICODEC  # noqa: E402

N_CLIPS = int(sys.argv[1]) if len(sys.argv) > 1 else 32
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
OUT = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "bicodec_ragged_bench.jsonl")
TOKENS = (100, 500)  # 2 s .. 10 s at 50 semantic tokens per second
HOP = 320
dev = torch.device("cuda:0")
espec, dspec = qa.SPEC_BICODEC_ENCODER, qa.SPEC_BICODEC
sd = synth.bicodec_state_dict(3, dspec)
sd.update(synth.bicodec_encoder_state_dict(4, espec))
sd.update(synth.bicodec_speaker_state_dict(5, espec))
model = qa.BiCodec(dspec, device=dev, encoder_spec=espec, check_tokens=False).load_state_dict(sd)
fx = qa.SSLFeatureExtractor(SPEC_XLSR53_BICODEC, device=dev).load_state_dict(synth.ssl_state_dict(SPEC_XLSR53_BICODEC, 21))
tok = qa.BiCodecTokenizer(model=model, feature_extractor=fx)
tokens = [round(TOKENS[0] + (TOKENS[1] - TOKENS[0]) * i / max(N_CLIPS - 1, 1)) for i in range(N_CLIPS)]
tokens = [tokens[i] for i in torch.randperm(N_CLIPS, generator=torch.Generator().manual_seed(7)).tolist()]  # a file list is not sorted
lens = [t * HOP + 80 for t in tokens]  # 400 samples make the first frame, 320 each further one: t frames, and not a multiple of the hop
assert tok.token_frames(lens) == tokens
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
    row = dict(bench="bicodec_ragged", name=name, clips=N_CLIPS, ms_median=round(ms[0], 3), ms_min=round(ms[1], 3), ms_max=round(ms[2], 3),
               reps=REPS, **kw)
    rows.append(row)
    print(json.dumps(row), flush=True)


def ratio(name, ms_g, ms_r, **kw):
    row = dict(bench="bicodec_ragged", name=name, clips=N_CLIPS, ratio_of_medians=round(ms_g[0] / ms_r[0], 2), ratio_min=round(ms_g[1] / ms_r[2], 2),
               ratio_max=round(ms_g[2] / ms_r[1], 2), distinct_lengths=len(distinct), **kw)
    rows.append(row)
    print(json.dumps(row), flush=True)


def tokenize_ragged():
    return tok.tokenize(wav, lengths=lens)


def tokenize_grouped():
    glob = torch.empty((N_CLIPS, 1, espec.token_num), dtype=torch.int32, device=dev)
    sem = torch.full((N_CLIPS, max(tokens)), -1, dtype=torch.int64, device=dev)
    for n in distinct:
        idx = torch.tensor([b for b, x in enumerate(lens) if x == n], device=dev)
        g, s = tok.tokenize(wav[idx, :n].contiguous())
        glob[idx] = g
        sem[idx, :s.shape[1]] = s
    return glob, sem


def detokenize_ragged(glob, sem):
    return tok.detokenize(glob, sem, lengths=tokens)


def detokenize_grouped(glob, sem):
    out = torch.zeros((N_CLIPS, 1, max(tokens) * HOP), device=dev)
    for t in sorted(set(tokens)):
        idx = torch.tensor([b for b, x in enumerate(tokens) if x == t], device=dev)
        part = tok.detokenize(glob[idx], sem[idx, :t].contiguous())
        out[idx, :, :t * HOP] = part
    return out


audio_s = sum(lens) / 16000.0
padded = round(1.0 - sum(tokens) / (N_CLIPS * max(tokens)), 3)
ms_tr, (gr, sr) = timed(tokenize_ragged)
ms_tg, (gg, sg) = timed(tokenize_grouped)
report("tokenize_ragged", ms_tr, distinct_lengths=len(distinct), seconds_min=min(lens) / 16000, seconds_max=max(lens) / 16000,
       padded_share=padded, audio_s_per_s=round(audio_s / ms_tr[0] * 1e3, 1))
report("tokenize_grouped", ms_tg, distinct_lengths=len(distinct), calls=len(distinct), audio_s_per_s=round(audio_s / ms_tg[0] * 1e3, 1))
ratio("tokenize_grouped_over_ragged", ms_tg, ms_tr, tokens_equal=bool(torch.equal(gr, gg) and torch.equal(sr, sg)))
ms_dr, wr = timed(lambda: detokenize_ragged(gr, sr))
ms_dg, wg = timed(lambda: detokenize_grouped(gr, sr))
report("detokenize_ragged", ms_dr, distinct_lengths=len(distinct), padded_share=padded, audio_s_per_s=round(audio_s / ms_dr[0] * 1e3, 1))
report("detokenize_grouped", ms_dg, distinct_lengths=len(distinct), calls=len(distinct), audio_s_per_s=round(audio_s / ms_dg[0] * 1e3, 1))
ratio("detokenize_grouped_over_ragged", ms_dg, ms_dr, wav_equal=bool(torch.equal(wr, wg)))
both_r = tuple(a + b for a, b in zip(ms_tr, ms_dr))
both_g = tuple(a + b for a, b in zip(ms_tg, ms_dg))
ratio("round_trip_grouped_over_ragged", both_g, both_r, ms_ragged=round(both_r[0], 3), ms_grouped=round(both_g[0], 3))
with open(OUT, "a") as f:
    f.write("== python tools/bicodec_ragged_bench.py " + " ".join(sys.argv[1:]) + "\n")
    for r in rows:
        f.write(json.dumps(r) + "\n")
