#!/usr/bin/env python
"""UniSE condition path with per-row lengths at the UniSE width (Conformer 6 x 512, LM 12 x 512): N clips of
2 - 5 s (seeded, any sample count), log-mel -> condition encoder -> CustomLlamaModel.generate with 32 global + 250 semantic greedy steps.

  ragged    ONE pass over all N clips: stft_logmel(lengths=samples), then generate(cond_lengths=frames)
  grouped   one pass per DISTINCT frame count - the only form there was before per-row lengths - each clip's log-mel computed alone
            (a log-mel row of a batch is not the short clip's log-mel), the clips of one frame count stacked for encoder + generate

for N = 16 and N = 64 (argument 1: a comma list of N).  Each figure is the median (min - max) of REPS runs after one warm-up run, host
clock around a device synchronisation; `encoder_ms` is the log-mel + encoder share of the ragged pass, timed the same way on its own.
The two forms' tokens are compared (tokens_equal; a row alone in a narrower batch is the same row bit for bit).  One JSON line per figure
is appended to profiles/lm_cond_ragged_bench.jsonl (argument 3: another path)."""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import unified_audio_amd as qa  # noqa: E402
from unified_audio_amd import synth, unise  # noqa: E402  (seeded weights / waveforms: data generation only)

SIZES = [int(v) for v in sys.argv[1].split(",")] if len(sys.argv) > 1 else [16, 64]
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
OUT = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "lm_cond_ragged_bench.jsonl")
G, S = 32, 250
SAMPLES = (32000, 80000)  # 2 s .. 5 s at 16 kHz
CF = synth.CONFORMER_PARAMS_UNISE
dev = torch.device("cuda:0")
sd = {k: v for k, v in synth.lm_state_dict(3).items() if not k.startswith(("task_embedding", "enroll_sos", "adapter"))}
sd.update(synth.cond_encoder_state_dict(4, 80, 512, CF, gain=2.0))
m = qa.CustomLlamaModel(cond_dim=80, hidden_size=512, num_layers=12, num_attention_heads=8, conformer_params=CF, device=dev).load_state_dict(sd)
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
    row = dict(bench="lm_cond_ragged", name=name, clips=n, ms_median=round(ms[0], 3), ms_min=round(ms[1], 3), ms_max=round(ms[2], 3), reps=REPS, **kw)
    rows.append(row)
    print(json.dumps(row), flush=True)


for n in SIZES:
    gen = torch.Generator().manual_seed(2000 + n)
    samples = torch.randint(SAMPLES[0], SAMPLES[1] + 1, (n,), generator=gen).tolist()
    frames = [unise.mel_frames(v) for v in samples]
    distinct = sorted(set(frames))
    wav = synth.synth_wav(5, n, max(samples)).to(dev)
    for b, v in enumerate(samples):
        wav[b, v:] = 0.0

    def front():
        return m.encode_condition(unise.stft_logmel(wav, lengths=samples), frames)

    def ragged():
        return m.generate(unise.stft_logmel(wav, lengths=samples), global_length=G, semantic_length=S, do_sample=False, cond_lengths=frames)

    def grouped():
        g = torch.empty((n, G), dtype=torch.int64, device=dev)
        s = torch.empty((n, S), dtype=torch.int64, device=dev)
        for f in distinct:
            idx = [b for b, x in enumerate(frames) if x == f]
            mel = torch.cat([unise.stft_logmel(wav[b:b + 1, :samples[b]].contiguous()) for b in idx])
            g[idx], s[idx] = m.generate(mel, global_length=G, semantic_length=S, do_sample=False)
        return g, s

    ms_f, _ = timed(front)
    ms_r, (gr, sr) = timed(ragged)
    ms_g, (gg, sg) = timed(grouped)
    same = bool(torch.equal(gr, gg) and torch.equal(sr, sg))
    agree = float(((gr == gg).float().mean() + (sr == sg).float().mean()) / 2)
    tok = n * (G + S)
    report("ragged", n, ms_r, distinct_frame_counts=len(distinct), frames_min=min(frames), frames_max=max(frames), encoder_ms=round(ms_f[0], 3),
           encoder_share=round(ms_f[0] / ms_r[0], 4), tok_per_s=round(tok / ms_r[0] * 1e3))
    report("grouped", n, ms_g, distinct_frame_counts=len(distinct), calls=len(distinct), tok_per_s=round(tok / ms_g[0] * 1e3))
    row = dict(bench="lm_cond_ragged", name="grouped_over_ragged", clips=n, ratio_of_medians=round(ms_g[0] / ms_r[0], 2),
               distinct_frame_counts=len(distinct), tokens_equal=same, token_agreement=round(agree, 5))
    rows.append(row)
    print(json.dumps(row), flush=True)
os.makedirs(os.path.dirname(OUT), exist_ok=True)
with open(OUT, "a") as f:
    for row in rows:
        f.write(json.dumps(row) + "\n")
