#!/usr/bin/env python
"""H-Codec ragged-batch micro-benchmark at the SPEC_10 size (or, with --model 1.5, SPEC_15): N clips (seeded) whose lengths are spread
over 2 - 10 s (50 - 250 code frames), resident on the device, features given.

  ragged    ONE Codec.encode(..., lengths=...) + ONE Codec.decode(..., lengths=...) over all N clips (1.5: encode_ragged + decode_ragged)
  grouped   one encode + decode per DISTINCT length (what a caller did before per-clip lengths existed)

--model 1.5 (anywhere on the command line; the default is 1.0): the adaptive codec, appended to profiles/hcodec15_ragged_bench.jsonl.  A
grouped 1.5 call holds the clips of ONE length; with every length distinct that is B = 1, the call a per-clip row is defined to equal, so
the two forms must agree bit for bit on every clip's valid part once the grouped encode takes the unfused stage 0 (QA_SEANET_FUSED=0,
set here for the grouped 1.5 encode): the run fails if they do not.

--model 2.0: H-Codec 2.0 at full depth (SPEC_20, 48 kHz, 12.5 code frames per second), lengths spread over 2 - 30 s (25 - 375 code
frames), ONE Codec.encode_ragged + ONE Codec.decode_ragged against one rectangular call per distinct length, appended to
profiles/hcodec20_ragged_bench.jsonl.  2.0 has no fused stage 0 and a row of a per-clip call is the rectangular call on that clip alone,
so the two forms must agree bit for bit on every clip's valid part: the run fails if they do not.  N defaults to 16 there.

Argument 1: N (default 32).  Each figure is the median (min - max) of REPS runs (argument 2, default 5) after one warm-up run, wall clock
around a device synchronisation; the two forms are compared on the valid part of every clip (codes_equal, wav_equal: the grouped calls
take the fused stage 0, so equality of the codes is expected but not guaranteed, and the waveforms are decoded from each form's own
codes).  One JSON line per figure is appended to profiles/hcodec_ragged_bench.jsonl (argument 3: another path)."""
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

ARGV = sys.argv[1:]
MODEL = "1.0"
if "--model" in ARGV:
    i = ARGV.index("--model")
    MODEL = ARGV[i + 1]
    del ARGV[i:i + 2]
if MODEL not in ("1.0", "1.5", "2.0"):
    sys.exit(f"--model {MODEL}: 1.0, 1.5 or 2.0")
ADAPTIVE = MODEL == "1.5"
V20 = MODEL == "2.0"
N_CLIPS = int(ARGV[0]) if len(ARGV) > 0 else (16 if V20 else 32)
REPS = int(ARGV[1]) if len(ARGV) > 1 else 5
BENCH = {"1.0": "hcodec_ragged", "1.5": "hcodec15_ragged", "2.0": "hcodec20_ragged"}[MODEL]
OUT = ARGV[2] if len(ARGV) > 2 else os.path.join(ROOT, "profiles", BENCH + "_bench.jsonl")
FRAMES = (25, 375) if V20 else (50, 250)  # 2 s .. 30 s at 12.5 code frames per second; 2 s .. 10 s at 25
SR = 48000.0 if V20 else 16000.0
dev = torch.device("cuda:0")
spec = qa.SPEC_20 if V20 else qa.SPEC_15 if ADAPTIVE else qa.SPEC_10
hop = spec.enc_hop
FPC = spec.dec_upsample if V20 else 2  # feature frames per code frame
codec = qa.Codec(None, None, None, spec=spec, device=dev, check_codes=False).load_state_dict(
    synth.hcodec20_state_dict(1234, synth.Shapes20()) if V20 else
    synth.hcodec10_state_dict(1234, spec) if ADAPTIVE else synth.hcodec10_state_dict(1234))
lens = [round(FRAMES[0] + (FRAMES[1] - FRAMES[0]) * i / max(N_CLIPS - 1, 1)) for i in range(N_CLIPS)]
lens = [lens[i] for i in torch.randperm(N_CLIPS, generator=torch.Generator().manual_seed(7)).tolist()]  # a file list is not sorted
distinct = sorted(set(lens))
n_max = max(lens)
wav = (synth.synth_wav_fullband(11, N_CLIPS, hop * n_max) if V20 else synth.synth_wav(11, N_CLIPS, hop * n_max)).to(dev)
feat = synth.synth_feat(12, N_CLIPS, FPC * n_max, spec.sem_in).to(dev)
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
    row = dict(bench=BENCH, name=name, clips=N_CLIPS, ms_median=round(ms[0], 3), ms_min=round(ms[1], 3), ms_max=round(ms[2], 3),
               reps=REPS, **kw)
    rows.append(row)
    print(json.dumps(row), flush=True)


def ragged():
    ac, sc = codec.encode(wav.unsqueeze(1), feat, lengths=lens)
    return ac, sc, codec.decode(ac, sc, lengths=lens)


def grouped():
    q = spec.num_quantizers
    ac = torch.full((N_CLIPS, q, n_max), -1, dtype=torch.int64, device=dev)
    sc = torch.full((N_CLIPS, q, n_max), -1, dtype=torch.int64, device=dev)
    w = torch.zeros((N_CLIPS, hop * n_max), device=dev)
    for f in distinct:
        idx = torch.tensor([b for b, x in enumerate(lens) if x == f], device=dev)
        a, s = codec.encode(wav[idx, :hop * f].unsqueeze(1), feat[idx, :, :2 * f])
        ac[idx, :, :f], sc[idx, :, :f] = a, s
        w[idx, :hop * f] = codec.decode(a, s)
    return ac, sc, w


def ragged15():
    c = codec.encode_ragged(wav.unsqueeze(1), feat, lens)
    return c["acoustic_codes"], c["semantic_codes"], codec.decode_ragged(**c)


def grouped15():
    """codes as a list per clip (every call has a group count of its own); the waveforms in one zero-initialised batch"""
    from unified_audio_amd import _lib

    ac, sc = [None] * N_CLIPS, [None] * N_CLIPS
    w = torch.zeros((N_CLIPS, hop * n_max), device=dev)
    for f in distinct:
        rows_f = [b for b, x in enumerate(lens) if x == f]
        idx = torch.tensor(rows_f, device=dev)
        old = _lib.set_knob("QA_SEANET_FUSED", 0)
        try:
            c = codec.encode(wav[idx, :hop * f].unsqueeze(1), feat[idx, :, :2 * f])
        finally:
            _lib.set_knob("QA_SEANET_FUSED", old)
        w[idx, :hop * f] = codec.decode(**c)
        for i, b in enumerate(rows_f):
            ac[b], sc[b] = c["acoustic_codes"][i], c["semantic_codes"][i]
    return ac, sc, w


def ragged20():
    ac, sc = codec.encode_ragged(wav, feat, lens)
    return ac, sc, codec.decode_ragged(ac, sc, lengths=lens)


def grouped20():
    q = spec.num_quantizers
    ac = torch.full((N_CLIPS, q, n_max), -1, dtype=torch.int64, device=dev)
    sc = torch.full((N_CLIPS, q, n_max), -1, dtype=torch.int64, device=dev)
    w = torch.zeros((N_CLIPS, hop * n_max), device=dev)
    for f in distinct:
        idx = torch.tensor([b for b, x in enumerate(lens) if x == f], device=dev)
        a, s = codec.encode(wav[idx, :hop * f], feat[idx, :, :FPC * f])
        ac[idx, :, :f], sc[idx, :, :f] = a, s
        w[idx, :hop * f] = codec.decode(a, s)
    return ac, sc, w


if V20:
    ms_r, (ar, sr, wr) = timed(ragged20)
    ms_g, (ag, sg, wg) = timed(grouped20)
    audio_s = sum(lens) * hop / SR
    report("ragged", ms_r, distinct_lengths=len(distinct), frames_min=min(lens), frames_max=max(lens), ms_per_clip=round(ms_r[0] / N_CLIPS, 3),
           audio_s_per_s=round(audio_s / ms_r[0] * 1e3, 1))
    report("grouped", ms_g, distinct_lengths=len(distinct), calls=len(distinct), ms_per_clip=round(ms_g[0] / N_CLIPS, 3),
           audio_s_per_s=round(audio_s / ms_g[0] * 1e3, 1))
    # the outputs are initialised to -1 / 0 behind every clip, which is what the per-clip calls write there: whole-tensor equality
    codes_equal = bool(torch.equal(ar, ag) and torch.equal(sr, sg))
    wav_equal = bool(torch.equal(wr, wg))
    row = dict(bench=BENCH, name="grouped_over_ragged", clips=N_CLIPS, ratio_of_medians=round(ms_g[0] / ms_r[0], 2),
               ratio_min=round(ms_g[1] / ms_r[2], 2), ratio_max=round(ms_g[2] / ms_r[1], 2), distinct_lengths=len(distinct),
               codes_equal=codes_equal, wav_equal=wav_equal)
    rows.append(row)
    print(json.dumps(row), flush=True)
    with open(OUT, "a") as f:
        f.write("== python tools/hcodec_ragged_bench.py " + " ".join(sys.argv[1:]) + "\n")
        for r in rows:
            f.write(json.dumps(r) + "\n")
    if not (codes_equal and wav_equal):
        sys.exit("the per-clip call and the rectangular calls differ on a clip's valid part")
    sys.exit(0)

if ADAPTIVE:
    ms_r, (ar, sr, wr) = timed(ragged15)
    ms_g, (ag, sg, wg) = timed(grouped15)
    audio_s = sum(lens) * hop / 16000.0
    K = spec.codebook_size
    nseg = (torch.div(sr[:, 0], K, rounding_mode="floor") + 1 > 0).sum(dim=1).tolist()
    report("ragged", ms_r, distinct_lengths=len(distinct), frames_min=min(lens), frames_max=max(lens), groups_min=min(nseg), groups_max=max(nseg),
           audio_s_per_s=round(audio_s / ms_r[0] * 1e3, 1))
    report("grouped", ms_g, distinct_lengths=len(distinct), calls=len(distinct), audio_s_per_s=round(audio_s / ms_g[0] * 1e3, 1))
    # a grouped call of more than one clip keeps the reference's batch semantics (padded queries are keys), so bit equality is defined
    # against B = 1 calls only: rows whose length is shared are compared on their own group count
    single = [b for b, x in enumerate(lens) if lens.count(x) == 1]
    codes_equal = all(torch.equal(ar[b, :, :nseg[b]], ag[b]) and torch.equal(sr[b, :, :nseg[b]], sg[b]) and bool((ar[b, :, nseg[b]:] == -1).all())
                      for b in single)
    wav_equal = all(torch.equal(wr[b, :hop * lens[b]], wg[b, :hop * lens[b]]) and not bool(wr[b, hop * lens[b]:].any()) for b in single)
    row = dict(bench=BENCH, name="grouped_over_ragged", clips=N_CLIPS, ratio_of_medians=round(ms_g[0] / ms_r[0], 2),
               ratio_min=round(ms_g[1] / ms_r[2], 2), ratio_max=round(ms_g[2] / ms_r[1], 2), distinct_lengths=len(distinct),
               rows_compared=len(single), codes_equal=codes_equal, wav_equal=wav_equal)
    rows.append(row)
    print(json.dumps(row), flush=True)
    with open(OUT, "a") as f:
        f.write("== python tools/hcodec_ragged_bench.py " + " ".join(sys.argv[1:]) + "\n")
        for r in rows:
            f.write(json.dumps(r) + "\n")
    if not (codes_equal and wav_equal):
        sys.exit("the per-clip call and the B = 1 calls differ on a clip's valid part")
    sys.exit(0)

ms_r, (ar, sr, wr) = timed(ragged)
ms_g, (ag, sg, wg) = timed(grouped)
audio_s = sum(lens) * hop / 16000.0
report("ragged", ms_r, distinct_lengths=len(distinct), frames_min=min(lens), frames_max=max(lens), audio_s_per_s=round(audio_s / ms_r[0] * 1e3, 1))
report("grouped", ms_g, distinct_lengths=len(distinct), calls=len(distinct), audio_s_per_s=round(audio_s / ms_g[0] * 1e3, 1))
codes_equal = bool(torch.equal(ar, ag) and torch.equal(sr, sg))
row = dict(bench="hcodec_ragged", name="grouped_over_ragged", clips=N_CLIPS, ratio_of_medians=round(ms_g[0] / ms_r[0], 2),
           ratio_min=round(ms_g[1] / ms_r[2], 2), ratio_max=round(ms_g[2] / ms_r[1], 2), distinct_lengths=len(distinct),
           codes_equal=codes_equal, wav_equal=bool(torch.equal(wr, wg)),
           wav_rel_rms=float(((wr - wg).double().pow(2).mean() / wg.double().pow(2).mean()).sqrt()))
rows.append(row)
print(json.dumps(row), flush=True)
with open(OUT, "a") as f:
    f.write("== python tools/hcodec_ragged_bench.py " + " ".join(sys.argv[1:]) + "\n")
    for r in rows:
        f.write(json.dumps(r) + "\n")
