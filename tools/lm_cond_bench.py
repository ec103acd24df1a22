"""Throughput of the UniSE condition path at the shipped spec (Conformer 6 x 512, 8 heads x 64, k = 31; LM 12 x 512), seeded weights:

    encoder  : stft_logmel (B x 5 s -> [B, 250, 80]) + condition encoder -> [B, 250, 512]
    generate : CustomLlamaModel.generate(cond), 32 global + 250 semantic greedy steps behind the 251-position prompt
    forward  : CustomLlamaModel.forward(global_ids, semantic_ids, cond), Lt = 283 targets behind the prompt

HIP events around each call, median of the timed repetitions.  The condition encoder's algorithmic FLOP count (per frame and layer:
FF 2 x 4 d^2 x 2, projections 8 d^2, attention 4 d T, 1x1 convolutions 6 d^2, depthwise 2 k d) over the time gives the fraction of
the fp32 MFMA peak (157.3 TFLOP/s).  The new byte-bound kernel (GLU + depthwise + BatchNorm + SiLU) is timed launch by launch by the
library's own hook (qa_profile_begin_ex(2), every kernel alone on the device) and priced against the HBM peak of 8 TB/s with its
algorithmic bytes (12 per element: both halves of the 1x1 output in, one value out).  Prints one JSON line per configuration and batch;
--out appends them to a file (profiles/lm_cond_bench.jsonl).

    python tools/lm_cond_bench.py [--batches 16,64] [--reps 5] [--warmup 2] [--out FILE] [--encoder-only]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import unified_audio_amd as qa  # noqa: E402
from unified_audio_amd import synth, unise  # noqa: E402

import ctypes as C  # noqa: E402

from unified_audio_amd import _lib  # noqa: E402

FP32_PEAK = 157.3e12
HBM_PEAK_GBPS = 8000.0
CF = synth.CONFORMER_PARAMS_UNISE


def encoder_flops(B, T, cond_dim=80, hidden=512):
    d, inner, k, ff = CF["dim"], CF["heads"] * CF["dim_head"], CF["depthwise_conv_kernel_size"], CF["ff_mult"]
    per_frame = 2 * (2 * 2 * d * ff * d) + 2 * d * 3 * inner + 2 * inner * d + 4 * inner * T + 2 * d * 2 * d + 2 * d * d + 2 * k * d
    return B * T * (CF["num_layers"] * per_frame + 2 * cond_dim * d + 2 * d * hidden)


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def hbm_rows(fn):
    """per-kind rows of the byte-bound kernels of one call of fn, each launch alone on the device"""
    lib = _lib.load_library()
    n = lib.qa_profile_hbm_kinds()
    hbm, iso = (C.c_double * (3 * n))(), (C.c_double * 64)()
    _lib.check(lib.qa_set_serial(1))
    _lib.check(lib.qa_profile_begin_ex(2))
    fn()
    torch.cuda.synchronize()
    _lib.check(lib.qa_profile_end_hbm(hbm, 3 * n))
    _lib.check(lib.qa_profile_end(iso, 64))
    _lib.check(lib.qa_set_serial(0))
    rows = []
    for k in range(n):
        by, ms, cnt = hbm[3 * k], hbm[3 * k + 1], hbm[3 * k + 2]
        if cnt:
            rows.append(dict(kernel=lib.qa_profile_hbm_name(k).decode(), launches=int(cnt), avg_us=round(1e3 * ms / cnt, 2),
                             algorithmic_MB_per_launch=round(by / cnt / 1e6, 3), achieved_GBps=round(by / (ms * 1e-3) / 1e9, 1),
                             roofline_hbm=round(by / (ms * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4)))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--encoder-only", action="store_true")
    ap.add_argument("--batches", default="16,64")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    sd = {k: v for k, v in synth.lm_state_dict(3).items() if not k.startswith(("task_embedding", "enroll_sos", "adapter"))}
    sd.update(synth.cond_encoder_state_dict(4, 80, 512, CF, gain=2.0))
    m = qa.CustomLlamaModel(cond_dim=80, hidden_size=512, num_layers=12, num_attention_heads=8, conformer_params=CF, device=dev).load_state_dict(sd)
    G, S = 32, 250
    sink = open(args.out, "a") if args.out else None

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()
    for B in (int(b) for b in args.batches.split(",")):
        wav = synth.synth_wav(5, B, 80000).to(dev)
        mel = unise.stft_logmel(wav)
        T = mel.shape[1]
        gen = torch.Generator().manual_seed(6)
        g = torch.randint(0, 4096, (B, G), generator=gen).to(dev)
        s = torch.randint(0, 8192, (B, S), generator=gen).to(dev)
        t_mel = timed(lambda: unise.stft_logmel(wav), args.reps, args.warmup)
        t_enc = timed(lambda: m.encode_condition(mel), args.reps, args.warmup)
        fl = encoder_flops(B, T)
        emit(dict(config="encoder", B=B, frames=T, logmel_ms=round(t_mel, 3), encoder_ms=round(t_enc, 3), encoder_tflop=round(fl / 1e12, 3),
                              fp32_peak_fraction=round(fl / (t_enc * 1e-3) / FP32_PEAK, 4), audio_s_per_s=round(B * 5.0 / ((t_mel + t_enc) * 1e-3), 1)))
        for row in hbm_rows(lambda: m.encode_condition(mel)):
            emit(dict(config="encoder_byte_bound", B=B, **row))
        if args.encoder_only:
            continue
        t_gen = timed(lambda: m.generate(mel, global_length=G, semantic_length=S, do_sample=False), args.reps, args.warmup)
        emit(dict(config="generate", B=B, prompt=T + 1, steps=G + S, ms=round(t_gen, 2), tok_per_s=round(B * (G + S) / (t_gen * 1e-3), 1)))
        t_fwd = timed(lambda: m(g, s, mel), args.reps, args.warmup)
        emit(dict(config="forward", B=B, positions=T + 1 + G + S, ms=round(t_fwd, 2), seq_per_s=round(B / (t_fwd * 1e-3), 1)))


if __name__ == "__main__":
    main()
