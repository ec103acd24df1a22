"""Throughput of LLM_SFT.forward (teacher-forced scoring, qa_lm_score) at the UniSE spec, seeded weights:

    se  : B sequences of 5 s (250 mix frames -> prompt 252) + 32 global + 250 semantic targets (Lt 284): 536 positions
    tse : the same with a 5 s enrollment (250 frames -> prompt 503): 787 positions

HIP events around forward (which includes the one host synchronisation of the ids' range check), median of the timed repetitions.
The algorithmic FLOP count (body GEMMs, causal attention, adapter, full-vocabulary head) over the time gives the fraction of the fp32
MFMA peak (157.3 TFLOP/s).  Prints one JSON line per configuration.

    python tools/lm_score_bench.py [--configs se:16,tse:64] [--reps 5] [--warmup 2]
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
from unified_audio_amd import synth  # noqa: E402
from oracle import llm_ref as L  # noqa: E402

FP32_PEAK = 157.3e12


def flops(spec, B, Ne, Nm, Lt):
    d, I, V = spec.hidden, spec.intermediate, spec.vocab
    n = 1 + (1 + Ne if Ne else 0) + 1 + Nm + Lt
    per_pos = spec.n_layers * (2 * d * 3 * d + 2 * d * d + 2 * d * 2 * I + 2 * I * d)
    attn = spec.n_layers * 2 * 2 * d * n * (n + 1) / 2  # QK^T and PV over the causal triangle
    adapter = 2 * spec.feats_dim * d * (Nm + Ne)
    head = 2 * d * V * Lt
    return B * (per_pos * n + attn + adapter + head), n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="se:16,tse:64")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    spec = L.SPEC_UNISE
    lm = qa.LLM_SFT(device=dev).load_state_dict(synth.lm_state_dict(3, spec))
    Nm, G, T = 250, 32, 250
    for cfg in args.configs.split(","):
        task, B = cfg.split(":")
        B = int(B)
        Ne = 250 if task != "se" else 0
        mix = synth.synth_feats(4, B, Nm, spec.feats_dim).to(dev)
        enr = synth.synth_feats(5, B, Ne, spec.feats_dim).to(dev) if Ne else None
        gen = torch.Generator().manual_seed(6)
        g = torch.randint(0, spec.global_size, (B, G), generator=gen, dtype=torch.int32).to(dev)
        s = torch.randint(0, spec.semantic_size, (B, T), generator=gen).to(dev)
        mel = torch.zeros(B, 1, 80)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ms = []
        for r in range(args.warmup + args.reps):
            ev[0].record()
            loss, acc = lm(task, None if enr is None else mel, enr, mel, mix, g, s)
            ev[1].record()
            torch.cuda.synchronize()
            if r >= args.warmup:
                ms.append(ev[0].elapsed_time(ev[1]))
        t = statistics.median(ms)
        f, n = flops(spec, B, Ne, Nm, G + T + 2)
        print(json.dumps({"workload": "lm_score", "task": task, "batch": B, "positions": n, "target_rows": B * (G + T + 2),
                          "ms": round(t, 3), "ms_min": round(min(ms), 3), "positions_per_s": round(B * n / (t / 1000.0)),
                          "tflop": round(f / 1e12, 3), "fp32_mfma_peak_fraction": round(f / (t / 1000.0) / FP32_PEAK, 3),
                          "loss": round(float(loss), 5), "acc": round(float(acc), 5), "reps": args.reps}), flush=True)


if __name__ == "__main__":
    main()
