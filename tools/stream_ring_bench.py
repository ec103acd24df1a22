#!/usr/bin/env python
"""Streaming steps of the codec Transformer over a ring K / V cache beside the linear stream, on the GPU.

The block is d = 512, 8 heads, 2 layers under a sliding window W = 250 and 1500; B = 1 / 8 / 32; steps of 1, 4 and 16 frames.  Two handles with
the same weights run side by side, alternated step by step in one process: a ring stream (max_chunk = 16, so W + 16 rows rounded up to 32)
and a linear stream of 2048 rows at an offset behind W, where the window shows it the same number of keys.  The ring is timed in four
phases: before its first wrap, after three turns, on the steps that end at position 8192 (the last of the static RoPE table) and on the
steps that start there (angles from the kernel's own evaluation).  HIP events around each step, median of REPS after one warm-up pair;
the offsets are recorded.  Also: the bytes of state a row holds in both forms.  One JSON line per figure, appended to
profiles/stream_ring_bench.jsonl (--out: another path).

    python tools/stream_ring_bench.py [--reps 5] [--out PATH] [--windows 250,1500] [--batches 1,8,32]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import unified_audio_amd as qa  # noqa: E402
from tests.transformer_stream_ref import random_state_dict  # noqa: E402  (seeded O(1) weights: data generation only)

D, HEADS, LAYERS = 512, 8, 2
MAX_CHUNK = 16
LINEAR_ROWS = 2048
TABLE = 8192  # positions of the static RoPE table


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def feed(m, B, upto, dev):
    """Advance the stream of m to `upto` frames in steps of up to MAX_CHUNK."""
    x = torch.randn(B, MAX_CHUNK, D, device=dev)
    while m.streaming_offset < upto:
        m(x[:, :min(MAX_CHUNK, upto - m.streaming_offset)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_ring_bench.jsonl"))
    ap.add_argument("--windows", default="250,1500")
    ap.add_argument("--batches", default="1,8,32")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []

    def report(**row):
        row = dict(bench="stream_ring", d=D, heads=HEADS, layers=LAYERS, **row)
        rows.append(row)
        print(json.dumps(row), flush=True)

    sd = random_state_dict(7, D, 3 * D, LAYERS)
    for W in (int(v) for v in args.windows.split(",")):
        ring, lin = (qa.Transformer(D, 3 * D, HEADS, LAYERS, causal=True, use_sliding_window=True, left_context=W, device=dev).load_state_dict(sd)
                     for _ in range(2))
        for B in (int(v) for v in args.batches.split(",")):
            step_in = {n: torch.randn(B, n, D, device=dev) for n in (1, 4, 16)}
            for n in (1, 4, 16):
                span = (args.reps + 1) * n  # frames the timed steps of one phase consume
                with ring.streaming(B, max_chunk=MAX_CHUNK), lin.streaming(B, max_frames=LINEAR_ROWS):
                    cap = ring.streaming_capacity
                    feed(lin, B, W + MAX_CHUNK, dev)
                    phases = (("ring_before_wrap", cap - span), ("ring_wrapped", 3 * cap + 7), ("ring_below_8192", TABLE - span),
                              ("ring_above_8192", TABLE))
                    for phase, start in phases:
                        feed(ring, B, start, dev)
                        t = {"ring": [], "linear": []}
                        first = {"ring": ring.streaming_offset, "linear": lin.streaming_offset}
                        for rep in range(args.reps + 1):
                            for name, m in (("ring", ring), ("linear", lin)):
                                ms = timed(lambda: m(step_in[n]))
                                if rep:  # rep 0: warm-up of both
                                    t[name].append(ms)
                        for name, m in (("ring", ring), ("linear", lin)):
                            med = statistics.median(t[name])
                            report(name=phase if name == "ring" else "linear_beside_" + phase, W=W, B=B, n=n, rows=m.streaming_capacity,
                                   offset_first=first[name], offset_last=m.streaming_offset, visible_keys=min(W, first[name] + 1),
                                   ms_median=round(med, 4), ms_min=round(min(t[name]), 4), ms_max=round(max(t[name]), 4), reps=args.reps)
        # what a row of the stream keeps: per layer the LSTM's (h, c) and the K / V rows, fp32
        for name, kv_rows in (("ring", qa_capacity(W)), ("linear_8192", TABLE)):
            report(name="state_bytes_per_row", form=name, W=W, rows=kv_rows, bytes=LAYERS * (2 * D + 2 * kv_rows * D) * 4)
        del ring, lin
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


def qa_capacity(W):
    """Rows of the ring for max_chunk = MAX_CHUNK (csrc/ring_geometry.h: W + max_chunk, rounded up to 32)."""
    return (W + MAX_CHUNK + 31) // 32 * 32


if __name__ == "__main__":
    main()
