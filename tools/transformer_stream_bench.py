#!/usr/bin/env python
"""Streaming steps of the codec Transformer (unified_audio_amd.Transformer) on the GPU, through both attention paths.

For d = 512 / 768 / 1024 (8 heads) and 1536 (24 heads), 2 layers, B = 1 / 8 / 32 and a history of 500 and 1500 frames: one streaming step of
1, 4 and 16 frames with the short-chunk kernel (QA_TR_SHORT_ATTN = 2) and through attention_kernel (= 0), the two alternated step by step in
one process.  HIP events around each step, median of REPS after one warm-up pair; the offset drifts by the timed steps themselves and is
recorded (offset_first .. offset_last).  Beside them: the offline causal forward of the whole history divided by its frames, and the
20 ms a 50 Hz frame lasts.  One JSON line per figure, appended to profiles/transformer_stream_bench.jsonl (--out: another path).

    python tools/transformer_stream_bench.py [--reps 5] [--out PATH] [--dims 512,768] [--batches 1,8]
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
from unified_audio_amd import _lib  # noqa: E402
from tests.transformer_stream_ref import random_state_dict  # noqa: E402  (seeded O(1) weights: data generation only)

HEADS = {512: 8, 768: 8, 1024: 8, 1536: 24}
FRAME_MS = 20.0  # one frame of a 50 Hz codec
CAPACITY = 2048


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transformer_stream_bench.jsonl"))
    ap.add_argument("--dims", default="512,768,1024,1536")
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--offsets", default="500,1500")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []

    def report(**row):
        row = dict(bench="transformer_stream", **row)
        rows.append(row)
        print(json.dumps(row), flush=True)

    for d in (int(v) for v in args.dims.split(",")):
        m = qa.Transformer(d, 3 * d, HEADS[d], 2, causal=True, device=dev).load_state_dict(random_state_dict(7, d, 3 * d, 2))
        for B in (int(v) for v in args.batches.split(",")):
            for off in (int(v) for v in args.offsets.split(",")):
                x = torch.randn(B, off, d, device=dev)
                step_in = {n: torch.randn(B, n, d, device=dev) for n in (1, 4, 16)}
                m(x)  # warm-up
                ts = [timed(lambda: m(x)) for _ in range(3)]
                off_ms = statistics.median(ts)
                report(name="offline_causal", d=d, heads=HEADS[d], B=B, frames=off, ms_median=round(off_ms, 4), ms_per_frame=round(off_ms / off, 5),
                       frame_budget_ms=FRAME_MS)
                with m.streaming(B, max_frames=CAPACITY):
                    m(x)  # the history, as one chunk
                    for n in (1, 4, 16):
                        t = {2: [], 0: []}
                        first = m.streaming_offset
                        for rep in range(args.reps + 1):
                            for path in (2, 0):  # 2: the short-chunk kernel whatever batch x frames is
                                _lib.set_knob("QA_TR_SHORT_ATTN", path)
                                ms = timed(lambda: m(step_in[n]))
                                if rep:  # rep 0: warm-up of both paths
                                    t[path].append(ms)
                        last = m.streaming_offset
                        for path, name in ((2, "short_chunk"), (0, "attention_kernel")):
                            med = statistics.median(t[path])
                            report(name="stream_step", attention=name, d=d, heads=HEADS[d], B=B, n=n, offset_first=first, offset_last=last,
                                   capacity=CAPACITY, ms_median=round(med, 4), ms_min=round(min(t[path]), 4), ms_max=round(max(t[path]), 4),
                                   ms_per_frame=round(med / n, 5), offline_ms_per_frame=round(off_ms / off, 5), frame_budget_ms=FRAME_MS,
                                   reps=args.reps)
                _lib.set_knob("QA_TR_SHORT_ATTN", 1)
        del m
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
