#!/usr/bin/env python
"""Steps of the chunked causal H-Codec 1.0 encoder (Codec.streaming / encode_stream) on the GPU.

Real H-Codec 1.0 encoder widths (ratios 2, 4, 5, 8; 32 -> 512 channels; two d = 512 Transformer layers; 4 x 1024 codes) with the causal
spec; the decoder, which a stream never runs, is cut to one layer each to keep the upload short.  For B = 1 / 8 / 32 and a history of 250
and 2000 code frames: one step of n = 1, 2, 5 and 25 code frames (codes only, as a caller streams), HIP events around each step, median of
REPS after a warm-up pair; the offset drifts by the timed steps themselves and is recorded.  Beside each figure: the offline causal
`encode` of the same history divided by its frames, the n x 40 ms the step's audio lasts (640 samples at 16 kHz per code frame) and the
real-time factor ms / (n x 40 ms).  One JSON line per figure, appended to profiles/hcodec_stream_bench.jsonl (--out: another path).

    python tools/hcodec_stream_bench.py [--reps 5] [--out PATH] [--batches 1,8] [--histories 250] [--steps 1,2,5,25]
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
from unified_audio_amd import synth  # noqa: E402

FRAME_MS = 40.0  # one code frame: 640 samples at 16 kHz
HISTORY_CHUNK = 250  # the history is streamed in chunks of this many code frames


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hcodec_stream_bench.jsonl"))
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--histories", default="250,2000")
    ap.add_argument("--steps", default="1,2,5,25")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    steps = [int(v) for v in args.steps.split(",")]
    spec = qa.HCodecSpec(dec_layers=1, convnext_layers=1, causal=True)
    codec = qa.Codec(None, None, None, spec=spec, device=dev).load_state_dict(synth.hcodec10_state_dict(1234, spec))
    hop = spec.enc_hop
    rows = []

    def report(**row):
        row = dict(bench="hcodec_stream", **row)
        rows.append(row)
        print(json.dumps(row), flush=True)

    for B in (int(v) for v in args.batches.split(",")):
        for hist in (int(v) for v in args.histories.split(",")):
            g = torch.Generator(device=dev).manual_seed(B * 10000 + hist)
            wav = 0.1 * torch.randn(B, 1, hist * hop, device=dev, generator=g)
            feat = torch.randn(B, spec.sem_in, 2 * hist, device=dev, generator=g)
            step_in = {n: 0.1 * torch.randn(B, 1, n * hop, device=dev, generator=g) for n in steps}
            codec.encode(wav, feat)  # warm-up (sizes the workspace)
            off_ms = statistics.median(timed(lambda: codec.encode(wav, feat)) for _ in range(3))
            report(name="offline_causal_encode", B=B, frames=hist, ms_median=round(off_ms, 4), ms_per_frame=round(off_ms / hist, 5),
                   frame_budget_ms=FRAME_MS, note="acoustic and semantic encoder, both RVQs")
            capacity = hist + (args.reps + 2) * sum(steps)
            with codec.streaming(B, max_frames=capacity):
                for t in range(0, hist, HISTORY_CHUNK):
                    codec.encode_stream(wav[..., t * hop:min(t + HISTORY_CHUNK, hist) * hop])
                for n in steps:
                    first = codec.streaming_offset
                    ts = [timed(lambda: codec.encode_stream(step_in[n])) for _ in range(args.reps + 2)][2:]  # a warm-up pair first
                    med = statistics.median(ts)
                    report(name="stream_step", B=B, n=n, offset_first=first, offset_last=codec.streaming_offset, capacity=capacity,
                           ms_median=round(med, 4), ms_min=round(min(ts), 4), ms_max=round(max(ts), 4), ms_per_frame=round(med / n, 5),
                           offline_ms_per_frame=round(off_ms / hist, 5), audio_ms=n * FRAME_MS, realtime_factor=round(med / (n * FRAME_MS), 5),
                           within_budget=bool(med < n * FRAME_MS), reps=args.reps)
            del wav, feat
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
