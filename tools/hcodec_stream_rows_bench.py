#!/usr/bin/env python
"""A step of the H-Codec 1.0 stream with per-row lengths (Codec.encode_stream(lengths=)) against the rectangular
step and against what a server has without it.

Real H-Codec 1.0 encoder widths, causal, B = 32, a history of 250 code frames, single-frame steps (codes only), HIP events around each step,
median of REPS after a warm-up pair - as tools/hcodec_stream_bench.py measures section 43:

    (a) rect        encode_stream(x): every row at one offset, the rectangular launches
    (b) staggered   encode_stream(x, lengths=[1] * 32) with row b at offset 250 - b (it joined b frames late): every row live, per-row launches
    (c) half_idle   the same stream, lengths = [1, 0] * 16: every second row idles
    (d) serial_b1   32 steps of a B = 1 stream between one pair of events: the 32 single-row streams a server steps one after another
                    today.  ONE B = 1 stream is stepped 32 times (a handle holds one stream; the launches, their grids and the weights are
                    those of 32 handles, only the few KiB of per-stream state stay warmer in cache)

One JSON line per figure, appended to profiles/hcodec_stream_rows_bench.jsonl (--out: another path).

    python tools/hcodec_stream_rows_bench.py [--reps 5] [--out PATH] [--batch 32] [--history 250]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hcodec_stream_rows_bench.jsonl"))
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--history", type=int, default=250)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, hist, reps = args.batch, args.history, args.reps
    assert hist - B >= 2, "row b joins b frames late and still needs a first chunk of 2 frames"
    spec = qa.HCodecSpec(dec_layers=1, convnext_layers=1, causal=True)
    codec = qa.Codec(None, None, None, spec=spec, device=dev).load_state_dict(synth.hcodec10_state_dict(1234, spec))
    hop = spec.enc_hop
    g = torch.Generator(device=dev).manual_seed(B * 10000 + hist)
    wav = 0.1 * torch.randn(B, 1, hist * hop, device=dev, generator=g)
    x1 = 0.1 * torch.randn(B, 1, hop, device=dev, generator=g)
    capacity = hist + 2 * (reps + 2) + 1
    rows = []

    def report(name, ts, **more):
        med = statistics.median(ts)
        row = dict(bench="hcodec_stream_rows", name=name, B=B, n=1, history=hist, ms_median=round(med, 4), ms_min=round(min(ts), 4),
                   ms_max=round(max(ts), 4), reps=reps, **more)
        rows.append(row)
        print(json.dumps(row), flush=True)
        return med

    def steps(fn):
        return [timed(fn) for _ in range(reps + 2)][2:]  # a warm-up pair first

    with codec.streaming(B, max_frames=capacity):
        codec.encode_stream(wav)
        a = report("rect", steps(lambda: codec.encode_stream(x1)), offsets="all %d" % hist)
    with codec.streaming(B, max_frames=capacity):
        codec.encode_stream(wav, lengths=[hist - b for b in range(B)])
        off = codec.streaming_offsets
        b_ms = report("staggered", steps(lambda: codec.encode_stream(x1, lengths=[1] * B)), offsets="%d .. %d" % (min(off), max(off)))
        c_ms = report("half_idle", steps(lambda: codec.encode_stream(x1, lengths=[1, 0] * (B // 2) + [1] * (B % 2))),
                      offsets="%d .. %d" % (min(off), max(off)))
    with codec.streaming(1, max_frames=hist + B * (reps + 2)):
        codec.encode_stream(wav[:1])
        x = x1[:1].contiguous()

        def serial():
            for _ in range(B):
                codec.encode_stream(x)

        d_ms = report("serial_b1", steps(serial), note="%d steps of a B = 1 stream" % B)
    summary = dict(bench="hcodec_stream_rows", name="summary", B=B, rows_over_rect_ms=round(b_ms - a, 4), staggered_over_rect=round(b_ms / a, 3),
                   half_idle_over_rect=round(c_ms / a, 3), serial_over_staggered=round(d_ms / b_ms, 2))
    rows.append(summary)
    print(json.dumps(summary), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
