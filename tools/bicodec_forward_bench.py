"""Cost of BiCodec.forward (qa_bicodec_forward: tokenize, the x-vector head, detokenize with the postnet, the code statistics) against
tokenize + detokenize at the published widths, seeded weights: 16 and 64 clips x 6 s (XLSR-53 features at 50 Hz, the 6 s rows as
the reference clip).  HIP events around each call, median of the timed repetitions; one JSON line per batch size.

    python tools/bicodec_forward_bench.py [--batches 16,64] [--seconds 6] [--reps 5] [--warmup 2]
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


def timed(fn, warmup, reps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = []
    for r in range(warmup + reps):
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        if r >= warmup:
            ms.append(ev[0].elapsed_time(ev[1]))
    return statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="16,64")
    ap.add_argument("--seconds", type=float, default=6.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    dspec, espec, fspec = qa.SPEC_BICODEC, qa.SPEC_BICODEC_ENCODER, qa.BiCodecForwardSpec()
    sd = synth.bicodec_state_dict(3, dspec)
    sd.update(synth.bicodec_encoder_state_dict(4, espec))
    sd.update(synth.bicodec_speaker_state_dict(5, espec))
    sd.update(synth.bicodec_forward_state_dict(6, fspec))
    m = qa.BiCodec(dspec, device=dev, encoder_spec=espec, forward_spec=fspec).load_state_dict(sd)
    del sd
    assert m.has_forward
    for B in (int(b) for b in args.batches.split(",")):
        samples = int(args.seconds * espec.sample_rate)
        N = samples // espec.hop_length
        wav = synth.synth_wav(7, B, samples).to(dev)
        feat = synth.synth_feat(8, B, N, espec.input_channels).transpose(1, 2).contiguous().to(dev)
        batch = {"feat": feat, "ref_wav": wav, "wav": wav}
        t_fwd = timed(lambda: m(batch), args.warmup, args.reps)
        t_td = timed(lambda: m.detokenize(*m.tokenize(batch)), args.warmup, args.reps)
        t_tok = timed(lambda: m.tokenize(batch), args.warmup, args.reps)
        print(json.dumps({"workload": "bicodec_forward", "batch": B, "seconds": args.seconds, "forward_ms": round(t_fwd, 2),
                          "tokenize_detokenize_ms": round(t_td, 2), "tokenize_ms": round(t_tok, 2), "extra_ms": round(t_fwd - t_td, 2),
                          "postnet_layers": fspec.vocos_layers, "prenet_layers": dspec.vocos_layers, "reps": args.reps}), flush=True)
        del batch, wav, feat
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
