"""Cost of Codec.forward (encode -> RVQ -> decode + the semantic decoder, qa_hcodec_forward*) against encode + decode, seeded weights:

    15 : H-Codec 1.5 (32-layer adaptive stacks), 32 clips x 10 s
    10 : H-Codec 1.0, 32 clips x 10 s
    20 : H-Codec 2.0, 16 clips x 30 s

HIP events around each call, median of the timed repetitions.  Per configuration: forward, encode + decode, the extra milliseconds
of forward, and the semantic decoder's algorithmic GFLOP with its fraction of the fp32 MFMA peak (157.3 TFLOP/s) over
those extra milliseconds.  One JSON line per configuration.

    python tools/hcodec_forward_bench.py [--configs 15,10,20] [--reps 5] [--warmup 2]
"""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import unified_audio_amd as qa  # noqa: E402
from unified_audio_amd import synth  # noqa: E402
from unified_audio_amd.hcodec import SemanticDecoderSpec  # noqa: E402

FP32_PEAK = 157.3e12
CONFIGS = {"15": (qa.SPEC_15, 32, 10.0), "10": (qa.SPEC_10, 32, 10.0), "20": (qa.SPEC_20, 16, 30.0)}


def semantic_decoder_flops(sds: SemanticDecoderSpec, B: int, n: int) -> float:
    """multiply-adds x 2 of semantic_module.Decoder on B x n input frames (the ConvTranspose1d k = 2 s: 2 taps per output frame)"""
    c = int(sds.decode_channels * sds.channel_ratios[0])
    f = 2.0 * n * sds.code_dim * c * 3
    for s, co in zip(sds.strides, sds.widths):
        f += 2.0 * n * c * co * 3 if s == 1 else 2.0 * n * s * c * co * 2
        n *= s
        f += 2 * (2.0 * n * co * co * 3 + 2.0 * n * co * co)
        c = co
    f += 2.0 * n * c * sds.output_channels * 3
    return B * f


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
    ap.add_argument("--configs", default="15,10,20")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for cfg in args.configs.split(","):
        spec, B, sec = CONFIGS[cfg]
        sds = SemanticDecoderSpec.from_codec_spec(spec)
        sd = synth.hcodec20_state_dict(3, synth.Shapes20()) if spec.version == 20 else synth.hcodec10_state_dict(3, spec)
        sd.update(synth.hcodec_semantic_decoder_state_dict(4, sds))
        codec = qa.Codec(None, None, None, spec=spec, device=dev).load_state_dict(sd)
        del sd
        sr = 48000 if spec.version == 20 else 16000
        T = int(sec * sr) // spec.enc_hop * spec.enc_hop
        wav = (synth.synth_wav_fullband(5, B, T) if spec.version == 20 else synth.synth_wav(5, B, T)).to(dev)
        x = wav if spec.version == 20 else wav.unsqueeze(1)
        n_ssl = T // (spec.hop if spec.version == 20 else 320)
        feat = synth.synth_feat(6, B, n_ssl, spec.sem_in).to(dev)

        def enc_dec():
            enc = codec.encode(x, feat)
            return codec.decode(enc["acoustic_codes"], enc["semantic_codes"]) if spec.adaptive else codec.decode(*enc)

        t_fwd = timed(lambda: codec(x, feat), args.warmup, args.reps)
        t_ed = timed(enc_dec, args.warmup, args.reps)
        n25 = T // spec.enc_hop
        f = semantic_decoder_flops(sds, B, n25)
        extra = t_fwd - t_ed
        print(json.dumps({"workload": "hcodec_forward", "version": {10: "1.0", 20: "2.0"}[spec.version] if not spec.adaptive else "1.5",
                          "batch": B, "seconds": sec, "forward_ms": round(t_fwd, 2),
                          "encode_decode_ms": round(t_ed, 2), "extra_ms": round(extra, 2),
                          "semantic_decoder_gflop": round(f / 1e9, 1), "gflop_per_audio_s": round(f / 1e9 / (B * sec), 2),
                          "fp32_mfma_peak_fraction_of_extra": round(f / (extra / 1000.0) / FP32_PEAK, 3) if extra > 0 else None,
                          "reps": args.reps, "pred_feat_shape": [B, sds.output_channels, n25 * int(math.prod(sds.strides))]}),
              flush=True)
        del codec
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
