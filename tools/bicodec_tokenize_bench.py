"""Throughput of BiCodecTokenizer.tokenize at the published shapes, seeded weights, split into its three parts:

    normalise + XLSR-53 (hidden states 11 / 14 / 16)   bicodec.wav_normalize + SSLFeatureExtractor(SPEC_XLSR53_BICODEC)
    semantic encoder + VQ                              BiCodec.get_semantic_tokens
    mel + ECAPA + perceiver + FSQ                      BiCodec.get_global_tokens (6 s reference clip)

HIP events around each part, B rows of S seconds (16 kHz), median of the timed repetitions.  Prints one JSON line per batch size.

    python tools/bicodec_tokenize_bench.py [--batches 16,64] [--seconds 6] [--reps 5] [--warmup 2]
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
from unified_audio_amd.ssl import SPEC_XLSR53_BICODEC  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="16,64")
    ap.add_argument("--seconds", type=float, default=6.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    fx = qa.SSLFeatureExtractor(SPEC_XLSR53_BICODEC, device=dev).load_state_dict(synth.ssl_state_dict(SPEC_XLSR53_BICODEC, 21))
    sd = synth.bicodec_state_dict(1, qa.SPEC_BICODEC)
    sd.update(synth.bicodec_encoder_state_dict(2, qa.SPEC_BICODEC_ENCODER))
    sd.update(synth.bicodec_speaker_state_dict(3, qa.SPEC_BICODEC_ENCODER))
    model = qa.BiCodec(qa.SPEC_BICODEC, device=dev).load_state_dict(sd)
    del sd
    T = int(16000 * args.seconds)
    for B in (int(b) for b in args.batches.split(",")):
        wav = synth.synth_wav(3, B, T).to(dev)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        front, sem, glob = [], [], []
        ref_len = qa.SPEC_BICODEC_ENCODER.ref_segment_length()
        for r in range(args.warmup + args.reps):
            ev[0].record()
            feat = fx(qa.wav_normalize(wav))
            ev[1].record()
            tok = model.get_semantic_tokens({"feat": feat})
            ev[2].record()
            gtok = model.get_global_tokens({"ref_wav": wav}, ref_len)
            ev[3].record()
            torch.cuda.synchronize()
            if r >= args.warmup:
                front.append(ev[0].elapsed_time(ev[1]))
                sem.append(ev[1].elapsed_time(ev[2]))
                glob.append(ev[2].elapsed_time(ev[3]))
        f, s, g = statistics.median(front), statistics.median(sem), statistics.median(glob)
        print(json.dumps({"workload": "bicodec_tokenize", "batch": B, "seconds": args.seconds, "frames": int(feat.shape[1]),
                          "normalize_xlsr_ms": round(f, 3), "semantic_encoder_vq_ms": round(s, 3), "mel_ecapa_perceiver_fsq_ms": round(g, 3),
                          "audio_s_per_s": round(B * args.seconds / ((f + s + g) / 1000.0), 1),
                          "distinct_semantic_tokens": int(torch.unique(tok).numel()),
                          "distinct_global_tokens": int(torch.unique(gtok).numel()), "reps": args.reps}), flush=True)


if __name__ == "__main__":
    main()
