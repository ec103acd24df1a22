"""Speed and agreement of conv_gemm's arithmetics (unified_audio_amd.gemm_math: fp32, split6, split3, bf16) on a codec's encode + decode
step at the bench shapes: ONE process, one set of weights and inputs, the modes alternated round by round in the way of tools/knob_ab.py.

    python tools/gemm_math_bench.py --model 1.5 [--modes split6,split3,bf16] [--rounds 3] [--steps 3] [--batch 32] [--seconds 10]

Per mode: ms per encode + decode step (every round, their mean and best); the fraction of acoustic and semantic codes equal to split-6's;
the relative RMS of the waveform decoded from split-6's codes against split-6's own decode; for split-6 itself the run-to-run spread of
the step time, (max - min) / mean over the rounds.  One JSON line per mode is appended to profiles/gemm_math_modes.jsonl.  Reads nothing
outside the repository (weights and inputs are synthetic, unified_audio_amd.synth).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="1.5", choices=["1.5", "1.0", "2.0"])
    ap.add_argument("--modes", default="split6,split3,bf16", help="comma-separated; split6 is always measured (the reference of the agreement figures)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gemm_math_modes.jsonl"))
    args = ap.parse_args()
    if args.rounds < 3:
        ap.error("--rounds: at least 3 alternating rounds")

    import unified_audio_amd as qa
    from unified_audio_amd import synth

    modes = ["split6"] + [m for m in args.modes.split(",") if m != "split6"]
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    model = args.model
    if model == "2.0":
        sr, spec = 48000, synth.Shapes20()
        codec = qa.Codec(None, None, None, spec=qa.SPEC_20, device=dev).load_state_dict(synth.hcodec20_state_dict(1234, spec))
        hop_in, frame_hop, sem_in = spec.hop, spec.frame_hop, spec.sem_in
    else:
        sr, spec = 16000, (qa.SPEC_15 if model == "1.5" else qa.SPEC_10)
        codec = qa.Codec(None, None, None, spec=spec, device=dev).load_state_dict(synth.hcodec10_state_dict(1234, spec))
        hop_in, frame_hop, sem_in = 320, spec.enc_hop, spec.sem_in
    adaptive = getattr(spec, "adaptive", False)
    B = args.batch
    T = int(round(args.seconds * sr / frame_hop)) * frame_hop
    wav = (synth.synth_wav_fullband(7, B, T) if model == "2.0" else synth.synth_wav(7, B, T)).to(dev)
    feats = synth.synth_feat(9, B, T // hop_in, sem_in).to(dev)

    def encode():
        if adaptive:
            return codec.encode(wav.unsqueeze(1), feats)
        ac, sc = codec.encode(wav.unsqueeze(1), feats)
        return {"acoustic_codes": ac, "semantic_codes": sc}

    def decode(codes):
        return codec.decode(**codes) if adaptive else codec.decode(codes["acoustic_codes"], codes["semantic_codes"])

    def step():
        codes = encode()
        return codes, decode(codes)

    # outputs and agreement, once per mode
    with qa.gemm_math("split6"):
        ref_codes, ref_wav = step()
        ref_codes = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in ref_codes.items()}
        ref_wav = ref_wav.clone()
    agree = {}
    for m in modes:
        with qa.gemm_math(m):
            codes, _ = step()
            w = decode(ref_codes)
            torch.cuda.synchronize(dev)
        a = {}
        for key in ("acoustic_codes", "semantic_codes"):
            u, v = codes[key], ref_codes[key]
            a[key + "_equal"] = float((u == v).float().mean()) if u.shape == v.shape else None  # adaptive models: another segmentation
        a["wave_rel_rms_from_split6_codes"] = float((w - ref_wav).double().pow(2).mean().sqrt() / ref_wav.double().pow(2).mean().sqrt())
        a["finite"] = bool(torch.isfinite(w).all())
        agree[m] = a

    # time, modes alternated round by round
    for m in modes:
        with qa.gemm_math(m):
            for _ in range(args.warmup):
                step()
    torch.cuda.synchronize(dev)
    times = {m: [] for m in modes}
    for _ in range(args.rounds):
        for m in modes:
            with qa.gemm_math(m):
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    step()
                torch.cuda.synchronize(dev)
                times[m].append(1e3 * (time.perf_counter() - t0) / args.steps)

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    base = sum(times["split6"]) / len(times["split6"])
    with open(args.out, "a") as f:
        for m in modes:
            t = times[m]
            mean = sum(t) / len(t)
            rec = {"tool": "gemm_math_bench", "model": f"H-Codec {model}", "batch": B, "seconds": args.seconds, "mode": m,
                   "QA_GEMM_MATH": qa._lib.GEMM_MATH_MODES[m], "steps_per_round": args.steps, "ms_per_step_rounds": [round(x, 3) for x in t],
                   "ms_per_step_mean": round(mean, 3), "ms_per_step_best": round(min(t), 3), "speedup_vs_split6": round(base / mean, 4),
                   **agree[m]}
            if m == "split6":
                rec["run_to_run_spread"] = round((max(t) - min(t)) / mean, 5)
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
