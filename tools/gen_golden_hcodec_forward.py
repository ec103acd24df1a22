"""Write tests/golden/hcodec_forward_{10,15,20}_*.npz: the reference's OWN Codec.forward (eval) on seeded synthetic weights and inputs.

The files hold outputs only (codes, recon, pred_feat, token_lengths) plus the seeds and shapes; tests/test_hcodec_forward_gpu.py
regenerates the inputs from the seeds.  Needs the reference tree (oracle/ref_shim.py):  python tools/gen_golden_hcodec_forward.py
"""
from __future__ import annotations

import dataclasses
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import hcodec_ref as R  # noqa: E402
from oracle import ref_shim, synth  # noqa: E402
from unified_audio_amd.hcodec import SemanticDecoderSpec  # noqa: E402
from unified_audio_amd.synth import hcodec_semantic_decoder_state_dict  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
# (name, version, seed, batch, samples); 1.5 at full width with 2-layer stacks and threshold 0.7, 2.0 at oracle/gen_golden.SPEC20_SMALL
CASES = [("hcodec_forward_10_b2", "1.0", 9501, 2, 640 * 6),
         ("hcodec_forward_15_b2", "1.5", 9601, 2, 640 * 6),
         ("hcodec_forward_20_b2", "2.0", 9701, 2, 3840 * 4)]


def spec_for(version):
    if version == "1.0":
        return R.SPEC_10
    if version == "1.5":
        return dataclasses.replace(R.SPEC_15, agg_layers=2, bt_layers=2, threshold=0.7)
    from oracle import hcodec20_ref as R20
    from oracle.gen_golden import SPEC20_SMALL

    return R20.HCodec20Spec(**SPEC20_SMALL)


def sd_spec_for(spec):
    code_dim = getattr(spec, "code_dim", None) or spec.dimension
    return SemanticDecoderSpec(code_dim=code_dim, output_channels=spec.sem_in, decode_channels=spec.sem_ch,
                               channel_ratios=(1,) * len(spec.sem_strides), strides=tuple(spec.sem_strides))


def inputs(version, seed, batch, samples, spec):
    """(state_dict with semantic_decoder.*, wav, feat): the seeds -> tensors rule the GPU test repeats"""
    if version == "2.0":
        sd = synth.hcodec20_state_dict(seed, spec)
        wav = synth.synth_wav_fullband(seed + 1, batch, samples)
        feat = synth.synth_feat(seed + 2, batch, samples // spec.hop, spec.sem_in)
    else:
        sd = synth.hcodec10_state_dict(seed, spec)
        wav = synth.synth_wav(seed + 1, batch, samples)
        feat = synth.synth_feat(seed + 2, batch, samples // 320, spec.sem_in)
    sd.update(hcodec_semantic_decoder_state_dict(seed + 3, sd_spec_for(spec)))
    return sd, wav, feat


def main():
    for name, version, seed, batch, samples in CASES:
        spec = spec_for(version)
        sd, wav, feat = inputs(version, seed, batch, samples, spec)
        model = ref_shim.load_reference_codec(version, spec if version != "1.0" else None)
        missing, unexpected = model.load_state_dict(sd, strict=False)
        assert not missing and not unexpected, (missing, unexpected)
        x = wav if version == "2.0" else wav.unsqueeze(1)
        with torch.no_grad():
            out = model(x, feat)
            enc = model.encode(x, feat)
        rec = {"seed": seed, "batch": batch, "samples": samples}
        if version == "1.5":
            rec.update(recon=out["recon"].numpy(), pred_feat=out["pred_feat"].numpy(), token_lengths=out["token_lengths"].numpy().astype(np.int16),
                       acoustic_codes=enc["acoustic_codes"].numpy().astype(np.int32), semantic_codes=enc["semantic_codes"].numpy().astype(np.int32))
        else:
            rec.update(recon=out[0].numpy(), pred_feat=out[1].numpy(), acoustic_codes=enc[0].numpy().astype(np.int16),
                       semantic_codes=enc[1].numpy().astype(np.int16))
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **rec)
        print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
