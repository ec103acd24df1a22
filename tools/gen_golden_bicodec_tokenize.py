"""Golden tokens of `BiCodec.get_semantic_tokens` / `get_global_tokens` (QuarkAudio-UniSE/model/bicodec/bicodec.py:167-180), produced
by the reference's OWN Encoder / FactorizedVectorQuantize and SpeakerEncoder modules on seeded weights, features and waveforms
(unified_audio_amd/synth.py: the GPU machine regenerates the same inputs from the seeds, so only outputs are stored: the tokens and
the values that decide them for the near-tie audits - the normalised 8-wide latents, the FSQ-bounded values).  The mel spectrogram in
front of the SpeakerEncoder is tests/bicodec_tokenize_ref.mel_spectrogram (torchaudio is not installed; that function is pinned to
transformers.audio_utils by tests/test_bicodec_tokenize_oracle_cpu.py) and is stored too.

Run where the reference tree is present:  python tools/gen_golden_bicodec_tokenize.py
"""
from __future__ import annotations

import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_bicodec_shim as RS  # noqa: E402
from unified_audio_amd import synth  # noqa: E402
from unified_audio_amd.bicodec import BiCodecEncoderSpec  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
SMALL = dict(input_channels=64, vocos_dim=32, vocos_inter=64, vocos_layers=2, latent_dim=64, codebook_size=128, codebook_dim=8)
CASES = {  # name -> (spec kwargs, weight seed, feature seed, batch, frames)
    "bicodec_tokenize_small": (SMALL, 11, 12, 2, 40),
    "bicodec_tokenize_published": ({}, 13, 14, 1, 50),  # the published widths, 1 s of features
}
GLOBAL_CASES = {  # name -> (weight seed, waveform seed, batch, samples of the row, reference clip length)
    "bicodec_tokenize_global_published": (15, 16, 2, 40000, 96000),  # 2.5 s rows tiled into the 6 s clip
}


def global_case_inputs(name):
    seed, wseed, batch, samples, ref_len = GLOBAL_CASES[name]
    spec = BiCodecEncoderSpec()
    return spec, synth.bicodec_speaker_state_dict(seed, spec), synth.synth_wav(wseed, batch, samples), ref_len


def case_inputs(name):
    kw, seed, fseed, batch, frames = CASES[name]
    spec = BiCodecEncoderSpec(**kw)
    sd = synth.bicodec_encoder_state_dict(seed, spec)
    feat = synth.synth_feat(fseed, batch, frames, spec.input_channels).transpose(1, 2).contiguous()  # [B, N, C_in]
    return spec, sd, feat


def main():
    if not RS.reference_available():
        raise SystemExit("the reference tree is needed to generate these goldens")
    enc_mod = RS._import("encoder_decoder.feat_encoder")
    fvq_mod = RS._import("vq.factorized_vector_quantize")
    for name in CASES:
        spec, sd, feat = case_inputs(name)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            enc = enc_mod.Encoder(input_channels=spec.input_channels, vocos_dim=spec.vocos_dim, vocos_intermediate_dim=spec.vocos_inter,
                                  vocos_num_layers=spec.vocos_layers, out_channels=spec.latent_dim, sample_ratios=[1, 1]).eval()
            fvq = fvq_mod.FactorizedVectorQuantize(input_dim=spec.latent_dim, codebook_size=spec.codebook_size,
                                                   codebook_dim=spec.codebook_dim, commitment=0.25).eval()
        enc.load_state_dict({k[len("encoder."):]: v for k, v in sd.items() if k.startswith("encoder.")})
        fvq.load_state_dict({k[len("quantizer."):]: v for k, v in sd.items() if k.startswith("quantizer.")}, strict=False)
        with torch.no_grad():
            z = enc(feat.transpose(1, 2))                                           # bicodec.py:170
            tokens = fvq.tokenize(z)                                                # bicodec.py:171
            latent = torch.nn.functional.normalize(fvq.in_project(z).transpose(1, 2).reshape(-1, spec.codebook_dim))
        path = os.path.join(GOLDEN, name + ".npz")
        np.savez_compressed(path, tokens=tokens.numpy().astype(np.int64), latent=latent.numpy().astype(np.float32))
        print(f"{path}: tokens {tuple(tokens.shape)}, {len(np.unique(tokens.numpy()))} distinct")
    from tests import bicodec_tokenize_ref as T

    spk_mod = RS._import("speaker.speaker_encoder")
    for name in GLOBAL_CASES:
        spec, sd, wav, ref_len = global_case_inputs(name)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            spk = spk_mod.SpeakerEncoder(input_dim=spec.mel_dim, out_dim=1024, latent_dim=spec.spk_latent_dim, token_num=spec.token_num,
                                         fsq_levels=list(spec.fsq_levels), fsq_num_quantizers=1).eval()
        spk.load_state_dict({k[len("speaker_encoder."):]: v for k, v in sd.items()}, strict=False)
        mel = T.mel_spectrogram(T.ref_clip(wav, ref_len).double(), spec.mel_params).float()     # bicodec.py:176
        with torch.no_grad():
            tokens = spk.tokenize(mel)                                                           # bicodec.py:177
            _, feats = spk.speaker_encoder(mel, True)
            z = spk.quantizer.project_in(spk.perceiver_sampler(feats.transpose(1, 2)))
            bounded = spk.quantizer.layers[0].bound(z)
        path = os.path.join(GOLDEN, name + ".npz")
        np.savez_compressed(path, tokens=tokens.numpy().astype(np.int32), bounded=bounded.numpy().astype(np.float32),
                            mel=mel.numpy().astype(np.float32)[:, ::10])
        print(f"{path}: tokens {tuple(tokens.shape)}, {len(np.unique(tokens.numpy()))} distinct")


if __name__ == "__main__":
    main()
