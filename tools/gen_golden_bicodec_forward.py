"""Golden outputs of `BiCodec.forward` (QuarkAudio-UniSE/model/bicodec/bicodec.py:113-149, eval mode), produced by the reference's OWN
modules - Encoder, FactorizedVectorQuantize.forward, SpeakerEncoder.forward (ECAPA-TDNN with its ASTP / BatchNorm / Linear head), the
prenet and postnet Decoders and the WaveGenerator - assembled as bicodec.py:123-137 assembles them, on seeded weights, features and
waveforms (unified_audio_amd/synth.py: the GPU machine regenerates the same inputs from the seeds, so only outputs are stored).  The mel
spectrogram is tests/bicodec_tokenize_ref.mel_spectrogram (torchaudio is not installed), as for the tokenize goldens.

The small case narrows the postnet and the encoder with the prenet (tests/ref_configs.small_bicodec_config keeps a 1024-wide postnet
input, which a 64-wide prenet cannot feed).

Run where the reference tree is present:  python tools/gen_golden_bicodec_forward.py
"""
from __future__ import annotations

import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from unified_audio_amd import synth  # noqa: E402
from unified_audio_amd.bicodec import BiCodecEncoderSpec, BiCodecForwardSpec, BiCodecSpec  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
SMALL_ENC = dict(input_channels=64, vocos_dim=32, vocos_inter=64, vocos_layers=2, latent_dim=64, codebook_size=128, codebook_dim=8,
                 spk_latent_dim=32, token_num=4)
SMALL_DEC = dict(latent_dim=64, codebook_size=128, codebook_dim=8, spk_latent_dim=32, token_num=4, vocos_dim=32, vocos_inter=64,
                 vocos_layers=2, gen_channels=256, rates=(4, 5, 2), kernel_sizes=(8, 11, 4))
SMALL_FWD = dict(input_channels=64, vocos_dim=32, vocos_inter=64, vocos_layers=2, out_channels=64, xvector_dim=64)
CASES = {  # name -> (small?, weight seed, batch, feature frames N, reference samples)
    "bicodec_forward_small": (True, 31, 2, 20, 12000),
    "bicodec_forward_published_1s": (False, 41, 1, 50, 16000),
}
PRED_STRIDE = 4  # pred_feat is stored every 4th channel (the published 1024 x 50 block alone would be 200 KB)


def specs(small: bool):
    if small:
        return BiCodecSpec(**SMALL_DEC), BiCodecEncoderSpec(**SMALL_ENC), BiCodecForwardSpec(**SMALL_FWD)
    return BiCodecSpec(), BiCodecEncoderSpec(), BiCodecForwardSpec()


def case_inputs(name):
    small, seed, B, N, samples = CASES[name]
    dspec, espec, fspec = specs(small)
    sd = synth.bicodec_state_dict(seed, dspec)
    sd.update(synth.bicodec_encoder_state_dict(seed + 1, espec))
    sd.update(synth.bicodec_speaker_state_dict(seed + 2, espec))
    sd.update(synth.bicodec_forward_state_dict(seed + 3, fspec))
    feat = synth.synth_feat(seed + 4, B, N, espec.input_channels).transpose(1, 2).contiguous()  # [B, N, C_in]
    wav = synth.synth_wav(seed + 5, B, samples)
    return dspec, espec, fspec, sd, feat, wav


def sub(sd, prefix):
    return {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}


def reference_forward(dspec, espec, fspec, sd, feat, mel):
    """bicodec.py:123-149 with the reference's own modules; mel [B, frames, n_mels] is the (transposed) mel_transformer output."""
    from oracle import ref_bicodec_shim as RS

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        enc = RS._import("encoder_decoder.feat_encoder").Encoder(
            input_channels=espec.input_channels, vocos_dim=espec.vocos_dim, vocos_intermediate_dim=espec.vocos_inter,
            vocos_num_layers=espec.vocos_layers, out_channels=espec.latent_dim, sample_ratios=[1, 1]).eval()
        fvq = RS._import("vq.factorized_vector_quantize").FactorizedVectorQuantize(
            input_dim=espec.latent_dim, codebook_size=espec.codebook_size, codebook_dim=espec.codebook_dim, commitment=0.25).eval()
        spk = RS._import("speaker.speaker_encoder").SpeakerEncoder(
            input_dim=espec.mel_dim, out_dim=fspec.xvector_dim, latent_dim=espec.spk_latent_dim, token_num=espec.token_num,
            fsq_levels=list(espec.fsq_levels), fsq_num_quantizers=1).eval()
        dec_mod = RS._import("encoder_decoder.feat_decoder")
        prenet = dec_mod.Decoder(input_channels=dspec.latent_dim, vocos_dim=dspec.vocos_dim, vocos_intermediate_dim=dspec.vocos_inter,
                                 vocos_num_layers=dspec.vocos_layers, out_channels=dspec.latent_dim, condition_dim=dspec.latent_dim,
                                 sample_ratios=[1, 1], use_tanh_at_final=False).eval()
        postnet = dec_mod.Decoder(input_channels=fspec.input_channels, vocos_dim=fspec.vocos_dim, vocos_intermediate_dim=fspec.vocos_inter,
                                  vocos_num_layers=fspec.vocos_layers, out_channels=fspec.out_channels,
                                  use_tanh_at_final=fspec.use_tanh_at_final).eval()
        decoder = RS._import("encoder_decoder.wave_generator").WaveGenerator(
            input_channel=dspec.latent_dim, channels=dspec.gen_channels, rates=list(dspec.rates), kernel_sizes=list(dspec.kernel_sizes)).eval()
    enc.load_state_dict(sub(sd, "encoder."))
    missing, unexpected = fvq.load_state_dict(sub(sd, "quantizer."), strict=False)
    assert missing == ["cluster_size"] and not unexpected, (missing, unexpected)
    spk.load_state_dict(sub(sd, "speaker_encoder."))
    prenet.load_state_dict(sub(sd, "prenet."))
    postnet.load_state_dict(sub(sd, "postnet."))
    decoder.load_state_dict(sub(sd, "decoder."))
    with torch.no_grad():
        z = enc(feat.transpose(1, 2))                                            # bicodec.py:126
        vq = fvq(z)                                                              # :127
        x_vector, d_vector = spk(mel)                                            # :129 (mel already [B, frames, n_mels])
        x = prenet(vq["z_q"], d_vector)                                          # :134
        pred = postnet(x)                                                        # :135
        recons = decoder(x + d_vector.unsqueeze(-1))                             # :136-137
        glob = spk.tokenize(mel)                                                 # the global tokens detokenize would take
    return {"vq_loss": vq["vq_loss"], "perplexity": vq["perplexity"], "cluster_size": vq["active_num"], "recons": recons,
            "pred_feat": pred, "x_vector": x_vector, "d_vector": d_vector, "semantic_tokens": vq["indices"], "global_tokens": glob}


def main():
    from oracle import ref_bicodec_shim as RS
    from tests import bicodec_tokenize_ref as T

    if not RS.reference_available():
        raise SystemExit("the reference tree is needed to generate these goldens")
    for name in CASES:
        dspec, espec, fspec, sd, feat, wav = case_inputs(name)
        mel = T.mel_spectrogram(wav.double(), espec.mel_params).float()
        out = reference_forward(dspec, espec, fspec, sd, feat, mel)
        assert torch.isnan(out["vq_loss"]) and out["vq_loss"].dim() == 0
        path = os.path.join(GOLDEN, name + ".npz")
        np.savez_compressed(path, semantic_tokens=out["semantic_tokens"].numpy().astype(np.int64),
                            global_tokens=out["global_tokens"].numpy().astype(np.int64).reshape(wav.shape[0], -1),
                            recons=out["recons"].numpy().astype(np.float32),
                            pred_feat=out["pred_feat"][:, ::PRED_STRIDE].numpy().astype(np.float32),
                            x_vector=out["x_vector"].numpy().astype(np.float32), d_vector=out["d_vector"].numpy().astype(np.float32),
                            perplexity=np.float32(out["perplexity"]), cluster_size=np.float32(out["cluster_size"]))
        print(f"{path}: {os.path.getsize(path)} bytes, perplexity {float(out['perplexity']):.3f}, cluster_size "
              f"{float(out['cluster_size']):.0f}, {len(np.unique(out['global_tokens'].numpy()))} distinct global tokens")


if __name__ == "__main__":
    main()
