"""Pins the CPU restatement of Codec.forward (tests/hcodec_forward_ref.py) to the reference's OWN Codec.forward (recon, pred_feat,
commit_loss, token_lengths) for H-Codec 1.0, 1.5 and 2.0, and the synthetic semantic-decoder weights / SemanticDecoderSpec to the
reference's module and YAML configurations.  Live where the reference tree is mounted."""
import dataclasses
import os

import pytest
import torch

from oracle import hcodec_ref as R
from oracle import ref_shim, synth
from tests import hcodec_forward_ref as F

live = pytest.mark.skipif(not ref_shim.reference_available(), reason="/root/reference is only mounted in the build container")
REF = os.path.join(ref_shim.REFERENCE_ROOT, "QuarkAudio-HCodec")


def _sds(spec):
    from unified_audio_amd.hcodec import SemanticDecoderSpec

    return SemanticDecoderSpec(code_dim=spec.code_dim if hasattr(spec, "code_dim") else spec.dimension, output_channels=spec.sem_in,
                               decode_channels=spec.sem_ch, channel_ratios=(1,) * len(spec.sem_strides), strides=tuple(spec.sem_strides))


def _with_semdec(model, sd, sds, seed):
    """the synth codec weights + synth semantic decoder weights, loaded strictly into the reference module"""
    from unified_audio_amd.synth import hcodec_semantic_decoder_state_dict

    full = dict(sd)
    full.update(hcodec_semantic_decoder_state_dict(seed, sds))
    ref_sd = model.state_dict()
    got = {k: tuple(v.shape) for k, v in full.items() if k.startswith("semantic_decoder.")}
    want = {k: tuple(v.shape) for k, v in ref_sd.items() if k.startswith("semantic_decoder.")}
    assert got == want, set(got) ^ set(want)
    missing, unexpected = model.load_state_dict(full, strict=False)
    assert not missing and not unexpected, (missing, unexpected)
    return full


def _close(a, b, tol):
    a, b = a.double(), b.double()
    return float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


@live
def test_forward10_matches_reference():
    spec = R.SPEC_10
    sd = synth.hcodec10_state_dict(9101, spec)
    model = ref_shim.load_reference_codec("1.0")
    full = _with_semdec(model, sd, _sds(spec), 9102)
    wav = synth.synth_wav(9103, 2, 640 * 5)
    feat = synth.synth_feat(9104, 2, wav.shape[-1] // 320, spec.sem_in)
    with torch.no_grad():
        recon_r, pred_r, loss_r = model(wav.unsqueeze(1), feat)
        recon, pred, loss, (ac, sc) = F.forward10(full, wav, feat, spec, _sds(spec))
        ac_r, sc_r = model.encode(wav.unsqueeze(1), feat)
    assert torch.equal(ac, ac_r) and torch.equal(sc, sc_r)
    assert recon.shape == recon_r.shape == (2, 640 * 5) and pred.shape == pred_r.shape == (2, 768, 10)
    assert loss_r.dim() == 0 and float(loss_r) == 0.0 == float(loss)
    assert _close(recon, recon_r, 1e-5) and _close(pred, pred_r, 1e-5)
    # fp64 restatement on the same codes: the fp32 one is within fp32 round-off of it
    pred64 = F.pred_feat(full, sc, spec.num_quantizers, _sds(spec), torch.float64)
    assert _close(pred, pred64, 1e-5)


@live
def test_forward15_matches_reference():
    spec = dataclasses.replace(R.SPEC_15, agg_layers=2, bt_layers=2, threshold=0.7)
    sd = synth.hcodec10_state_dict(9201, spec)
    model = ref_shim.load_reference_codec("1.5", spec)
    full = _with_semdec(model, sd, _sds(spec), 9202)
    wav = synth.synth_wav(9203, 2, 640 * 9)
    feat = synth.synth_feat(9204, 2, wav.shape[-1] // 320, spec.sem_in)
    with torch.no_grad():
        ref = model(wav.unsqueeze(1), feat)
        mine, (ac, sc) = F.forward15(full, wav.unsqueeze(1), feat, spec, _sds(spec))
        enc = model.encode(wav.unsqueeze(1), feat)
    assert set(ref) == set(mine) == {"recon", "pred_feat", "commit_loss", "token_lengths"}
    assert torch.equal(ac, enc["acoustic_codes"]) and torch.equal(sc, enc["semantic_codes"])
    assert torch.equal(mine["token_lengths"], ref["token_lengths"]) and ref["token_lengths"].dtype == torch.int64
    assert mine["pred_feat"].shape == ref["pred_feat"].shape == (2, 1024, 18)
    assert ref["commit_loss"].dim() == 0 and float(ref["commit_loss"]) == 0.0
    assert _close(mine["recon"], ref["recon"], 1e-5) and _close(mine["pred_feat"], ref["pred_feat"], 1e-5)


@live
def test_forward20_matches_reference():
    from oracle import hcodec20_ref as R20
    from oracle.gen_golden import SPEC20_SMALL

    spec = R20.HCodec20Spec(**SPEC20_SMALL)
    sd = synth.hcodec20_state_dict(9301, spec)
    model = ref_shim.load_reference_codec("2.0", spec)
    full = _with_semdec(model, sd, _sds(spec), 9302)
    wav = synth.synth_wav_fullband(9303, 2, 3840 * 3)
    feat = synth.synth_feat(9304, 2, wav.shape[-1] // spec.hop, spec.sem_in)
    with torch.no_grad():
        recon_r, pred_r, loss_r = model(wav, feat)
        recon, pred, loss, _ = F.forward20(full, wav, feat, spec, _sds(spec))
    assert pred.shape == pred_r.shape == (2, spec.sem_in, 3 * 4) and recon.shape == recon_r.shape
    assert float(loss_r) == 0.0 and loss_r.dim() == 0
    assert _close(recon, recon_r, 1e-5) and _close(pred, pred_r, 1e-5)


@live
def test_semantic_decoder_matches_reference_module_at_other_widths():
    """A reduced width / odd channel ratios through the reference's OWN Decoder class (the way ref_shim.make_causal_10 swaps modules),
    including the widths the codec spec cannot express."""
    from unified_audio_amd.hcodec import SemanticDecoderSpec

    model = ref_shim.load_reference_codec("1.0")
    cls = type(model.semantic_decoder)
    for sds in (SemanticDecoderSpec(code_dim=64, output_channels=96, decode_channels=128, channel_ratios=(1, 1), strides=(2, 1)),
                SemanticDecoderSpec(code_dim=64, output_channels=32, decode_channels=64, channel_ratios=(2, 1, 1), strides=(2, 4, 1))):
        dec = cls(code_dim=sds.code_dim, output_channels=sds.output_channels, decode_channels=sds.decode_channels,
                  channel_ratios=sds.channel_ratios, strides=sds.strides).eval()
        from unified_audio_amd.synth import hcodec_semantic_decoder_state_dict

        sd = hcodec_semantic_decoder_state_dict(9401, sds)
        dec.load_state_dict({k[len("semantic_decoder."):]: v for k, v in sd.items()}, strict=True)
        z = torch.randn(2, sds.code_dim, 5, generator=torch.Generator().manual_seed(3))
        with torch.no_grad():
            want = dec(z)
            got = F.semantic_decoder(sd, z, sds)
        assert got.shape == want.shape and _close(got, want, 1e-5)


@live
def test_semantic_decoder_spec_from_the_reference_configs():
    import yaml

    import unified_audio_amd as qa
    from unified_audio_amd.hcodec import SemanticDecoderSpec, _semantic_decoder_spec_from_config

    c15 = yaml.safe_load(open(os.path.join(REF, "HCodec-1.5", "conf", "config_adaptive_v3.yaml")))
    c20 = yaml.safe_load(open(os.path.join(REF, "HCodec-2.0", "conf", "large_12.5hz_config.yaml")))
    assert _semantic_decoder_spec_from_config(c15) == SemanticDecoderSpec.from_codec_spec(qa.SPEC_15)
    assert _semantic_decoder_spec_from_config(c20) == SemanticDecoderSpec.from_codec_spec(qa.SPEC_20)
    # codec.py:130-136 hard-codes 1.0's
    assert SemanticDecoderSpec() == SemanticDecoderSpec.from_codec_spec(qa.SPEC_10)
    m20 = qa.Codec(c20["encoder_config"], c20["decoder_config"], c20["quantizer_config"], c20["semantic_encoder_config"],
                   c20["semantic_decoder_config"])
    m15 = qa.Codec(c15["encoder_config"], c15["decoder_config"], c15["quantizer_config"], c15["adaptive_config"])
    assert m20.semantic_decoder_spec == SemanticDecoderSpec.from_codec_spec(qa.SPEC_20)
    assert m15.semantic_decoder_spec == SemanticDecoderSpec.from_codec_spec(qa.SPEC_15) and not m15.dynamic_threshold


def test_synth_semantic_decoder_shapes_and_stream():
    """Parameter counts of the shipped configurations, and a generator of its own: the codec streams do not change."""
    import unified_audio_amd as qa
    from unified_audio_amd.hcodec import SemanticDecoderSpec
    from unified_audio_amd.synth import hcodec_semantic_decoder_state_dict

    n10 = sum(v.numel() for v in hcodec_semantic_decoder_state_dict(1, SemanticDecoderSpec.from_codec_spec(qa.SPEC_10)).values())
    assert n10 == 16_516_608  # the 16.5 M of a real 1.0 checkpoint
    a = hcodec_semantic_decoder_state_dict(5, SemanticDecoderSpec(code_dim=64, output_channels=64, decode_channels=64))
    b = hcodec_semantic_decoder_state_dict(5, SemanticDecoderSpec(code_dim=64, output_channels=64, decode_channels=64))
    assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)
    assert all(k.startswith("semantic_decoder.") for k in a)
