"""tests/bicodec_forward_ref.py (the restatement the GPU tests of BiCodec.forward compare against) pinned to the reference's own modules
(QuarkAudio-UniSE/model/bicodec/modules/*): the x-vector head of ECAPA_TDNN_GLOB_c512, the postnet Decoder, FactorizedVectorQuantize's
code statistics; and the goldens of tools/gen_golden_bicodec_forward.py regenerate identically."""
import importlib.util
import math
import os
import warnings

import numpy as np
import pytest
import torch

from oracle import ref_bicodec_shim as RS
from tests import bicodec_forward_ref as F
from tests import bicodec_tokenize_ref as T

HERE = os.path.dirname(os.path.abspath(__file__))
pytestmark = pytest.mark.skipif(not RS.reference_available(), reason="needs the reference tree")


def _gen():
    spec = importlib.util.spec_from_file_location("gen_golden_bicodec_forward", os.path.join(HERE, "..", "tools", "gen_golden_bicodec_forward.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _speaker(espec, fspec, sd):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        spk = RS._import("speaker.speaker_encoder").SpeakerEncoder(
            input_dim=espec.mel_dim, out_dim=fspec.xvector_dim, latent_dim=espec.spk_latent_dim, token_num=espec.token_num,
            fsq_levels=list(espec.fsq_levels), fsq_num_quantizers=1).eval()
    spk.load_state_dict({k[len("speaker_encoder."):]: v for k, v in sd.items() if k.startswith("speaker_encoder.")})
    return spk


@pytest.mark.parametrize("name", ["bicodec_forward_small", "bicodec_forward_published_1s"])
def test_xvector_head_equals_reference_modules(name):
    """fp32: the same op sequence as ASTP + BatchNorm1d + Linear, so the same bits."""
    gen = _gen()
    dspec, espec, fspec, sd, feat, wav = gen.case_inputs(name)
    mel = T.mel_spectrogram(wav.double(), espec.mel_params).float()
    spk = _speaker(espec, fspec, sd)
    with torch.no_grad():
        x_ref, latent = spk.speaker_encoder(mel, True)
        x = F.x_vector(T.cast(sd, torch.float32), latent.transpose(1, 2))
        x64 = F.x_vector(T.cast(sd), latent.transpose(1, 2).double())
    assert torch.equal(x, x_ref)
    assert float((x.double() - x64).abs().max() / x64.abs().max()) < 1e-5


@pytest.mark.parametrize("tanh", [False, True])
def test_postnet_matches_reference_decoder(tanh):
    gen = _gen()
    dspec, espec, fspec, sd, feat, wav = gen.case_inputs("bicodec_forward_small")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        post = RS._import("encoder_decoder.feat_decoder").Decoder(
            input_channels=fspec.input_channels, vocos_dim=fspec.vocos_dim, vocos_intermediate_dim=fspec.vocos_inter,
            vocos_num_layers=fspec.vocos_layers, out_channels=fspec.out_channels, use_tanh_at_final=tanh).eval()
    post.load_state_dict({k[len("postnet."):]: v for k, v in sd.items() if k.startswith("postnet.")})
    x = torch.randn(3, fspec.input_channels, 17, generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        want = post(x)
        got = F.postnet(T.cast(sd, torch.float32), x, fspec.vocos_layers, tanh)
        got64 = F.postnet(T.cast(sd), x.double(), fspec.vocos_layers, tanh)
    # oracle.bicodec_ref.vocos_backbone restates VocosBackbone with functional ops (the SamplingBlock's 3 x is one product here)
    assert float((got - want).abs().max() / want.abs().max()) < 1e-5
    assert float((want.double() - got64).abs().max() / got64.abs().max()) < 1e-5


def test_code_statistics_equal_reference_forward():
    """FactorizedVectorQuantize.forward in eval: perplexity and active_num over the whole batch, vq_loss a 0-dim NaN."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        fvq = RS._import("vq.factorized_vector_quantize").FactorizedVectorQuantize(
            input_dim=64, codebook_size=128, codebook_dim=8, commitment=0.25).eval()
    z = torch.randn(2, 64, 40, generator=torch.Generator().manual_seed(9))
    with torch.no_grad():
        out = fvq(z)
    p32, a32 = F.code_stats(out["indices"], 128, torch.float32)
    assert torch.equal(p32, out["perplexity"]) and torch.equal(a32, out["active_num"])
    assert out["vq_loss"].dim() == 0 and math.isnan(float(out["vq_loss"]))
    exact = F.perplexity_exact(out["indices"], 128)
    assert abs(float(out["perplexity"]) - exact) <= 1e-6 * exact
    per_item = [F.perplexity_exact(out["indices"][i], 128) for i in range(2)]
    assert all(abs(p - exact) > 1e-3 * exact for p in per_item)  # batch-level, not an average of per-item values


def test_goldens_regenerate_identically():
    gen = _gen()
    for name in gen.CASES:
        dspec, espec, fspec, sd, feat, wav = gen.case_inputs(name)
        mel = T.mel_spectrogram(wav.double(), espec.mel_params).float()
        out = gen.reference_forward(dspec, espec, fspec, sd, feat, mel)
        g = np.load(os.path.join(HERE, "golden", name + ".npz"))
        assert np.array_equal(g["semantic_tokens"], out["semantic_tokens"].numpy())
        assert np.array_equal(g["global_tokens"], out["global_tokens"].numpy().reshape(wav.shape[0], -1))
        for k in ("recons", "x_vector", "d_vector"):
            assert np.array_equal(g[k], out[k].numpy()), k
        assert np.array_equal(g["pred_feat"], out["pred_feat"][:, ::gen.PRED_STRIDE].numpy())
        assert float(g["perplexity"]) == float(out["perplexity"]) and float(g["cluster_size"]) == float(out["cluster_size"])
        assert os.path.getsize(os.path.join(HERE, "golden", name + ".npz")) < 128 * 1024
