"""Every model handle refuses a weight table with a required tensor missing: its create returns QA_ERR_MISSING (QuarkAudioError -3)
naming the tensor, frees what it had built, and a create from the full table afterwards loads and runs one small call."""
import dataclasses

import pytest
import torch

from oracle import hcodec_ref as R
from oracle import llm_ref as LR
from oracle import ssl_ref as S
from oracle import synth as osynth
from tests.test_bicodec_tokenize_gpu import SMALL as BICODEC_SMALL
from tests.test_bicodec_tokenize_gpu import _dspec, _full_sd
from tests.test_llm_gpu import SMALL as LM_SMALL
from tests.test_mimi_stream_cpu import D, FF, H, L
from tests.util import MINI
from unified_audio_amd import synth

pytestmark = pytest.mark.gpu
QA_ERR_MISSING = -3


def _without(sd, key):
    assert key in sd, key
    return {k: v for k, v in sd.items() if k != key}


def _refused(load, sd, key, named=None):
    from unified_audio_amd import QuarkAudioError

    with pytest.raises(QuarkAudioError) as e:
        load(_without(sd, key))
    assert e.value.status == QA_ERR_MISSING
    assert (named or key) in str(e.value)


def test_hcodec_missing_tensor(qa_lib, gpu_device):
    import unified_audio_amd as qa

    ospec = R.HCodecSpec(**MINI)
    sd = osynth.hcodec10_state_dict(9, ospec)
    load = lambda d: qa.Codec(None, None, None, spec=qa.HCodecSpec(**MINI), device=gpu_device).load_state_dict(d)  # noqa: E731
    _refused(load, sd, "encoder.model.1.block.1.conv.conv.weight_v")  # a weight-normed SEANet convolution
    _refused(load, sd, "semantic_encoder.conv.conv.weight")           # a plain one
    T = 640
    wav = osynth.synth_wav(10, 1, T).to(gpu_device).unsqueeze(1)
    feat = osynth.synth_feat(11, 1, T // (ospec.enc_hop // 2), ospec.sem_in).to(gpu_device)
    ac, sc = load(sd).encode(wav, feat)
    torch.cuda.synchronize()
    assert ac.shape == sc.shape and ac.shape[0] == 1


def test_mimi_missing_tensor(qa_lib, gpu_device):
    import unified_audio_amd as qa

    sd = osynth.mimi_state_dict(31, D, L, FF)
    load = lambda d: qa.StreamingTransformer(D, H, L, FF, device=gpu_device, prefix="transformer").load_state_dict(d)  # noqa: E731
    _refused(load, sd, "transformer.layers.0.linear1.weight", named="layers.0.linear1.weight")
    y = load(sd)(torch.randn(1, 8, D, generator=torch.Generator().manual_seed(3)).to(gpu_device))
    assert y.shape == (1, 8, D) and torch.isfinite(y).all()


def test_ssl_missing_tensor(qa_lib, gpu_device):
    import unified_audio_amd as qa

    ospec = S.SSLSpec(conv_dim=(64,) * 7, hidden_size=96, num_hidden_layers=2, num_attention_heads=3, intermediate_size=192,
                      num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=2)
    sd = S.synth_state_dict(3, ospec, "hubert")
    kw = {f.name: getattr(ospec, f.name) for f in dataclasses.fields(ospec)}
    load = lambda d: qa.SSLFeatureExtractor(qa.SSLSpec(**kw), device=gpu_device).load_state_dict(d)  # noqa: E731
    _refused(load, sd, "encoder.layers.1.feed_forward.output_dense.weight")
    _refused(load, sd, "encoder.layers.0.attention.k_proj.bias")
    fx = load(sd)
    got = fx(torch.randn(1, 4000, generator=torch.Generator().manual_seed(4)).to(gpu_device))
    assert got.shape == (1, fx.frames(4000), ospec.hidden_size) and torch.isfinite(got).all()


def test_bicodec_missing_tensor(qa_lib, gpu_device):
    import unified_audio_amd as qa

    espec = qa.BiCodecEncoderSpec(**BICODEC_SMALL)
    sd = _full_sd(espec, 41)
    load = lambda d: qa.BiCodec(_dspec(espec), device=gpu_device, encoder_spec=espec).load_state_dict(d)  # noqa: E731
    _refused(load, sd, "prenet.linear_pre.bias")          # the detokenizer (qa_bicodec_create)
    _refused(load, sd, "quantizer.in_project.bias")       # the tokenizer (qa_bicodec_enc_create)
    m = load(sd)
    sem, glob = synth.bicodec_tokens(42, 1, 6, _dspec(espec))
    wav = m.detokenize(sem.to(gpu_device), glob.to(gpu_device))
    feat = synth.synth_feat(43, 1, 9, espec.input_channels).transpose(1, 2).contiguous().to(gpu_device)
    tokens = m.get_semantic_tokens({"feat": feat})
    torch.cuda.synchronize()
    assert torch.isfinite(wav).all() and tokens.shape == (1, 9)


def test_lm_missing_tensor(qa_lib, gpu_device):
    import unified_audio_amd as qa

    spec = LM_SMALL
    sd = LR.lm_state_dict(21, spec)
    cfg = dict(global_size=spec.global_size, semantic_size=spec.semantic_size, hidden_size=spec.hidden, num_layers=spec.n_layers,
               num_attention_heads=spec.n_heads)
    load = lambda d: qa.LLM_SFT(num_tasks=spec.num_tasks, feats_dim=spec.feats_dim, llm_base_config=cfg,  # noqa: E731
                                device=gpu_device).load_state_dict(d)
    _refused(load, sd, "layers.1.mlp.down_proj.weight")
    _refused(load, sd, "norm.weight")
    mix = LR.synth_feats(1, 2, 5, spec.feats_dim).to(gpu_device)
    mel = torch.zeros(2, 4, 80)
    gids, sids = load(sd).generate("se", None, None, mel, mix, global_length=3, do_sample=False)
    assert gids.shape == (2, 3) and sids.shape == (2, 4)
