"""The CPU restatement of the condition path (tests/conformer_ref.py) against the reference's OWN modules (skipped where the reference
tree is absent, like the other pin tests): ConformerEncoder with and without a mask and partial RoPE, Model.stft_logmel (the reference's
own function; its filter bank call goes to oracle/stubs/torchaudio), CustomLlamaModel.forward and greedy generate with and without a
condition - and against the committed goldens those classes produced (tests/golden/lm_cond_*.npz), which travel where the tree does not.  The reference imports `x_transformers`, which is not
available offline: tests/conformer_ref.py's restatement of its two symbols [upstream-memory] is injected first."""
from __future__ import annotations

import math

import numpy as np
import pytest
import torch

from oracle import llm_ref as L
from oracle import ref_llm_shim as S
from tests import conformer_ref as R
from tests.test_llm_gpu import SMALL
from unified_audio_amd import synth

needs_ref = pytest.mark.skipif(not S.reference_available(), reason="reference tree not present")

CF = dict(num_layers=2, dim=64, heads=2, dim_head=32, depthwise_conv_kernel_size=31, ff_mult=2, dropout=0.1, qk_norm=None, pe_attn_head=None)


def _ref_module():
    import importlib

    R.install_x_transformers()
    mod = S._import_llm_sft()
    # another test may have imported the reference package first, with oracle/stubs' raising stand-ins bound into conformer.py
    conf = importlib.import_module("model.llm.conformer")
    conf.RotaryEmbedding, conf.apply_rotary_pos_emb = R.RotaryEmbedding, R.apply_rotary_pos_emb
    return mod


def _ref_encoder(params, sd):
    import importlib

    _ref_module()
    conf = importlib.import_module("model.llm.conformer")
    enc = conf.ConformerEncoder(**params).eval()
    missing, unexpected = enc.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.startswith("rotary_embedding") for k in missing), (missing, unexpected)
    return enc


@needs_ref
@pytest.mark.parametrize("pe", [None, 1])
@pytest.mark.parametrize("masked", [False, True])
def test_conformer_restatement_equals_reference(pe, masked):
    params = dict(CF, pe_attn_head=pe)
    sd = synth.conformer_state_dict(31, params)
    enc = _ref_encoder(params, sd)
    x = torch.from_numpy(np.random.default_rng(3).standard_normal((3, 50, 64)).astype("float32"))
    mask = None
    if masked:
        mask = torch.arange(50)[None, :] < torch.tensor([50, 33, 41])[:, None]
    with torch.no_grad():
        want = enc(x.clone(), mask=mask)
    got = R.conformer_encoder(sd, params, x, mask)
    assert (got - want).abs().max() <= 2e-5 * want.abs().max()
    # the float64 restatement is the same function
    assert (R.conformer_encoder(sd, params, x, mask, dtype=torch.float64) - want.double()).abs().max() <= 1e-4 * want.abs().max()


def test_even_kernel_is_refused_like_the_reference():
    with pytest.raises(ValueError, match="must be odd"):
        R.conformer_encoder({}, dict(CF, depthwise_conv_kernel_size=30), torch.zeros(1, 4, 64))


def test_synth_batchnorm_statistics_are_not_trivial():
    sd = synth.conformer_state_dict(1, CF)
    assert sd["layers.0.conv_module.sequential.3.running_mean"].abs().max() > 0.05
    assert (sd["layers.0.conv_module.sequential.3.running_var"] - 1).abs().max() > 0.1


def test_logmel_restatement_float32_equals_product_cpu_path():
    from unified_audio_amd import unise

    wav = synth.synth_wav(5, 2, 16123)
    a, b = R.stft_logmel(wav), unise.stft_logmel(wav)
    assert a.shape == b.shape == (2, unise.mel_frames(16123), 80)
    assert (a - b).abs().max() <= 1e-4
    assert (R.stft_logmel(torch.zeros(1, 3200)) - math.log(1e-10)).abs().max() <= 1e-6


def _ref_custom(spec, params, sd, eps=0.1):
    mod = _ref_module()
    import importlib

    llm = importlib.import_module("model.llm.llm")
    model = llm.CustomLlamaModel(cond_dim=80, global_size=spec.global_size, semantic_size=spec.semantic_size, hidden_size=spec.hidden,
                                 num_layers=spec.n_layers, num_attention_heads=spec.n_heads, label_smoothing=eps, conformer_params=params)
    for layer in model.layers:
        S._patch_layer(layer)
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected, unexpected
    assert all(k.startswith("rotary_emb.") or "rotary_embedding" in k for k in missing), missing
    return model.eval()


def _weights(spec, params, seed, gain=2.0):
    sd = {k: v for k, v in L.lm_state_dict(seed, spec).items() if not k.startswith(("task_embedding", "enroll_sos", "adapter"))}
    sd.update(synth.cond_encoder_state_dict(seed + 1, 80, spec.hidden, params, gain))
    return sd


@needs_ref
@pytest.mark.parametrize("with_cond", [True, False])
def test_custom_llama_restatement_equals_reference(with_cond):
    sd = _weights(SMALL, CF, 71)
    model = _ref_custom(SMALL, CF, sd)
    G, T = 6, 11
    gen = torch.Generator().manual_seed(17)
    g = torch.randint(0, SMALL.global_size, (1, G), generator=gen)
    s = torch.randint(0, SMALL.semantic_size, (1, T), generator=gen)
    cond = synth.synth_logmel(13, 1, 18) if with_cond else None
    with torch.no_grad():
        loss, acc = model(g, s, cond)
        gi, si = model.generate(cond, global_length=G, semantic_length=T, do_sample=False)
    r = R.score(sd, SMALL, CF, g, s, cond, 0.1)
    assert abs(float(loss) - r["loss"]) <= 2e-5 * abs(r["loss"])
    assert abs(float(acc) - r["acc"]) < 1e-6
    g_o, s_o, _, gaps = R.generate(sd, SMALL, CF, cond, G, T, 1)
    assert gaps.min() > 2e-4
    assert torch.equal(gi, g_o) and torch.equal(si, s_o)


def test_condition_changes_the_greedy_stream():
    """with the synthetic gains the conditional stream differs from the unconditional one: a path that ignored `cond` cannot pass"""
    sd = _weights(SMALL, CF, 71)
    cond = synth.synth_logmel(11, 3, 20)
    a = R.generate(sd, SMALL, CF, cond, 6, 14)
    b = R.generate(sd, SMALL, CF, None, 6, 14, batch_size=3)
    assert not (torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]))


# ------------------------------------------------------------------------------- committed goldens (tools/gen_golden_lm_cond.py)

def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().pow(2).mean().sqrt())


@pytest.mark.parametrize("name", list(R.CONFORMER_CASES))
def test_restatement_equals_conformer_golden(name):
    params, sd, x, mask = R.golden_conformer_case(name)
    golden = R.load_golden("lm_cond_conformer")[name]
    assert _rel(R.conformer_encoder(sd, params, x, mask), golden) <= 2e-5
    assert _rel(R.conformer_encoder(sd, params, x, mask, dtype=torch.float64), golden) <= 2e-5
    if name != "pe_none":  # partial RoPE and the mask are visible in the golden
        assert _rel(R.conformer_encoder(sd, dict(params, pe_attn_head=None), x, None), golden) > 1e-3


def test_restatement_equals_logmel_golden():
    """lm_cond_logmel.npz is Model.stft_logmel's own output (model.py:53-79: padding, STFT, window, log; the filter bank call goes to
    oracle/stubs/torchaudio, torchaudio itself is not available offline)"""
    wav = R.golden_logmel_wav()
    golden = R.load_golden("lm_cond_logmel")["logmel"]
    got = R.stft_logmel(wav)
    assert got.shape == golden.shape == (3, 51, 80)
    assert _rel(got, golden) <= 2e-4  # float32 against float32 through a log: e_cpu32 of the GPU test is of this size
    assert _rel(R.stft_logmel(wav, dtype=torch.float64), golden) <= 2e-4
    assert (golden[1, 11:27] - math.log(1e-10)).abs().max() <= 1e-5  # frames inside the all-zero stretch 3000 .. 9000


@needs_ref
def test_logmel_restatement_equals_reference_function():
    import types

    from oracle import ref_unise_shim as U

    mod = U._import_model_module()
    me = types.SimpleNamespace(stft_conf=dict(hop_length=320, win_length=640, n_fft=640, n_mels=80))
    for n in (16000, 16123, 4001):
        wav = synth.synth_wav(9, 2, n)
        want = mod.Model.stft_logmel(me, wav)
        got = R.stft_logmel(wav)
        assert got.shape == want.shape
        assert _rel(got, want) <= 2e-4


def test_restatement_equals_generate_and_forward_goldens():
    gold = R.load_golden("lm_cond_generate")
    assert float(gold["cond_gap"].min()) > 2e-4 and float(gold["nocond_gap"].min()) > 2e-4  # no near-tie: streams must be identical
    sd, spec, params = R.golden_lm_weights(), R.GOLDEN_SPEC, R.GOLDEN_CF
    cond, g, s = R.golden_lm_inputs()
    gi, si, _, _ = R.generate(sd, spec, params, cond, R.GOLDEN_G, R.GOLDEN_S)
    assert torch.equal(gi, gold["cond_global"].long()) and torch.equal(si, gold["cond_semantic"].long())
    g0, s0, _, _ = R.generate(sd, spec, params, None, R.GOLDEN_G, R.GOLDEN_S, 1)
    assert torch.equal(g0, gold["nocond_global"].long()) and torch.equal(s0, gold["nocond_semantic"].long())
    for b in range(R.GOLDEN_B):  # a path that ignored `cond` cannot reproduce the conditional golden
        assert not (torch.equal(gold["cond_global"][b], gold["nocond_global"][0]) and torch.equal(gold["cond_semantic"][b], gold["nocond_semantic"][0]))
    fwd = R.load_golden("lm_cond_forward")
    for name, (with_cond, eps) in R.FORWARD_CASES.items():
        r = R.score(sd, spec, params, g, s, cond if with_cond else None, eps)
        assert abs(r["loss"] - float(fwd[name + "_loss"])) <= 2e-5 * abs(r["loss"]), name
        assert abs(r["acc"] - float(fwd[name + "_acc"])) < 1e-6, name
    assert abs(float(fwd["cond_eps01_loss"]) - float(fwd["nocond_eps01_loss"])) > 1e-3
