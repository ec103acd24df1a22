"""GPU tests of the UniSE condition path: log-mel front, ConformerEncoder / condition encoder, CustomLlamaModel.generate / forward.

Metric and margin: e = max|y - y64| / rms(y64) against the float64 restatement (tests/conformer_ref.py), bound
4 * max(e_cpu32, 1e-6) where e_cpu32 is the error of the float32 CPU restatement (the reference's arithmetic) on the same input."""
from __future__ import annotations

import pytest
import torch

from oracle import llm_ref as L
from tests import conformer_ref as R
from tests.test_llm_gpu import SMALL
from unified_audio_amd import synth

pytestmark = pytest.mark.gpu

SMALL_CF = dict(num_layers=2, dim=64, heads=2, dim_head=32, depthwise_conv_kernel_size=31, ff_mult=2, dropout=0.1, qk_norm=None,
                pe_attn_head=None)
UNISE_CF = synth.CONFORMER_PARAMS_UNISE


def _err(y, y64):
    y64 = y64.double()
    return float((y.double().cpu() - y64).abs().max() / y64.pow(2).mean().sqrt())


def _check(got, y64, y32, label):
    e, e32 = _err(got, y64), _err(y32, y64)
    bound = 4 * max(e32, 1e-6)
    print(f"{label}: e_hip {e:.3e}  e_cpu32 {e32:.3e}  bound {bound:.3e}")
    assert e <= bound, f"{label}: {e:.3e} > {bound:.3e}"


def _encoder(params, seed, dev, **kw):
    import unified_audio_amd as qa
    from unified_audio_amd.conformer import ConformerEncoder

    sd = synth.conformer_state_dict(seed, params)
    enc = ConformerEncoder(**params, device=dev, **kw).load_state_dict({"dnn.cond_encoder." + k: v for k, v in sd.items()})
    return sd, enc


def _ragged_mask(B, T):
    lens = torch.tensor([T - (7 * b) % (T // 2) for b in range(B)])
    return torch.arange(T)[None, :] < lens[:, None]


# ------------------------------------------------------------------------------- log-mel

@pytest.mark.parametrize("n", [16000, 80000, 16000 + 123])
def test_logmel_matches_fp64(qa_lib, gpu_device, n):
    from unified_audio_amd import unise

    wav = synth.synth_wav(5, 3, n)
    wav[1, 3000:9000] = 0.0
    got = unise.stft_logmel(wav.to(gpu_device))
    assert got.shape == (3, unise.mel_frames(n), 80)
    _check(got, R.stft_logmel(wav, dtype=torch.float64), R.stft_logmel(wav), f"logmel n={n}")


def test_logmel_of_silence(qa_lib, gpu_device):
    """all-zero input segment: log-mel = log(1e-10) within 1e-5 absolute"""
    import math

    from unified_audio_amd import unise

    wav = synth.synth_wav(6, 2, 32000)
    wav[0, 6400:16000] = 0.0  # frames 21 .. 48 see only zeros (a frame covers samples 320 t - 160 .. 320 t + 479)
    got = unise.stft_logmel(wav.to(gpu_device)).cpu()
    assert (got[0, 21:49] - math.log(1e-10)).abs().max() <= 1e-5
    assert (unise.stft_logmel(torch.zeros(1, 4000, device=gpu_device)).cpu() - math.log(1e-10)).abs().max() <= 1e-5


def test_logmel_batch_invariance(qa_lib, gpu_device):
    from unified_audio_amd import unise

    wav = synth.synth_wav(7, 16, 80000).to(gpu_device)
    full = unise.stft_logmel(wav)
    for b in (0, 5, 15):
        assert torch.equal(full[b], unise.stft_logmel(wav[b:b + 1])[0])


# ------------------------------------------------------------------------------- ConformerEncoder

@pytest.mark.parametrize("pe", [None, 1])
@pytest.mark.parametrize("interleaved", [True, False])
def test_small_conformer_matches_fp64(qa_lib, gpu_device, pe, interleaved):
    params = dict(SMALL_CF, pe_attn_head=pe)
    sd, enc = _encoder(params, 31, gpu_device, rope_interleaved=interleaved)
    x = torch.from_numpy(__import__("numpy").random.default_rng(3).standard_normal((3, 70, 64)).astype("float32"))
    enc.enable_taps(True)
    got = enc(x.to(gpu_device))
    t64, t32 = {}, {}
    y64 = R.conformer_encoder(sd, params, x, interleaved=interleaved, dtype=torch.float64, taps=t64)
    y32 = R.conformer_encoder(sd, params, x, interleaved=interleaved, taps=t32)
    for name in t64:  # per-layer taps localise a failure
        _check(enc.tap(name).view(3, 70, 64), t64[name], t32[name], f"{name} pe={pe} il={interleaved}")
    _check(got, y64, y32, f"small conformer pe={pe} il={interleaved}")
    # the two pairings are different functions: the switch is live
    other = R.conformer_encoder(sd, params, x, interleaved=not interleaved, dtype=torch.float64)
    assert _err(got, other) > 1e-3


@pytest.mark.parametrize("k", [3, 7, 15])
def test_depthwise_kernel_sizes(qa_lib, gpu_device, k):
    params = dict(SMALL_CF, depthwise_conv_kernel_size=k, num_layers=1)
    sd, enc = _encoder(params, 40 + k, gpu_device)
    x = torch.from_numpy(__import__("numpy").random.default_rng(4).standard_normal((2, 130, 64)).astype("float32"))
    _check(enc(x.to(gpu_device)), R.conformer_encoder(sd, params, x, dtype=torch.float64), R.conformer_encoder(sd, params, x), f"k={k}")


def test_small_conformer_mask(qa_lib, gpu_device):
    params = dict(SMALL_CF, pe_attn_head=1)
    sd, enc = _encoder(params, 33, gpu_device)
    B, T = 5, 90
    rng = __import__("numpy").random.default_rng(8)
    x = torch.from_numpy(rng.standard_normal((B, T, 64)).astype("float32"))
    mask = _ragged_mask(B, T)
    assert not mask.all() and mask.any(dim=1).all()
    enc.enable_taps(True)
    got = enc(x.to(gpu_device), mask.to(gpu_device))
    tap_a = enc.tap("conformer.0.attn").view(B, T, 64).clone()
    _check(got, R.conformer_encoder(sd, params, x, mask, dtype=torch.float64), R.conformer_encoder(sd, params, x, mask), "masked conformer")
    # everything before layer 0's attention is per-frame: the input at masked positions cannot reach the valid rows of this tap
    x2 = x.clone()
    x2[~mask] = torch.from_numpy(rng.standard_normal((int((~mask).sum()), 64)).astype("float32")) * 3.0
    enc(x2.to(gpu_device), mask.to(gpu_device))
    tap_b = enc.tap("conformer.0.attn").view(B, T, 64)
    m = mask.to(gpu_device)
    assert torch.equal(tap_a[m], tap_b[m])
    assert (tap_a[~m] == 0).all() and (tap_b[~m] == 0).all()


@pytest.mark.parametrize("B", [1, 16])
def test_unise_condition_encoder_matches_fp64(qa_lib, gpu_device, B):
    from unified_audio_amd.conformer import ConditionEncoder

    T = 250
    sd = synth.cond_encoder_state_dict(51, 80, 512, UNISE_CF)
    enc = ConditionEncoder(80, 512, UNISE_CF, device=gpu_device).load_state_dict({"dnn." + k: v for k, v in sd.items()})
    mel = synth.synth_logmel(9, B, T)
    enc.enable_taps(True)
    got = enc(mel.to(gpu_device))
    t64, t32 = {}, {}
    y64 = R.condition(sd, UNISE_CF, mel, dtype=torch.float64, taps=t64)
    y32 = R.condition(sd, UNISE_CF, mel, taps=t32)
    for name in t64:
        _check(enc.tap(name).view(B, T, 512), t64[name], t32[name], f"B={B} {name}")
    _check(got, y64, y32, f"UniSE condition encoder B={B}")


def test_condition_encoder_batch_invariance(qa_lib, gpu_device):
    from unified_audio_amd.conformer import ConditionEncoder

    sd = synth.cond_encoder_state_dict(52, 80, 512, UNISE_CF)
    enc = ConditionEncoder(80, 512, UNISE_CF, device=gpu_device).load_state_dict(sd)
    mel = synth.synth_logmel(10, 16, 250).to(gpu_device)
    full = enc(mel)
    for b in (0, 7, 15):
        assert torch.equal(full[b], enc(mel[b:b + 1])[0])


def test_refusals(qa_lib, gpu_device):
    import unified_audio_amd as qa
    from unified_audio_amd._lib import QuarkAudioError
    from unified_audio_amd.conformer import ConditionEncoder, ConformerEncoder

    sd = synth.conformer_state_dict(1, SMALL_CF)
    with pytest.raises(QuarkAudioError, match="qk_norm"):
        ConformerEncoder(**dict(SMALL_CF, qk_norm="rms_norm"), device=gpu_device).load_state_dict(sd)
    with pytest.raises(ValueError, match="qk_norm"):
        ConformerEncoder(**dict(SMALL_CF, qk_norm="layer_norm"), device=gpu_device)
    with pytest.raises(QuarkAudioError, match="must be odd"):
        ConformerEncoder(**dict(SMALL_CF, depthwise_conv_kernel_size=30), device=gpu_device).load_state_dict(sd)
    enc = ConformerEncoder(**SMALL_CF, device=gpu_device).load_state_dict(sd)
    mask = torch.ones(2, 40, dtype=torch.bool)
    mask[1] = False
    with pytest.raises(QuarkAudioError, match="no valid position"):
        enc(torch.zeros(2, 40, 64), mask)
    missing = {k: v for k, v in sd.items() if k != "layers.1.conv_module.sequential.3.running_var"}
    with pytest.raises(QuarkAudioError, match="running_var"):
        ConformerEncoder(**SMALL_CF, device=gpu_device).load_state_dict(missing)
    extra = dict(sd, **{"layers.0.attn.q_norm.weight": torch.ones(32)})
    with pytest.raises(QuarkAudioError, match="unexpected"):
        ConformerEncoder(**SMALL_CF, device=gpu_device).load_state_dict(extra)
    # a checkpoint without cond_* keys loads for the body; the condition path then raises
    lm_sd = {k: v for k, v in L.lm_state_dict(3, SMALL).items() if not k.startswith(("task_embedding", "enroll_sos", "adapter"))}
    m = _custom(SMALL, SMALL_CF, gpu_device)
    with pytest.raises(QuarkAudioError, match="cond_"):
        m.load_state_dict(lm_sd)
    m.load_state_dict(lm_sd, strict=False)
    m.generate(None, global_length=2, semantic_length=2, do_sample=False)
    with pytest.raises(QuarkAudioError, match="cond_"):
        m.generate(torch.zeros(1, 8, 80), global_length=2, semantic_length=2, do_sample=False)


# ------------------------------------------------------------------------------- CustomLlamaModel

def _custom(spec, params, dev, **kw):
    import unified_audio_amd as qa
    from unified_audio_amd.llm import CustomLlamaModel

    return CustomLlamaModel(cond_dim=80, global_size=spec.global_size, semantic_size=spec.semantic_size, hidden_size=spec.hidden,
                            num_layers=spec.n_layers, num_attention_heads=spec.n_heads, conformer_params=params, device=dev, **kw)


def _weights(spec, params, seed, gain=2.0):
    sd = L.lm_state_dict(seed, spec)
    sd = {k: v for k, v in sd.items() if not k.startswith(("task_embedding", "enroll_sos", "adapter"))}
    sd.update(synth.cond_encoder_state_dict(seed + 1, 80, spec.hidden, params, gain))
    return sd


def _audit(sd, spec, params, cond, B, G, S, gids, sids, tol=2e-4):
    """tests/test_llm_gpu.py::_audit's protocol: the restatement is re-run teacher-forced on the HIP tokens; a stream may only differ
    where the restatement's own decision is a near-tie (top-2 gap <= 2e-4)."""
    g_o, s_o, _, _ = R.generate(sd, spec, params, cond, G, S, B)
    free = min((gids == g_o).float().mean().item(), (sids == s_o).float().mean().item())
    forced = torch.cat([gids + spec.global_offset, sids + spec.semantic_offset], dim=1)
    _, _, toks_f, gaps = R.generate(sd, spec, params, cond, G, S, B, forced=forced)
    wrong = toks_f != forced
    assert not (wrong & (gaps > tol)).any(), f"{int((wrong & (gaps > tol)).sum())} decisive mismatches"
    return free, int(wrong.sum())


@pytest.mark.parametrize("with_cond", [True, False])
def test_small_generate_matches_restatement(qa_lib, gpu_device, with_cond):
    sd = _weights(SMALL, SMALL_CF, 71)
    m = _custom(SMALL, SMALL_CF, gpu_device).load_state_dict({"dnn." + k: v for k, v in sd.items()})
    B, G, S = 3, 6, 14
    cond = synth.synth_logmel(11, B, 20) if with_cond else None
    gids, sids = m.generate(None if cond is None else cond.to(gpu_device), global_length=G, semantic_length=S, do_sample=False, batch_size=B)
    assert gids.shape == (B, G) and sids.shape == (B, S) and gids.dtype == torch.int64
    free, ties = _audit(sd, SMALL, SMALL_CF, cond, B, G, S, gids.cpu(), sids.cpu())
    print("free-running agreement", free, "near-tie flips", ties)
    assert ties > 0 or free == 1.0
    if with_cond:  # a path that ignored the condition would produce the unconditional stream
        g0, s0 = m.generate(None, global_length=G, semantic_length=S, do_sample=False, batch_size=B)
        assert not (torch.equal(g0, gids) and torch.equal(s0, sids))


def test_unise_generate_rows_equal_single_runs(qa_lib, gpu_device):
    """UniSE spec, B = 16 rows with distinct conditions: free-running audit against the restatement for two rows, every row equal to its
    one-sequence run, sampling seeded and reproducible."""
    sd = _weights(L.SPEC_UNISE, UNISE_CF, 81)
    m = _custom(L.SPEC_UNISE, UNISE_CF, gpu_device).load_state_dict(sd)
    B, G, S, T = 16, 32, 40, 50
    cond = synth.synth_logmel(12, B, T)
    gids, sids = m.generate(cond.to(gpu_device), global_length=G, semantic_length=S, do_sample=False)
    for b in (0, 9, 15):
        g1, s1 = m.generate(cond[b:b + 1].to(gpu_device), global_length=G, semantic_length=S, do_sample=False)
        assert torch.equal(g1[0], gids[b]) and torch.equal(s1[0], sids[b])
    free, ties = _audit(sd, L.SPEC_UNISE, UNISE_CF, cond[:2], 2, G, S, gids[:2].cpu(), sids[:2].cpu())
    print("UniSE free-running agreement", free, "near-tie flips", ties)
    assert ties > 0 or free == 1.0
    gu, su = m.generate(None, global_length=G, semantic_length=S, do_sample=False, batch_size=2)
    assert torch.equal(gu[0], gu[1]) and torch.equal(su[0], su[1])
    freeu, tiesu = _audit(sd, L.SPEC_UNISE, UNISE_CF, None, 2, G, S, gu.cpu(), su.cpu())
    assert tiesu > 0 or freeu == 1.0
    torch.manual_seed(5)
    a = m.generate(cond[:4].to(gpu_device), global_length=G, semantic_length=S, do_sample=True)
    torch.manual_seed(5)
    b2 = m.generate(cond[:4].to(gpu_device), global_length=G, semantic_length=S, do_sample=True)
    assert torch.equal(a[0], b2[0]) and torch.equal(a[1], b2[1])
    assert int(a[0].min()) >= 0 and int(a[0].max()) < 4096 and int(a[1].min()) >= 0 and int(a[1].max()) < 8192


@pytest.mark.parametrize("with_cond", [True, False])
@pytest.mark.parametrize("eps", [0.1, 0.0])
def test_small_forward_matches_fp64(qa_lib, gpu_device, with_cond, eps):
    sd = _weights(SMALL, SMALL_CF, 91)
    m = _custom(SMALL, SMALL_CF, gpu_device, label_smoothing=eps).load_state_dict(sd)
    B, G, T = 4, 6, 11
    gen = torch.Generator().manual_seed(17)
    g = torch.randint(0, SMALL.global_size, (B, G), generator=gen, dtype=torch.int32)
    s = torch.randint(0, SMALL.semantic_size, (B, T), generator=gen, dtype=torch.int64)
    cond = synth.synth_logmel(13, B, 18) if with_cond else None
    dc = None if cond is None else cond.to(gpu_device)
    m.enable_taps(True)
    loss, acc = m(g, s, dc)
    z = m.tap("logits.forced").view(B, G + T + 1, SMALL.vocab).cpu()
    loss_seq, acc_seq = m.score(g, s, dc)
    r64 = R.score(sd, SMALL, SMALL_CF, g, s, cond, eps, dtype=torch.float64)
    r32 = R.score(sd, SMALL, SMALL_CF, g, s, cond, eps)
    _check(z, r64["logits"], r32["logits"], f"forced logits cond={with_cond}")
    rel = ((loss_seq.cpu().double() - r64["loss_seq"]).abs() / r64["loss_seq"].abs()).max().item()
    print(f"per-sequence loss: relative error {rel:.3e} (bound 4e-6)")
    assert rel <= 4e-6
    assert abs(float(loss) - r64["loss"]) <= 4e-6 * abs(r64["loss"])
    # accuracy: equal except at audited near-ties of the restatement
    top2 = r64["logits"].topk(2, dim=-1).values
    decisive = (top2[..., 0] - top2[..., 1]) > 2e-4
    am = R.SR.first_argmax(z)
    assert torch.equal(am[decisive], r64["argmax"][decisive])
    # the count of correct rows can differ from the restatement's by at most the non-decisive rows of the sequence
    slack = (~decisive).sum(-1)
    correct = (acc_seq.cpu().double() * (G + T + 1)).round().long()
    assert ((correct - r64["correct"]).abs() <= slack).all()
    assert torch.equal(((am == r64["targets"]) & decisive).sum(-1), ((r64["argmax"] == r64["targets"]) & decisive).sum(-1))
    assert abs(float(acc) * z.shape[0] * z.shape[1] - float(r64["correct"].sum())) <= float(slack.sum()) + 1e-3
    # a sequence's values do not depend on its batch
    l1, _ = m.score(g[2:3], s[2:3], None if dc is None else dc[2:3])
    assert torch.equal(l1[0], loss_seq[2])


def test_llm_sft_is_unchanged_by_condition_calls(qa_lib, gpu_device):
    """LLM_SFT.generate / forward tokens and logits on the SAME handle are bit-identical before and after condition-path calls."""
    sd = _weights(SMALL, SMALL_CF, 95)
    import dataclasses

    spec1 = dataclasses.replace(SMALL, feats_dim=32, num_tasks=1)  # the inner handle's LLM_SFT shapes
    full = dict(L.lm_state_dict(95, spec1), **{k: v for k, v in sd.items() if k.startswith("cond_")})
    m = _custom(SMALL, SMALL_CF, gpu_device)
    m.load_state_dict(full)  # the SFT-only tensors are real here: the inner LLM_SFT handle is a complete one
    sft = m.lm
    sft.task_map = {"se": 0}
    B, Nm, S, G = 3, 9, 10, 5
    mix = L.synth_feats(1, B, Nm, 32).to(gpu_device)
    mel = torch.zeros(B, S, 80)
    gi = torch.randint(0, SMALL.global_size, (B, G))
    si = torch.randint(0, SMALL.semantic_size, (B, S))

    def run():
        sft.enable_taps(True)
        g, s = sft.generate("se", None, None, mel, mix, global_length=G, do_sample=False)
        zg, zs = sft.tap("logits.global").clone(), sft.tap("logits.semantic").clone()
        loss, acc = sft("se", None, None, mel, mix, gi, si)
        return g, s, zg, zs, sft.tap("logits.forced").clone(), loss.clone(), acc.clone()

    before = run()
    cond = synth.synth_logmel(14, B, 12).to(gpu_device)
    m.generate(cond, global_length=G, semantic_length=S, do_sample=False)
    m.generate(None, global_length=G, semantic_length=S, do_sample=True, batch_size=2)
    m(gi, si, cond)
    m(gi, si, None)
    after = run()
    for a, b in zip(before, after):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------- reference goldens (tools/gen_golden_lm_cond.py)

def _check_golden(got, golden, y64, y32, label):
    """against what the reference's own class computed in float32: |got - golden| <= |got - y64| + |golden - y64|"""
    e, eg, e32 = _err(got, golden), _err(golden, y64), _err(y32, y64)
    bound = 4 * max(e32, 1e-6) + eg
    print(f"{label}: e_hip_vs_golden {e:.3e}  golden_vs_fp64 {eg:.3e}  e_cpu32 {e32:.3e}  bound {bound:.3e}")
    assert e <= bound, f"{label}: {e:.3e} > {bound:.3e}"


@pytest.mark.parametrize("name", list(R.CONFORMER_CASES))
def test_conformer_reference_golden(qa_lib, gpu_device, name):
    from unified_audio_amd.conformer import ConformerEncoder

    params, sd, x, mask = R.golden_conformer_case(name)
    enc = ConformerEncoder(**params, device=gpu_device).load_state_dict(sd)
    got = enc(x.to(gpu_device), None if mask is None else mask.to(gpu_device))
    _check_golden(got, R.load_golden("lm_cond_conformer")[name], R.conformer_encoder(sd, params, x, mask, dtype=torch.float64),
                  R.conformer_encoder(sd, params, x, mask), f"golden conformer {name}")


def test_logmel_reference_golden(qa_lib, gpu_device):
    from unified_audio_amd import unise

    wav = R.golden_logmel_wav()
    got = unise.stft_logmel(wav.to(gpu_device))
    golden = R.load_golden("lm_cond_logmel")["logmel"]
    assert got.shape == golden.shape
    _check_golden(got, golden, R.stft_logmel(wav, dtype=torch.float64), R.stft_logmel(wav), "golden logmel")


def test_generate_reference_goldens(qa_lib, gpu_device):
    """every step of the golden streams has a top-2 gap above the 2e-4 near-tie bar: the streams must be identical"""
    gold = R.load_golden("lm_cond_generate")
    assert float(gold["cond_gap"].min()) > 2e-4 and float(gold["nocond_gap"].min()) > 2e-4
    sd = R.golden_lm_weights()
    m = _custom(R.GOLDEN_SPEC, R.GOLDEN_CF, gpu_device).load_state_dict(sd)
    cond, _, _ = R.golden_lm_inputs()
    g, s = m.generate(cond.to(gpu_device), global_length=R.GOLDEN_G, semantic_length=R.GOLDEN_S, do_sample=False)
    assert torch.equal(g.cpu(), gold["cond_global"].long()) and torch.equal(s.cpu(), gold["cond_semantic"].long())
    for b in range(R.GOLDEN_B):  # and each row alone
        g1, s1 = m.generate(cond[b:b + 1].to(gpu_device), global_length=R.GOLDEN_G, semantic_length=R.GOLDEN_S, do_sample=False)
        assert torch.equal(g1[0], g[b]) and torch.equal(s1[0], s[b])
    g0, s0 = m.generate(None, global_length=R.GOLDEN_G, semantic_length=R.GOLDEN_S, do_sample=False, batch_size=2)
    for b in range(2):
        assert torch.equal(g0[b].cpu(), gold["nocond_global"][0].long()) and torch.equal(s0[b].cpu(), gold["nocond_semantic"][0].long())


@pytest.mark.parametrize("name", list(R.FORWARD_CASES))
def test_forward_reference_goldens(qa_lib, gpu_device, name):
    with_cond, eps = R.FORWARD_CASES[name]
    gold = R.load_golden("lm_cond_forward")
    sd = R.golden_lm_weights()
    m = _custom(R.GOLDEN_SPEC, R.GOLDEN_CF, gpu_device, label_smoothing=eps).load_state_dict(sd)
    cond, g, s = R.golden_lm_inputs()
    loss, acc = m(g, s, cond.to(gpu_device) if with_cond else None)
    r64 = R.score(sd, R.GOLDEN_SPEC, R.GOLDEN_CF, g, s, cond if with_cond else None, eps, dtype=torch.float64)
    gl, ga = float(gold[name + "_loss"]), float(gold[name + "_acc"])
    print(f"{name}: loss {float(loss):.7f} golden {gl:.7f} fp64 {r64['loss']:.7f}; acc {float(acc):.5f} golden {ga:.5f}")
    assert abs(float(loss) - gl) <= 4e-6 * abs(r64["loss"]) + abs(gl - r64["loss"])
    top2 = r64["logits"].topk(2, dim=-1).values
    n_rows = r64["targets"].numel()
    slack = int(((top2[..., 0] - top2[..., 1]) <= 2e-4).sum())
    assert abs(float(acc) - ga) * n_rows <= slack + 1e-3
