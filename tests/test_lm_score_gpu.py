"""LLM_SFT.forward / score (qa_lm_score: teacher-forced scoring, QuarkAudio-UniSE/model/llm/llm_sft.py:37-90) and Model.validation_step
(model/model.py:134-160) on the HIP path.

(a) fp64 parity at the teacher-forced logits (tap logits.forced) and at the per-sequence loss, against tests/lm_score_ref.py in float64
    (the truth) and float32 (the yardstick): e = max |l - l64| / rms(l64) per row, bound C_PARITY * max(e_cpu32, floor) as in
    tests/test_lm_logits_gpu.py; the accuracy equals the fp64 oracle's except at audited near-ties.
(b) the row kernel's arg-max is the FIRST of exactly tied maxima (duplicated output_head rows in different GEMM tiles).
(c) bit-exact invariance: batch, head row chunks, taps; generate is unchanged by a score call on the same handle.
(d) errors, int32 / int64 ids, the reference's golden values (tools/gen_golden_lm_score.py) and validation_step end to end.
"""
import os

import numpy as np
import pytest
import torch

from oracle import llm_ref as L
from tests import lm_score_ref as R
from tests.test_llm_gpu import SMALL, _model

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
C_PARITY = 4.0
E_FLOOR = 1e-6       # logits, as tests/test_lm_logits_gpu.py
LOSS_FLOOR = 1e-6    # relative error of a sequence's loss


def _inputs(spec, task, B, Nm, Ne, G, T, seed):
    mix = L.synth_feats(seed, B, Nm, spec.feats_dim)
    enr = L.synth_feats(seed + 1, B, Ne, spec.feats_dim) if task != "se" else None
    gen = torch.Generator().manual_seed(seed + 2)
    g = torch.randint(0, spec.global_size, (B, G), generator=gen, dtype=torch.int32)
    s = torch.randint(0, spec.semantic_size, (B, T), generator=gen)
    return enr, mix, g, s


def _score(lm, dev, task, enr, mix, g, s, taps=True):
    """HIP score + forward values on the host: (loss_seq, correct_seq, loss, acc, logits [B, Lt, V] or None)."""
    B = mix.shape[0]
    mel = torch.zeros(B, 1, 80)
    lm.enable_taps(taps)
    loss_seq, correct, loss, acc, Lt = lm._score(task, None if enr is None else mel, None if enr is None else enr.to(dev), mel, mix.to(dev),
                                                 g.to(dev), s.to(dev))
    z = lm.tap("logits.forced").view(B, Lt, -1).cpu() if taps else None
    torch.cuda.synchronize()
    return loss_seq.cpu(), correct.cpu(), float(loss), float(acc), z


def _row_err(hip, truth):
    truth = truth.double()
    rms = truth.pow(2).mean(-1).sqrt()
    return float(((hip.double() - truth).abs().amax(-1) / rms).max())


def _parity(sd, spec, task, enr, mix, g, s, eps, got, label):
    loss_seq, correct, loss, acc, z = got
    o64 = R.score(sd, spec, task, enr, mix, g, s, eps, torch.float64)
    o32 = R.score(sd, spec, task, enr, mix, g, s, eps, torch.float32)
    e_hip, e_cpu = _row_err(z, o64["logits"]), _row_err(o32["logits"], o64["logits"])
    bound = C_PARITY * max(e_cpu, E_FLOOR)
    l64 = o64["loss_seq"]
    el_hip = float(((loss_seq.double() - l64).abs() / l64.abs()).max())
    el_cpu = float(((o32["loss_seq"] - l64).abs() / l64.abs()).max())
    lbound = C_PARITY * max(el_cpu, LOSS_FLOOR)
    print(f"score parity {label}: logits e_hip {e_hip:.3e} e_cpu32 {e_cpu:.3e} bound {bound:.3e}; loss e_hip {el_hip:.3e} "
          f"e_cpu32 {el_cpu:.3e} bound {lbound:.3e}; acc {acc:.4f}")
    assert e_hip <= bound, f"{label}: logits {e_hip:.3e} from the fp64 truth, bound {bound:.3e}"
    assert el_hip <= lbound, f"{label}: per-sequence loss {el_hip:.3e} from the fp64 truth, bound {lbound:.3e}"
    n = l64.numel() * o64["targets"].shape[1]
    assert abs(loss - float(o64["loss"])) <= lbound * abs(float(o64["loss"])) + 1e-7
    # the kernel's correct count is its own first arg-max of the logits it produced
    am = R.first_argmax(z)
    assert torch.equal(correct, (am == o64["targets"]).sum(-1)), f"{label}: correct counts disagree with the tapped logits"
    assert acc == pytest.approx(float(correct.sum()) / n, abs=1e-7)
    # against fp64: a row may flip only when its fp64 top-2 gap is within the parity bound (audit)
    flip = am != o64["argmax"]
    if flip.any():
        top2 = o64["logits"].topk(2, dim=-1).values
        gap = (top2[..., 0] - top2[..., 1]) / o64["logits"].pow(2).mean(-1).sqrt()
        assert bool((gap[flip] <= 2 * bound).all()), f"{label}: arg-max differs from fp64 at a row that is no near-tie"
    return o64


# (spec, weight seed, task, B, n_mix, n_enroll, G, T, eps, targets)
CASES = {
    "small_b1_se": (SMALL, 71, "se", 1, 9, 0, 4, 10, 0.1, "random"),
    "small_b16_tse": (SMALL, 72, "tse", 16, 7, 5, 6, 12, 0.1, "random"),
    "small_b65_rtse_eps0": (SMALL, 73, "rtse", 65, 6, 4, 3, 8, 0.0, "random"),     # two groups of sequences (64 + 1)
    "small_b16_greedy_tse": (SMALL, 74, "tse", 16, 8, 6, 5, 14, 0.1, "greedy"),   # accuracy strictly between 0 and 1
    "unise_b2_se_greedy": (L.SPEC_UNISE, 75, "se", 2, 20, 0, 32, 30, 0.1, "greedy"),
    "unise_b3_rtse": (L.SPEC_UNISE, 76, "rtse", 3, 12, 8, 32, 20, 0.1, "random"),
    "small_long_se": (SMALL, 77, "se", 1, 3000, 0, 32, 1000, 0.1, "greedy"),      # 4036 positions (limit 4096)
}


@pytest.mark.parametrize("case", list(CASES))
def test_score_matches_fp64_oracle(qa_lib, gpu_device, case):
    spec, seed, task, B, Nm, Ne, G, T, eps, kind = CASES[case]
    sd, lm = _model(spec, seed, gpu_device)
    lm.label_smoothing = eps
    enr, mix, g, s = _inputs(spec, task, B, Nm, Ne, G, T, seed + 100)
    if kind == "greedy":  # the model's own greedy stream as targets
        mel = torch.zeros(B, T, 80)
        g, s = lm.generate(task, None if enr is None else mel, None if enr is None else enr.to(gpu_device), mel, mix.to(gpu_device),
                           global_length=G, do_sample=False)
        g, s = g.cpu(), s.cpu()
    got = _score(lm, gpu_device, task, enr, mix, g, s)
    assert torch.isfinite(got[4]).all() and torch.isfinite(got[0]).all()
    _parity(sd, spec, task, enr, mix, g, s, eps, got, case)
    if kind == "greedy":
        assert 0.0 < got[3] < 1.0, got[3]


@pytest.mark.parametrize("name", list(R.CASES))
def test_reference_goldens(qa_lib, gpu_device, name):
    """The values the reference's own forward produced (loss, accuracy, per-row KL and arg-max), from the same seeded inputs."""
    gold = np.load(os.path.join(HERE, "golden", name + ".npz"))
    spec, sd, task, mix, enr, g, s, eps = R.case_tensors(name)
    cfg = dict(global_size=spec.global_size, semantic_size=spec.semantic_size, hidden_size=spec.hidden, num_layers=spec.n_layers,
               num_attention_heads=spec.n_heads, label_smoothing=eps)
    import unified_audio_amd as qa

    lm = qa.LLM_SFT(num_tasks=spec.num_tasks, feats_dim=spec.feats_dim, llm_base_config=cfg, device=gpu_device).load_state_dict(sd)
    loss_seq, correct, loss, acc, z = _score(lm, gpu_device, task, enr, mix, g, s)
    assert loss == pytest.approx(float(gold["loss"]), rel=2e-5)
    np.testing.assert_allclose(R.row_kl(z, torch.from_numpy(gold["targets"].astype(np.int64)), eps).numpy(), gold["row_kl"], rtol=2e-5, atol=2e-5)
    torch.testing.assert_close(loss_seq, torch.from_numpy(gold["row_kl"]).double().mean(-1).float(), rtol=2e-5, atol=0)
    am = R.first_argmax(z).numpy()
    clear = gold["gap"] > 1e-3
    assert np.array_equal(am[clear], gold["argmax"].astype(np.int64)[clear])
    if clear.all():
        assert acc == pytest.approx(float(gold["acc"]), abs=1e-6)


def test_head_argmax_takes_the_first_of_exactly_tied_maxima(qa_lib, gpu_device):
    """Two output_head rows made identical: their logits are bit-identical (each column's k order is the same), in different GEMM tiles.
    The pair is pointed along the mean final hidden state (fp32 oracle) and scaled to win most rows.  Tied rows whose target is the lower
    index count as correct, tied rows whose target is the higher never do."""
    import torch.nn.functional as F

    import unified_audio_amd as qa

    for spec, (gl, sm) in ((SMALL, (1, 100)), (L.SPEC_UNISE, (2, 8000))):
        sd = L.lm_state_dict(81, spec)
        B, G, T = 8, 8, 12
        mix = L.synth_feats(82, B, 6, spec.feats_dim)
        g = torch.full((B, G), gl, dtype=torch.int64)
        s = torch.full((B, T), sm, dtype=torch.int64)
        inp, tgt = R.token_ids(g, s, spec)
        with torch.no_grad():
            x = torch.cat([L.build_prompt(sd, 0, None, mix), sd["codec_embedding.weight"][inp]], dim=1)
            hs = L.llm_forward(sd, x, L.KVCache(spec.n_layers), spec)[:, -tgt.shape[1]:]
            m = hs.reshape(-1, spec.hidden).mean(0)
            scale = 8.0 * float(F.linear(hs, sd["output_head.weight"]).abs().amax()) / float((hs @ m).median())
        a, b = spec.global_offset + gl, spec.semantic_offset + sm
        w = sd["output_head.weight"].clone()
        w[a] = scale * m
        w[b] = w[a]
        sd["output_head.weight"] = w
        cfg = dict(global_size=spec.global_size, semantic_size=spec.semantic_size, hidden_size=spec.hidden, num_layers=spec.n_layers,
                   num_attention_heads=spec.n_heads)
        lm = qa.LLM_SFT(num_tasks=spec.num_tasks, feats_dim=spec.feats_dim, llm_base_config=cfg, device=gpu_device).load_state_dict(sd)
        _, correct, _, _, z = _score(lm, gpu_device, "se", None, mix, g, s)
        tie = (z[..., a] == z[..., b]) & (z[..., a] == z.amax(-1))
        assert int((tie & (tgt == a)).sum()) > 0 and int((tie & (tgt == b)).sum()) > 0, "the case decides no tie for both targets"
        ok_rows = R.first_argmax(z) == tgt
        assert torch.equal(correct, ok_rows.sum(-1))
        assert bool(ok_rows[tie & (tgt == a)].all()) and not bool(ok_rows[tie & (tgt == b)].any())


@pytest.mark.parametrize("spec_name", ["small", "unise"])
def test_sequence_values_do_not_depend_on_the_batch(qa_lib, gpu_device, spec_name):
    spec = SMALL if spec_name == "small" else L.SPEC_UNISE
    _, lm = _model(spec, 83, gpu_device)
    enr, mix, g, s = _inputs(spec, "tse", 65, 6, 5, 5, 9, 84)
    ref = _score(lm, gpu_device, "tse", enr, mix, g, s)
    for B in (1, 2, 7, 16, 33, 64, 65):
        got = _score(lm, gpu_device, "tse", enr[:B], mix[:B], g[:B], s[:B])
        assert torch.equal(got[0], ref[0][:B]) and torch.equal(got[1], ref[1][:B]), B
        assert torch.equal(got[4], ref[4][:B]), B
    for i in (40, 64):  # a sequence alone equals itself inside the batch of 65
        one = _score(lm, gpu_device, "tse", enr[i:i + 1], mix[i:i + 1], g[i:i + 1], s[i:i + 1])
        assert torch.equal(one[0], ref[0][i:i + 1]) and torch.equal(one[1], ref[1][i:i + 1]), i


def test_head_row_chunks_and_taps_do_not_change_a_bit(qa_lib, gpu_device, knob):
    spec = L.SPEC_UNISE
    _, lm = _model(spec, 85, gpu_device)
    enr, mix, g, s = _inputs(spec, "se", 5, 15, 0, 32, 40, 86)
    ref = _score(lm, gpu_device, "se", enr, mix, g, s)
    for rows in (1, 7, 100, 370, 1 << 20):
        knob("QA_LM_SCORE_ROWS", rows)
        got = _score(lm, gpu_device, "se", enr, mix, g, s)
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]) and got[2:4] == ref[2:4] and torch.equal(got[4], ref[4]), rows
    off = _score(lm, gpu_device, "se", enr, mix, g, s, taps=False)
    assert torch.equal(off[0], ref[0]) and torch.equal(off[1], ref[1]) and off[2:4] == ref[2:4]


@pytest.mark.parametrize("B,graph", [(12, 0), (12, 1), (65, 0)])
def test_generate_is_unchanged_by_a_score_call(qa_lib, gpu_device, knob, B, graph):
    """Scoring uses a workspace of its own: tokens and decode logits of generate are the same before and after a score call on the
    same handle (B = 65 and QA_LM_GRAPH = 1 replay captured steps, which must survive)."""
    knob("QA_LM_GRAPH", graph)
    spec = SMALL
    _, lm = _model(spec, 87, gpu_device)
    enr, mix, g, s = _inputs(spec, "tse", B, 8, 5, 4, 9, 88)
    mel = torch.zeros(B, 9, 80)
    args = ("tse", mel, enr.to(gpu_device), mel, mix.to(gpu_device))

    def gen():
        lm.enable_taps(True)
        out = lm.generate(*args, global_length=4, do_sample=False)
        t = (lm.tap("logits.global"), lm.tap("logits.semantic"))
        torch.cuda.synchronize()
        return [x.cpu() for x in (*out, *t)]

    before = gen()
    _score(lm, gpu_device, "tse", enr, mix, g, s)
    _score(lm, gpu_device, "tse", enr[:3], L.synth_feats(89, 3, 40, spec.feats_dim), g[:3], s[:3])  # a larger workspace
    after = gen()
    assert all(torch.equal(x, y) for x, y in zip(before, after))


def test_ids_dtypes_and_forward_interface(qa_lib, gpu_device):
    """int32 and int64 ids give the same bits; forward returns 0-dim fp32 device tensors and is callable as self.dnn(...); score's
    per-sequence values average to forward's."""
    spec = SMALL
    _, lm = _model(spec, 90, gpu_device)
    enr, mix, g, s = _inputs(spec, "rtse", 4, 6, 5, 7, 11, 91)
    mel = torch.zeros(4, 1, 80)
    kw = dict(task_name="rtse", enroll_mel=mel, enroll_feats=enr.to(gpu_device), mix_mel=mel, mix_feats=mix.to(gpu_device))
    loss, acc = lm(global_ids=g.to(gpu_device), semantic_ids=s.to(gpu_device), **kw)
    assert loss.dim() == 0 and acc.dim() == 0 and loss.dtype == torch.float32 and loss.device.type == "cuda"
    loss2, acc2 = lm.forward(global_ids=g.long().to(gpu_device), semantic_ids=s.int().to(gpu_device), **kw)
    assert torch.equal(loss, loss2) and torch.equal(acc, acc2)
    ls, accs = lm.score(global_ids=g.to(gpu_device), semantic_ids=s.to(gpu_device), **kw)
    assert ls.shape == (4,) and accs.shape == (4,)
    assert float(ls.double().mean()) == pytest.approx(float(loss), rel=1e-6)
    assert float(accs.double().mean()) == pytest.approx(float(acc), abs=1e-7)


def test_errors(qa_lib, gpu_device):
    import unified_audio_amd as qa

    spec = SMALL
    _, lm = _model(spec, 92, gpu_device)
    enr, mix, g, s = _inputs(spec, "se", 2, 6, 0, 4, 6, 93)
    V = 3 + spec.global_size + spec.semantic_size
    for gg, ss in ((g.clone().fill_(V - 3), s), (g, s.clone().fill_(-spec.semantic_size - 4)), (g, s.clone().fill_(V))):
        with pytest.raises(IndexError):
            _score(lm, gpu_device, "se", None, mix, gg, ss)
    # in range after the shift, as nn.Embedding sees it: accepted (the reference does not restrict ids to their slices)
    _score(lm, gpu_device, "se", None, mix, g.clone().fill_(-3), s.clone().fill_(-spec.semantic_offset))
    with pytest.raises(KeyError):
        _score(lm, gpu_device, "denoise", None, mix, g, s)
    with pytest.raises(qa.QuarkAudioError, match="max_position_embeddings"):
        _score(lm, gpu_device, "se", None, L.synth_feats(94, 1, 4000, spec.feats_dim), g[:1], torch.zeros(1, 100, dtype=torch.int64))
    cfg = dict(global_size=spec.global_size, semantic_size=spec.semantic_size, hidden_size=spec.hidden, num_layers=spec.n_layers,
               num_attention_heads=spec.n_heads)
    empty = qa.LLM_SFT(num_tasks=3, feats_dim=spec.feats_dim, llm_base_config=cfg, device=gpu_device)
    with pytest.raises(qa.QuarkAudioError, match="no weights"):
        empty("se", None, None, torch.zeros(2, 1, 80), mix.to(gpu_device), g.to(gpu_device), s.to(gpu_device))
    with pytest.raises(qa.QuarkAudioError, match="no intermediate"):
        lm.enable_taps(False)
        lm("se", None, None, torch.zeros(2, 1, 80), mix.to(gpu_device), g.to(gpu_device), s.to(gpu_device))
        lm.tap("logits.forced")


def _validation_model(device):
    """Model with synthetic components: a small WavLM (semantic model), a BiCodec tokenizer with its encoder (small XLSR-53 front end, 4
    global tokens of 4096 values, 128 semantic codes) and an LM whose vocabulary covers both."""
    import dataclasses

    import unified_audio_amd as qa
    from oracle import ssl_ref as SR
    from tests.test_bicodec_tokenize_gpu import SMALL as BSMALL
    from tests.test_bicodec_tokenize_gpu import _espec, _full_sd, _model as _bicodec
    from unified_audio_amd import unise as U

    sspec = SR.SSLSpec(conv_dim=(64,) * 7, hidden_size=96, num_hidden_layers=2, num_attention_heads=3, intermediate_size=192,
                       num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=2, num_buckets=32, max_bucket_distance=100,
                       compress_exponent=0.0)
    fx = qa.SSLFeatureExtractor(qa.SSLSpec(**{f: getattr(sspec, f) for f in sspec.__dataclass_fields__}), device=device)
    fx.load_state_dict(SR.synth_state_dict(4, sspec, "wavlm"))
    xs = SR.SSLSpec(conv_dim=(32,) * 7, conv_bias=True, feat_extract_norm="layer", hidden_size=96, num_hidden_layers=16, num_attention_heads=3,
                    intermediate_size=192, do_stable_layer_norm=True, num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=2,
                    pad=0, select=(11, 14, 16), compress_exponent=0.0)
    xfx = qa.SSLFeatureExtractor(qa.SSLSpec(**{f.name: getattr(xs, f.name) for f in dataclasses.fields(xs)}), device=device)
    xfx.load_state_dict(SR.synth_state_dict(101, xs, "wav2vec2"))
    espec = dataclasses.replace(_espec(**BSMALL), input_channels=96, spk_latent_dim=32, token_num=4)
    tok = qa.BiCodecTokenizer(model=_bicodec(espec, _full_sd(espec, 102), device), feature_extractor=xfx)
    lspec = L.LMSpec(hidden=256, n_layers=2, n_heads=4, global_size=4096, semantic_size=128, feats_dim=96)
    lm = qa.LLM_SFT(feats_dim=96, llm_base_config=dict(global_size=4096, semantic_size=128, hidden_size=256, num_layers=2,
                                                       num_attention_heads=4), device=device).load_state_dict(L.lm_state_dict(8, lspec))
    return U.Model({}, device=device, semantic_model=fx, tokenizer=tok, dnn=lm), tok, fx, lm


@pytest.mark.parametrize("mode", ["se", "tse", "rtse"])
def test_validation_step_equals_tokenize_then_forward(qa_lib, gpu_device, mode):
    from unified_audio_amd import synth

    model, tok, fx, lm = _validation_model(gpu_device)
    B = 2
    speech = synth.synth_wav(111, B, 16000).to(gpu_device)
    interf = synth.synth_wav(112, B, 16000).to(gpu_device)
    mix = (speech + 0.5 * interf).contiguous()
    enroll = synth.synth_wav(113, B, 12000).to(gpu_device) if mode != "se" else None
    batch = (mode, enroll, mix, speech, interf, torch.tensor([16000] * B), torch.tensor([16000] * B), ["a", "b"])
    out = model.validation_step(batch, 0)
    assert set(out) == {"valid_loss", "valid_acc"} and out["valid_loss"].dim() == 0
    glob, sem = tok.tokenize(interf if mode == "rtse" else speech)
    assert glob.dtype == torch.int32 and glob.shape == (B, 1, 4) and sem.shape == (B, 49)
    mel = torch.zeros(B, 1, 80)
    loss, acc = lm(mode, None if enroll is None else mel, None if enroll is None else fx(enroll), mel, fx(mix), glob.squeeze(1), sem)
    assert torch.equal(out["valid_loss"], loss) and torch.equal(out["valid_acc"], acc)
    assert torch.isfinite(loss) and 0.0 <= float(acc) <= 1.0
    if mode == "rtse":  # the interferer's tokens, not the speech's
        g_sp, s_sp = tok.tokenize(speech)
        other, _ = lm(mode, mel, fx(enroll), mel, fx(mix), g_sp.squeeze(1), s_sp)
        assert not torch.equal(other, loss)
