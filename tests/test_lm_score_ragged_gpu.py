"""Teacher-forced scoring with per-row lengths on the HIP path: LLM_SFT.forward / score(mix_lengths=, semantic_lengths=, enroll_lengths=)
(qa_lm_score_ragged), build_prompt(enroll_lengths=, mix_lengths=) (qa_lm_prompt_ragged) and Model.validation_step(use_lengths=True);
DESIGN.md section 35.  The yardstick is the RECTANGULAR path on the trimmed row, or the fp64 restatement tests/lm_score_ref.py (through
tests/lm_score_ragged_ref.py, row by row) - never the ragged code itself.

(1) each row equals itself alone, bit for bit  (2) a row does not depend on its surroundings  (3) fp64 parity  (4) padding is never read
(5) all-equal lengths are the rectangular call  (6) build_prompt and a KVCache session  (7) validation_step(use_lengths=True)  (8) errors.
"""
import ctypes as C

import pytest
import torch

from oracle import llm_ref as L
from tests import lm_score_ragged_ref as RR
from tests import lm_score_ref as R
from tests.test_lm_score_gpu import C_PARITY, E_FLOOR, LOSS_FLOOR, _model, _score, _validation_model

pytestmark = pytest.mark.gpu
NE, NM, T_, G_, EPS = RR.CASE_NE, RR.CASE_NM, RR.CASE_T, RR.CASE_G, RR.CASE_EPS


def _rag(lm, dev, task, enr, mix, g, s, ne, nm, T, taps=True):
    """HIP score with per-row lengths, on the host: (loss_seq, correct, loss, acc, [logits [Lt_b, V] per row] or None)."""
    B = mix.shape[0]
    mel = torch.zeros(B, 1, 80)
    lm.enable_taps(taps)
    e = None if enr is None else enr.to(dev)
    loss_seq, correct, loss, acc, Lt = lm._score_ragged(task, None if enr is None else mel, e, mel, mix.to(dev), g.to(dev), s.to(dev), nm, T, ne)
    z = list(lm.tap("logits.forced").view(-1, lm.vocab_size).cpu().split(Lt.tolist())) if taps else None
    torch.cuda.synchronize()
    return loss_seq.cpu(), correct.cpu(), float(loss), float(acc), z


def _alone(lm, dev, task, enr, mix, g, s, ne, nm, T, b):
    """Row b through the RECTANGULAR B = 1 call on its trimmed inputs: (loss_seq [1], correct [1], logits [Lt_b, V])."""
    e = None if enr is None else enr[b:b + 1, :ne[b]].contiguous()
    m, gg, ss = mix[b:b + 1, :nm[b]].contiguous(), g[b:b + 1], s[b:b + 1, :T[b]].contiguous()
    if T[b] == 0:  # LLM_SFT._score cannot shape an id tensor of width 0; a uniform vector at full width takes qa_lm_score's own path
        one = _rag(lm, dev, task, e, m, gg, ss, None, None, [0])
        return one[0], one[1], one[4][0]
    one = _score(lm, dev, task, e, m, gg, ss)
    return one[0], one[1], one[4][0]


def _same_row(got, b, one, label):
    assert torch.equal(got[0][b:b + 1], one[0]), f"{label}: loss_seq of row {b}"
    assert torch.equal(got[1][b:b + 1], one[1]), f"{label}: correct of row {b}"
    assert got[4][b].shape == one[2].shape and torch.equal(got[4][b], one[2]), f"{label}: logits.forced of row {b}"


@pytest.mark.parametrize("spec_name,task", [("small", "tse"), ("small", "se"), ("unise", "tse"), ("unise", "se")])
def test_each_row_equals_itself_alone(qa_lib, gpu_device, spec_name, task):
    """(1) loss_seq, correct and the row's slice of logits.forced are torch.equal to the rectangular B = 1 call on the trimmed row."""
    spec, G = (R.SMALL, G_) if spec_name == "small" else (L.SPEC_UNISE, 32)  # unise: the longest row holds 293 positions
    _, lm = _model(spec, RR.CASE_SEED, gpu_device)
    enr, mix, g, s = RR.case_inputs(spec, RR.CASE_SEED, NE, NM, T_, G)
    enr, ne = (enr, NE) if task != "se" else (None, None)
    got = _rag(lm, gpu_device, task, enr, mix, g, s, ne, NM, T_)
    assert [z.shape[0] for z in got[4]] == [G + t + 2 for t in T_]
    for b in range(len(NM)):
        _same_row(got, b, _alone(lm, gpu_device, task, enr, mix, g, s, ne, NM, T_, b), f"{spec_name}/{task}")


def test_a_row_does_not_depend_on_its_surroundings(qa_lib, gpu_device, knob):
    """(2) torch.equal throughout: other neighbours and a larger padded width, alone with padding, B = 70 across the group boundary,
    QA_LM_SCORE_ROWS, taps."""
    spec, dev = R.SMALL, gpu_device
    _, lm = _model(spec, RR.CASE_SEED, dev)
    enr, mix, g, s = RR.case_inputs()
    ref = _rag(lm, dev, "tse", enr, mix, g, s, NE, NM, T_)

    def batch(rows, pad=0):
        """The case's rows `rows` as a batch, `pad` more (random) frames / ids of padding at every maximum."""
        idx = torch.tensor(rows)
        ne, nm, T = [NE[r] for r in rows], [NM[r] for r in rows], [T_[r] for r in rows]
        e = torch.cat([enr[idx, :max(ne)], L.synth_feats(7, len(rows), pad, spec.feats_dim)], dim=1) if pad else enr[idx, :max(ne)]
        m = torch.cat([mix[idx, :max(nm)], L.synth_feats(8, len(rows), pad, spec.feats_dim)], dim=1) if pad else mix[idx, :max(nm)]
        ss = torch.cat([s[idx, :max(T)], torch.full((len(rows), pad), 5, dtype=torch.int64)], dim=1) if pad else s[idx, :max(T)]
        return (e.contiguous(), m.contiguous(), g[idx], ss.contiguous(), ne, nm, T)

    def check(got, rows, label):
        for i, r in enumerate(rows):
            assert torch.equal(got[0][i], ref[0][r]) and torch.equal(got[1][i], ref[1][r]), (label, i, r)
            if got[4] is not None:
                assert torch.equal(got[4][i], ref[4][r]), (label, i, r)

    rows = [4, 0, 2, 0, 5]  # other neighbours, row 3 (the longest) gone, every maximum 37 entries wider than any row needs
    check(_rag(lm, dev, "tse", *batch(rows, pad=37)), rows, "neighbours + width")
    for r in (1, 3):        # alone with padding
        check(_rag(lm, dev, "tse", *batch([r], pad=50)), [r], "alone, padded")
    rows = [i % 6 for i in range(70)]
    rows[63], rows[64:69], rows[69] = 3, [1, 4, 0, 2, 4], 5  # group 0 (rows 0 .. 63) at 265 positions, group 1 (64 .. 69) at its own 139
    got70 = _rag(lm, dev, "tse", *batch(rows))
    check(got70, rows, "B = 70")
    knob("QA_LM_SCORE_ROWS", 64)
    check(_rag(lm, dev, "tse", enr, mix, g, s, NE, NM, T_), list(range(6)), "QA_LM_SCORE_ROWS = 64")
    small = _rag(lm, dev, "tse", *batch(rows))
    assert torch.equal(small[0], got70[0]) and torch.equal(small[1], got70[1]) and small[2:4] == got70[2:4]
    off = _rag(lm, dev, "tse", enr, mix, g, s, NE, NM, T_, taps=False)
    check(off, list(range(6)), "taps off")
    assert off[2:4] == ref[2:4]


def _parity_rows(o64, o32, got, label):
    """tests/test_lm_score_gpu.py::_parity over rows of different lengths: the same bounds, the oracle row by row."""
    loss_seq, correct, loss, acc, z = got

    def err(a, truth):
        truth = truth.double()
        return float(((a.double() - truth).abs().amax(-1) / truth.pow(2).mean(-1).sqrt()).max())

    e_hip = max(err(z[b], o["logits"][0]) for b, o in enumerate(o64["rows"]))
    e_cpu = max(err(o["logits"][0], t["logits"][0]) for o, t in zip(o32["rows"], o64["rows"]))
    bound = C_PARITY * max(e_cpu, E_FLOOR)
    l64 = o64["loss_seq"]
    el_hip = float(((loss_seq.double() - l64).abs() / l64.abs()).max())
    el_cpu = float(((o32["loss_seq"] - l64).abs() / l64.abs()).max())
    lbound = C_PARITY * max(el_cpu, LOSS_FLOOR)
    print(f"ragged score parity {label}: logits e_hip {e_hip:.3e} e_cpu32 {e_cpu:.3e} bound {bound:.3e}; loss e_hip {el_hip:.3e} "
          f"e_cpu32 {el_cpu:.3e} bound {lbound:.3e}; acc {acc:.4f}")
    assert e_hip <= bound, f"{label}: logits {e_hip:.3e} from the fp64 truth, bound {bound:.3e}"
    assert el_hip <= lbound, f"{label}: per-sequence loss {el_hip:.3e} from the fp64 truth, bound {lbound:.3e}"
    n = sum(o64["Lt"])
    assert abs(loss - o64["loss"]) <= lbound * abs(o64["loss"]) + 1e-7
    # the pooled scalars are the sums of the per-row outputs over all target rows
    pooled = float((loss_seq.double() * torch.tensor(o64["Lt"], dtype=torch.float64)).sum()) / n
    assert loss == pytest.approx(pooled, rel=1e-6)
    assert acc == pytest.approx(float(correct.sum()) / n, abs=1e-7)
    for b, o in enumerate(o64["rows"]):
        am = R.first_argmax(z[b])
        assert int(correct[b]) == int((am == o["targets"][0]).sum()), f"{label}: correct of row {b} disagrees with the tapped logits"
        flip = am != o["argmax"][0]
        if flip.any():  # a row may flip only when its fp64 top-2 gap is within the parity bound (audit)
            top2 = o["logits"][0].topk(2, dim=-1).values
            gap = (top2[..., 0] - top2[..., 1]) / o["logits"][0].pow(2).mean(-1).sqrt()
            assert bool((gap[flip] <= 2 * bound).all()), f"{label}: arg-max of row {b} differs from fp64 at a row that is no near-tie"


@pytest.mark.parametrize("task", ["tse", "se"])
def test_case_matches_fp64_oracle(qa_lib, gpu_device, task):
    """(3) every row of the case against score_ragged(float64)."""
    sd, (enr, mix, g, s), o64, o32 = RR.case_oracle(task)
    _, lm = _model(R.SMALL, RR.CASE_SEED, gpu_device)
    lm.label_smoothing = EPS
    got = _rag(lm, gpu_device, task, enr, mix, g, s, None if enr is None else NE, NM, T_)
    assert all(torch.isfinite(z).all() for z in got[4]) and torch.isfinite(got[0]).all()
    _parity_rows(o64, o32, got, f"case/{task}")


def test_greedy_targets_match_fp64_oracle(qa_lib, gpu_device):
    """(3) row b's ids are the model's own greedy stream of a B = 1 generate on its trimmed inputs: accuracy strictly inside (0, 1)."""
    dev = gpu_device
    sd, lm = _model(R.SMALL, RR.CASE_SEED, dev)
    lm.label_smoothing = EPS
    enr, mix, _, _ = RR.case_inputs()
    B = len(NM)
    g = torch.zeros(B, G_, dtype=torch.int64)
    s = torch.zeros(B, max(T_), dtype=torch.int64)
    for b in range(B):
        mel = torch.zeros(1, max(T_[b], 1), 80)
        gb, sb = lm.generate("tse", mel, enr[b:b + 1, :NE[b]].to(dev), mel, mix[b:b + 1, :NM[b]].to(dev), global_length=G_, do_sample=False)
        g[b], s[b, :T_[b]] = gb[0].cpu(), sb[0, :T_[b]].cpu()
    o64 = RR.score_ragged(sd, R.SMALL, "tse", enr, mix, g, s, NE, NM, T_, EPS, torch.float64)
    o32 = RR.score_ragged(sd, R.SMALL, "tse", enr, mix, g, s, NE, NM, T_, EPS, torch.float32)
    got = _rag(lm, dev, "tse", enr, mix, g, s, NE, NM, T_)
    _parity_rows(o64, o32, got, "case/greedy")
    assert 0.0 < got[3] < 1.0, got[3]


def test_padding_is_never_read(qa_lib, gpu_device):
    """(4) NaN frames and out-of-range ids at or behind a row's lengths change no output and raise nothing; a bad id inside does."""
    dev = gpu_device
    _, lm = _model(R.SMALL, RR.CASE_SEED, dev)
    enr, mix, g, s = RR.case_inputs()
    clean = _rag(lm, dev, "tse", enr, mix, g, s, NE, NM, T_)
    e2, m2, s2 = enr.clone(), mix.clone(), s.clone()
    for b in range(len(NM)):
        e2[b, NE[b]:] = float("nan")
        m2[b, NM[b]:] = float("nan")
        s2[b, T_[b]:] = -7 if b % 2 else 10 ** 9
    got = _rag(lm, dev, "tse", e2, m2, g, s2, NE, NM, T_)
    assert torch.equal(got[0], clean[0]) and torch.equal(got[1], clean[1]) and got[2:4] == clean[2:4]
    assert all(torch.equal(a, b) for a, b in zip(got[4], clean[4]))
    s3 = s2.clone()
    s3[2, T_[2] - 1] = 10 ** 9
    with pytest.raises(IndexError):
        _rag(lm, dev, "tse", e2, m2, g, s3, NE, NM, T_)
    s3 = s2.clone()
    s3[4, 0] = -R.SMALL.semantic_offset - 1
    with pytest.raises(IndexError):
        _rag(lm, dev, "tse", e2, m2, g, s3, NE, NM, T_)


def test_all_equal_lengths_are_the_rectangular_call(qa_lib, gpu_device):
    """(5) uniform vectors at full width: qa_lm_score's own bits, the tap's shape included; a missing vector means full width."""
    dev = gpu_device
    _, lm = _model(R.SMALL, RR.CASE_SEED, dev)
    enr, mix, g, s = RR.case_inputs()
    enr, mix, s = enr[:, :11].contiguous(), mix[:, :14].contiguous(), s[:, :9].contiguous()
    B = mix.shape[0]
    rect = _score(lm, dev, "tse", enr, mix, g, s)
    for ne, nm, T in (([11] * B, [14] * B, [9] * B), (None, [14] * B, None), ([11] * B, None, None), (None, None, [9] * B)):
        got = _rag(lm, dev, "tse", enr, mix, g, s, ne, nm, T)
        assert torch.equal(got[0], rect[0]) and torch.equal(got[1], rect[1]) and got[2:4] == rect[2:4]
        assert lm.tap("logits.forced").numel() == rect[4].numel()
        assert torch.equal(torch.stack(got[4]), rect[4])
    # only some of the vectors, not uniform: the missing ones mean full width
    nm = [14, 3, 14, 9, 1, 14]
    part = _rag(lm, dev, "tse", enr, mix, g, s, None, nm, None)
    full = _rag(lm, dev, "tse", enr, mix, g, s, [11] * B, nm, [9] * B)
    assert torch.equal(part[0], full[0]) and torch.equal(part[1], full[1]) and all(torch.equal(a, b) for a, b in zip(part[4], full[4]))
    for b in (1, 4):
        _same_row(part, b, _alone(lm, dev, "tse", enr, mix, g, s, [11] * B, nm, [9] * B, b), "partial vectors")
    # forward / score: the public keywords, pooled and per row
    mel = torch.zeros(B, 1, 80)
    kw = dict(task_name="tse", enroll_mel=mel, enroll_feats=enr.to(dev), mix_mel=mel, mix_feats=mix.to(dev), global_ids=g.to(dev),
              semantic_ids=s.to(dev))
    loss, acc = lm(**kw, mix_lengths=torch.tensor(nm))
    assert float(loss) == part[2] and float(acc) == part[3] and loss.dim() == 0
    ls, accs = lm.score(**kw, mix_lengths=nm)
    assert torch.equal(ls.cpu(), part[0]) and torch.equal(accs.cpu(), part[1].float() / (G_ + 9 + 2))


@pytest.mark.parametrize("task", ["tse", "se"])
def test_build_prompt_with_lengths_feeds_a_session(qa_lib, gpu_device, task):
    """(6) row b's first Lp_b positions are build_prompt of the row alone, exact zeros behind, NaN-poisoned padding frames; the result
    with chunk_lengths = Lp on a KVCache gives the last_hidden rows of the row-alone session call."""
    import unified_audio_amd as qa

    dev = gpu_device
    _, lm = _model(R.SMALL, RR.CASE_SEED, dev)
    enr, mix, _, _ = RR.case_inputs()
    enr = enr if task == "tse" else None
    B = len(NM)
    lp, _, _ = RR.positions(NE, NM, [0] * B, 0, enroll=enr is not None)
    m2 = mix.clone()
    e2 = None if enr is None else enr.clone()
    for b in range(B):
        m2[b, NM[b]:] = float("nan")
        if e2 is not None:
            e2[b, NE[b]:] = float("nan")
    kw = dict(mix_lengths=NM) if enr is None else dict(mix_lengths=NM, enroll_lengths=NE)
    out = lm.build_prompt(task, None if e2 is None else e2.to(dev), m2.to(dev), **kw)
    assert out.shape == (B, 1 + (1 + max(NE) if enr is not None else 0) + 1 + max(NM), R.SMALL.hidden)
    cache = qa.KVCache(lm, B, out.shape[1])
    hid = lm.llm_forward(out, past_key_values=cache, use_cache=True, chunk_lengths=lp).last_hidden_state
    assert cache.get_seq_lengths() == lp
    for b in range(B):
        one = lm.build_prompt(task, None if enr is None else enr[b:b + 1, :NE[b]].to(dev), mix[b:b + 1, :NM[b]].to(dev))
        assert one.shape[1] == lp[b]
        assert torch.equal(out[b, :lp[b]], one[0]), b
        assert not out[b, lp[b]:].any(), b
        solo = qa.KVCache(lm, 1, lp[b])
        assert torch.equal(hid[b, :lp[b]], lm.llm_forward(one, past_key_values=solo, use_cache=True).last_hidden_state[0]), b
        solo.free()
    # uniform vectors at full width are build_prompt itself
    full = lm.build_prompt(task, None if enr is None else enr.to(dev), mix.to(dev))
    kw = dict(mix_lengths=[max(NM)] * B) if enr is None else dict(mix_lengths=[max(NM)] * B, enroll_lengths=[max(NE)] * B)
    assert torch.equal(lm.build_prompt(task, None if enr is None else enr.to(dev), mix.to(dev), **kw), full)


@pytest.mark.parametrize("mode", ["se", "tse", "rtse"])
def test_validation_step_with_lengths(qa_lib, gpu_device, mode):
    """(7) validation_step(use_lengths=True) is the ragged forward on tokenize(lengths=) / semantic_model(lengths=); the default is today's."""
    from unified_audio_amd import synth

    dev = gpu_device
    model, tok, fx, lm = _validation_model(dev)
    B, lens = 3, [16000, 9000, 12345]
    speech = synth.synth_wav(111, B, 16000).to(dev)
    interf = synth.synth_wav(112, B, 16000).to(dev)
    mix = (speech + 0.5 * interf).contiguous()
    enroll = synth.synth_wav(113, B, 12000).to(dev) if mode != "se" else None
    batch = (mode, enroll, mix, speech, interf, torch.tensor([16000] * B), torch.tensor(lens), ["a", "b", "c"])
    out = model.validation_step(batch, 0, use_lengths=True)
    assert set(out) == {"valid_loss", "valid_acc"} and out["valid_loss"].dim() == 0
    glob, sem = tok.tokenize(interf if mode == "rtse" else speech, lengths=lens)
    mel = torch.zeros(B, 1, 80)
    e_mel, e_feats = (None, None) if enroll is None else (mel, fx(enroll))
    loss, acc = lm(mode, e_mel, e_feats, mel, fx(mix, lengths=lens), glob.squeeze(1), sem, mix_lengths=[fx.frames(n) for n in lens],
                   semantic_lengths=tok.token_frames(lens))
    assert torch.equal(out["valid_loss"], loss) and torch.equal(out["valid_acc"], acc)
    assert torch.isfinite(loss) and 0.0 <= float(acc) <= 1.0
    plain = model.validation_step(batch, 0)
    assert not torch.equal(plain["valid_loss"], loss)
    g0, s0 = tok.tokenize(interf if mode == "rtse" else speech)
    loss0, acc0 = lm(mode, e_mel, e_feats, mel, fx(mix), g0.squeeze(1), s0)  # today's path: the lengths are ignored
    assert torch.equal(plain["valid_loss"], loss0) and torch.equal(plain["valid_acc"], acc0)
    assert torch.equal(model.validation_step(batch, 0, use_lengths=False)["valid_loss"], loss0)

    class NoLengths:  # a component that cannot take lengths is named
        def __call__(self, wavs):
            return fx(wavs)

    model.semantic_model = NoLengths()
    with pytest.raises(TypeError, match="semantic model needs"):
        model.validation_step(batch, 0, use_lengths=True)


def test_errors_leave_the_handle_usable(qa_lib, gpu_device):
    """(8) every refusal names its cause (row and value) before anything is launched; the handle then gives the bits it gave before;
    generate and a session call around a ragged score call are undisturbed."""
    import unified_audio_amd as qa
    from tests.test_lm_session_gpu import _embeds, _feed
    from unified_audio_amd import _lib

    spec, dev = R.SMALL, gpu_device
    sd, lm = _model(spec, RR.CASE_SEED, dev)
    enr, mix, g, s = RR.case_inputs()
    want = _rag(lm, dev, "tse", enr, mix, g, s, NE, NM, T_)

    def good():
        got = _rag(lm, dev, "tse", enr, mix, g, s, NE, NM, T_)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and got[2:4] == want[2:4]
        assert all(torch.equal(a, b) for a, b in zip(got[4], want[4]))

    def bad(vec, i, v):
        out = list(vec)
        out[i] = v
        return out

    with pytest.raises(qa.QuarkAudioError, match=r"n_mix\[2\] = 130 is outside 1 \.\. n_mix_max = 129"):
        _rag(lm, dev, "tse", enr, mix, g, s, NE, bad(NM, 2, 130), T_)
    good()
    with pytest.raises(qa.QuarkAudioError, match=r"n_mix\[0\] = 0 is outside"):
        _rag(lm, dev, "tse", enr, mix, g, s, NE, bad(NM, 0, 0), T_)
    with pytest.raises(qa.QuarkAudioError, match=r"n_enroll\[1\] = 0 is outside 1 \.\. n_enroll_max = 40"):
        _rag(lm, dev, "tse", enr, mix, g, s, bad(NE, 1, 0), NM, T_)
    with pytest.raises(qa.QuarkAudioError, match=r"n_enroll\[5\] = 41 is outside"):
        _rag(lm, dev, "tse", enr, mix, g, s, bad(NE, 5, 41), NM, T_)
    with pytest.raises(qa.QuarkAudioError, match=r"n_semantic\[3\] = 127 is outside 0 \.\. semantic_length_max = 126"):
        _rag(lm, dev, "tse", enr, mix, g, s, NE, NM, bad(T_, 3, 127))
    with pytest.raises(qa.QuarkAudioError, match=r"n_semantic\[0\] = -1 is outside"):
        _rag(lm, dev, "tse", enr, mix, g, s, NE, NM, bad(T_, 0, -1))
    good()
    with pytest.raises(qa.QuarkAudioError, match=r"n_enroll given \(n_enroll\[0\] = 3\) without an enrollment"):
        _rag(lm, dev, "se", None, mix, g, s, NE, NM, T_)
    with pytest.raises(qa.QuarkAudioError, match="5 entries for a batch of 6"):
        _rag(lm, dev, "tse", enr, mix, g, s, NE, NM[:5], T_)
    with pytest.raises(KeyError):
        _rag(lm, dev, "denoise", enr, mix, g, s, NE, NM, T_)
    # the longest row above max_position_embeddings: 2 + 4000 + (4 + 100 + 2) = 4108 positions in row 1 alone
    long_mix = L.synth_feats(95, 2, 4000, spec.feats_dim)
    with pytest.raises(qa.QuarkAudioError, match=r"row 1 holds 4108 positions .* max_position_embeddings 4096"):
        _rag(lm, dev, "se", None, long_mix, g[:2], torch.zeros(2, 100, dtype=torch.int64), None, [10, 4000], [5, 100])
    short = _rag(lm, dev, "se", None, long_mix, g[:2], torch.zeros(2, 100, dtype=torch.int64), None, [10, 20], [5, 100])  # the rows decide
    assert torch.isfinite(short[0]).all()
    good()
    # a NULL pointer where data is needed (the C entry itself)
    out = torch.empty(16, dtype=torch.float32, device=dev)
    arr = (C.c_int64 * 1)(3)
    st = qa_lib.qa_lm_score_ragged(lm._handle, 0, None, 0, None, None, 5, arr, 1, None, 0, None, 0, None, 0.1, out.data_ptr(),
                                   out[4:].data_ptr(), out[8:].data_ptr(), out[9:].data_ptr(), None)
    with pytest.raises(qa.QuarkAudioError, match="qa_lm_score_ragged: null argument"):
        _lib.check(st)
    st = qa_lib.qa_lm_prompt_ragged(lm._handle, 0, None, 0, None, None, 5, arr, 1, out.data_ptr(), None)
    with pytest.raises(qa.QuarkAudioError, match="qa_lm_prompt_ragged: null argument"):
        _lib.check(st)
    with pytest.raises(qa.QuarkAudioError, match=r"qa_lm_prompt_ragged: n_mix\[4\] = 200 is outside 1 \.\. n_mix_max = 129"):
        lm.build_prompt("tse", enr.to(dev), mix.to(dev), enroll_lengths=NE, mix_lengths=bad(NM, 4, 200))
    good()
    # a caller's stream capture: refused with the reason (the lengths are host data)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    graph = torch.cuda.CUDAGraph()
    mel = torch.zeros(6, 1, 80)
    e_d, m_d, g_d, s_d = enr.to(dev), mix.to(dev), g.to(dev).long(), s.to(dev)
    loss_seq, correct, two = torch.empty(6, device=dev), torch.empty(6, dtype=torch.int64, device=dev), torch.empty(2, device=dev)
    nm_arr = (C.c_int64 * 6)(*NM)
    with pytest.raises(qa.QuarkAudioError, match="stream capture"):
        with torch.cuda.graph(graph, stream=side):
            _lib.check(qa_lib.qa_lm_score_ragged(lm._handle, 1, e_d.data_ptr(), e_d.shape[1], None, m_d.data_ptr(), m_d.shape[1], nm_arr, 6,
                                                 g_d.data_ptr(), G_, s_d.data_ptr(), s_d.shape[1], None, 0.1, loss_seq.data_ptr(),
                                                 correct.data_ptr(), two.data_ptr(), two[1:].data_ptr(),
                                                 torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize()
    good()
    # neighbours: generate and a session around a ragged score call
    S = 8
    gmel = torch.zeros(6, S, 80)

    def gen():
        a, b = lm.generate("tse", gmel, e_d, gmel, m_d[:, :9].contiguous(), global_length=G_, do_sample=False)
        return a.cpu(), b.cpu()

    g0 = gen()
    x = _embeds(sd, spec, 6, 5, 12)
    schedule = [7, 1, 3, 1]
    cache = qa.KVCache(lm, 5, 16)
    first = _feed(lm, dev, cache, x, schedule)
    cache.reset()
    a = _feed(lm, dev, cache, x, schedule[:2])
    good()
    b = _feed(lm, dev, cache, x[:, 8:], schedule[2:])
    assert torch.equal(torch.cat([a, b], dim=1), first)
    g1 = gen()
    assert all(torch.equal(p, q) for p, q in zip(g0, g1))
    good()
