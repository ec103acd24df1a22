"""GPU tests of the condition path with per-row lengths: log-mel, the convolution module's kernel alone, the
Conformer condition encoder, CustomLlamaModel.generate and forward / score.

One meaning everywhere: row b behaves as the rectangular call would for that clip ALONE at its own length; what the tensors hold at or
behind a row's length is never read (NaN there changes nothing); what the call writes behind a row's length is exactly 0.0f.

Metrics and margins are those of tests/test_lm_cond_gpu.py: e = max|y - y64| / rms(y64) against the float64 restatement with bound
4 * max(e_cpu32, 1e-6); per-sequence loss 4e-6 relative; tokens by _audit's near-tie bar of 2e-4.  The oracle is
tests/lm_cond_ragged_ref.py: the rectangular restatement on x[b:b+1, :L_b], one row at a time."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import conformer_ref as R
from tests import front_kernels_ref as K
from tests import lm_cond_ragged_ref as RR
from tests.test_front_kernels_gpu import HEAD, _dev, _finish, _gen, _glu_dw_operands, _p, _parity, _stream
from tests.test_llm_gpu import SMALL
from tests.test_lm_cond_gpu import SMALL_CF, UNISE_CF, _audit, _check, _custom, _encoder, _weights
from tests.util import guarded_out
from unified_audio_amd import synth

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _nan_behind(x, lengths):
    y = x.clone()
    for b, n in enumerate(lengths):
        y[b, n:] = NAN
    return y


def _arr(v):
    return (C.c_int64 * len(v))(*v)


# ------------------------------------------------------------------------------------------------------------ 1  log-mel

LOGMEL_LENS = [1083, 1, 320, 321, 480]  # full; one frame; an exact hop multiple; one sample more; the middle of a window


def test_logmel_lengths(qa_lib, gpu_device):
    from unified_audio_amd import unise

    wav = synth.synth_wav(5, 5, 1083)
    got = unise.stft_logmel(wav.to(gpu_device), lengths=LOGMEL_LENS)
    assert got.shape == (5, RR.frames(1083), 80)
    o64, o32 = RR.stft_logmel(wav, LOGMEL_LENS, dtype=torch.float64), RR.stft_logmel(wav, LOGMEL_LENS)
    for b, n in enumerate(LOGMEL_LENS):
        F = RR.frames(n)
        _check(got[b, :F], o64[b, :F], o32[b, :F], f"logmel row {b} of {n} samples")
        assert torch.equal(got[b, F:], torch.zeros_like(got[b, F:])), f"row {b}: the frames behind {F} are not exactly 0"
    holes = unise.stft_logmel(_nan_behind(wav, LOGMEL_LENS).to(gpu_device), lengths=LOGMEL_LENS)
    assert torch.equal(holes, got), "NaN behind a row's samples reached the output"
    assert torch.equal(unise.stft_logmel(wav.to(gpu_device), lengths=[1083] * 5), unise.stft_logmel(wav.to(gpu_device)))
    assert torch.equal(unise.stft_logmel(wav.to(gpu_device), lengths=torch.tensor(LOGMEL_LENS)), got)


# ------------------------------------------------------------------------------------------------------------ 2  glu_dwconv alone

GDW_LENS = [130, 1, 15, 16, 31, 33, 64, 65, 129]  # the halo width, both sides of the 64-frame tile edge, a whole dead tile (rows of <= 64)


@pytest.fixture(scope="module")
def gdw_hook(qa_lib):
    fn = qa_lib.qa_debug_glu_dwconv_bn_silu_rows
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p] * 6 + [C.c_int] * 3 + [C.c_void_p, C.c_void_p]
    return qa_lib


def _glu_dw_rows(lib, dev, u, w, bias, bn, lens):
    B, T, C2 = u.shape
    Cc = C2 // 2
    sc, sh = K.pack_batchnorm(*bn)
    buf, y = guarded_out(B * T, Cc, Cc, HEAD, dev)
    ud, wd, bd, scd, shd = _dev(dev, u, K.pack_dw31(w), bias, sc, sh)
    ld = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=dev)
    st = lib.qa_debug_glu_dwconv_bn_silu_rows(_p(ud), _p(wd), _p(bd), _p(scd), _p(shd), _p(y), B, T, Cc, _p(ld), _stream())
    return _finish(lib, st, buf, y, (B, T, Cc))


@pytest.mark.parametrize("k", [31, 3])
@pytest.mark.parametrize("Cc", [64, 96])
def test_glu_dwconv_rows(gdw_hook, gpu_device, Cc, k):
    B, T = 9, 130
    u, w, bias, bn = _glu_dw_operands(_gen(7000 + Cc + k), B, T, Cc, k)
    y = _glu_dw_rows(gdw_hook, gpu_device, u, w, bias, bn, GDW_LENS)
    ref, yard = torch.full((B, T, Cc), NAN, dtype=torch.float64), torch.full((B, T, Cc), NAN)
    for b, n in enumerate(GDW_LENS):  # the closed form on the row alone at its own length
        ref[b, :n] = K.glu_dwconv_bn_silu_ref(u[b:b + 1, :n], w, bias, *bn)[0]
        yard[b, :n] = K.glu_dwconv_bn_silu_torch(u[b:b + 1, :n], w, bias, *bn)[0]
        assert torch.equal(y[b, n:], torch.zeros(T - n, Cc)), f"row {b}: the frames behind {n} are not exactly 0"
    _parity(f"glu_dwconv rows C {Cc} k {k}", y, ref, yard)
    assert torch.equal(_glu_dw_rows(gdw_hook, gpu_device, _nan_behind(u, GDW_LENS), w, bias, bn, GDW_LENS), y), "NaN behind a row's frames was read"
    # null rows and full rows are the kernel as it was: the bits of the existing hook
    from tests.test_front_kernels_gpu import HOOKS

    plain = gdw_hook.qa_debug_glu_dwconv_bn_silu
    plain.restype, plain.argtypes = HOOKS["qa_debug_glu_dwconv_bn_silu"]
    sc, sh = K.pack_batchnorm(*bn)
    buf, yp = guarded_out(B * T, Cc, Cc, HEAD, gpu_device)
    ops = _dev(gpu_device, u, K.pack_dw31(w), bias, sc, sh)
    full = _finish(gdw_hook, plain(*[_p(t) for t in ops], _p(yp), B, T, Cc, _stream()), buf, yp, (B, T, Cc))
    assert torch.equal(_glu_dw_rows(gdw_hook, gpu_device, u, w, bias, bn, None), full)
    assert torch.equal(_glu_dw_rows(gdw_hook, gpu_device, u, w, bias, bn, [T] * B), full)
    for b, n in enumerate(GDW_LENS):  # a row among other lengths == the row alone
        if n < T:
            alone = _glu_dw_rows(gdw_hook, gpu_device, u[b:b + 1], w, bias, bn, [n])
            assert torch.equal(alone[0], y[b]), f"row {b} alone differs from the row in the batch"


# ------------------------------------------------------------------------------------------------------------ 3  encoder

ENC_LENS = [130, 1, 15, 16, 31, 32, 33, 64, 65]  # 31 / 32 / 33 straddle the attention's 32-key tile


@functools.lru_cache(maxsize=None)
def _enc_case(pe):
    """(params, sd, x, oracle float64, oracle float32, taps64, taps32): computed once, shared, never modified"""
    params = dict(SMALL_CF, pe_attn_head=pe)
    sd = synth.conformer_state_dict(33, params)
    x = torch.from_numpy(np.random.default_rng(8).standard_normal((9, 130, 64)).astype("float32"))
    t64, t32 = {}, {}
    y64 = RR.conformer_encoder(sd, params, x, ENC_LENS, dtype=torch.float64, taps=t64)
    y32 = RR.conformer_encoder(sd, params, x, ENC_LENS, taps=t32)
    return params, sd, x, y64, y32, t64, t32


@pytest.mark.parametrize("pe", [None, 1])
def test_encoder_lengths(qa_lib, gpu_device, pe):
    params, sd, x, y64, y32, t64, t32 = _enc_case(pe)
    _, enc = _encoder(params, 33, gpu_device)
    B, T = 9, 130
    xd = x.to(gpu_device)
    enc.enable_taps(True)
    got = enc(xd, lengths=ENC_LENS)
    taps = {name: enc.tap(name).view(B, T, 64).clone() for name in t64}
    enc.enable_taps(False)
    for b, n in enumerate(ENC_LENS):
        for name in t64:
            _check(taps[name][b, :n], t64[name][b, :n], t32[name][b, :n], f"pe={pe} row {b} ({n}) {name}")
        _check(got[b, :n], y64[b, :n], y32[b, :n], f"pe={pe} row {b} ({n}) output")
        assert torch.equal(got[b, n:], torch.zeros_like(got[b, n:])), f"row {b}: the output behind {n} is not exactly 0"
        for name in t64:
            if name.endswith(".attn"):
                assert torch.equal(taps[name][b, n:], torch.zeros_like(taps[name][b, n:])), f"{name} row {b}"
    assert torch.equal(enc(_nan_behind(x, ENC_LENS).to(gpu_device), lengths=ENC_LENS), got), "NaN behind a row's frames reached the output"
    # a row's bits do not depend on its neighbours' lengths, nor on having neighbours at all
    other = [n if b % 2 == 0 else max(1, (n * 7) % 130) for b, n in enumerate(ENC_LENS)]
    assert other != ENC_LENS
    got2 = enc(xd, lengths=other)
    for b in range(0, B, 2):
        assert torch.equal(got2[b], got[b]), f"row {b} changed with its neighbours' lengths"
    for b in (1, 4, 6, 8):
        alone = enc(xd[b:b + 1], lengths=[ENC_LENS[b]])
        assert torch.equal(alone[0], got[b]), f"row {b} alone at T = {T} differs from the row in the batch"
    # full lengths are the call without a mask and without lengths
    assert torch.equal(enc(xd, lengths=[T] * B), enc(xd))


def test_condition_encoder_lengths_at_unise_size(qa_lib, gpu_device):
    from unified_audio_amd.conformer import ConditionEncoder

    B, T, lens = 4, 250, [250, 100, 33, 249]
    sd = synth.cond_encoder_state_dict(51, 80, 512, UNISE_CF)
    enc = ConditionEncoder(80, 512, UNISE_CF, device=gpu_device).load_state_dict({"dnn." + k: v for k, v in sd.items()})
    mel = synth.synth_logmel(9, B, T)
    got = enc(mel.to(gpu_device), lengths=lens)
    y64, y32 = RR.condition(sd, UNISE_CF, mel, lens, dtype=torch.float64), RR.condition(sd, UNISE_CF, mel, lens)
    for b, n in enumerate(lens):
        _check(got[b, :n], y64[b, :n], y32[b, :n], f"UniSE condition encoder row {b} ({n})")
        assert torch.equal(got[b, n:], torch.zeros_like(got[b, n:]))
    assert torch.equal(enc(_nan_behind(mel, lens).to(gpu_device), lengths=lens), got)
    assert torch.equal(enc(mel.to(gpu_device), lengths=[T] * B), enc(mel.to(gpu_device)))


# ------------------------------------------------------------------------------------------------------------ 4  generate

GEN_LENS = [20, 1, 7, 13]


def _gen_model(dev, seed=71):
    sd = _weights(SMALL, SMALL_CF, seed)
    return sd, _custom(SMALL, SMALL_CF, dev).load_state_dict({"dnn." + k: v for k, v in sd.items()})


def test_generate_cond_lengths(qa_lib, gpu_device):
    sd, m = _gen_model(gpu_device)
    B, T, G, S = 4, 20, 6, 14
    cond = synth.synth_logmel(11, B, T)
    cd = cond.to(gpu_device)

    def run(c, lens, **kw):
        m.enable_taps(True)
        g, s = m.generate(c, global_length=G, semantic_length=S, do_sample=False, cond_lengths=lens, **kw)
        return g, s, m.tap("logits.global").view(-1, G, SMALL.global_size).clone(), m.tap("logits.semantic").view(-1, S, SMALL.semantic_size).clone()

    gids, sids, zg, zs = run(cd, GEN_LENS)
    assert gids.shape == (B, G) and sids.shape == (B, S) and gids.dtype == torch.int64
    for b, n in enumerate(GEN_LENS):  # every row audited against the restatement on its own slice
        free, ties = _audit(sd, SMALL, SMALL_CF, cond[b:b + 1, :n], 1, G, S, gids[b:b + 1].cpu(), sids[b:b + 1].cpu())
        print(f"row {b} ({n} frames): free-running agreement {free}, near-tie flips {ties}")
        assert ties > 0 or free == 1.0
        g1, s1, zg1, zs1 = run(cd[b:b + 1], [n])  # the row alone at the same T_max
        assert torch.equal(g1[0], gids[b]) and torch.equal(s1[0], sids[b]), f"row {b} alone: other tokens"
        assert torch.equal(zg1[0], zg[b]) and torch.equal(zs1[0], zs[b]), f"row {b} alone: other logits"
    # the lengths are live: row 2 is not what the full-width condition gives
    full = run(cd, None)
    assert not (torch.equal(full[2][2], zg[2]) and torch.equal(full[3][2], zs[2]))
    for a, b_ in zip(run(_nan_behind(cond, GEN_LENS).to(gpu_device), GEN_LENS), (gids, sids, zg, zs)):
        assert torch.equal(a, b_), "NaN behind a row's frames reached the tokens or the logits"
    for a, b_ in zip(run(cd, [T] * B), full):
        assert torch.equal(a, b_), "full lengths are not generate(cond)"
    m.enable_taps(False)
    torch.manual_seed(5)
    a = m.generate(cd, global_length=G, semantic_length=S, do_sample=True, cond_lengths=GEN_LENS)
    torch.manual_seed(5)
    b2 = m.generate(cd, global_length=G, semantic_length=S, do_sample=True, cond_lengths=GEN_LENS)
    assert torch.equal(a[0], b2[0]) and torch.equal(a[1], b2[1])
    assert int(a[0].min()) >= 0 and int(a[0].max()) < SMALL.global_size and int(a[1].min()) >= 0 and int(a[1].max()) < SMALL.semantic_size


# ------------------------------------------------------------------------------------------------------------ 5  score

SC_COND, SC_SEM = [18, 1, 9, 18], [11, 0, 5, 11]


@pytest.mark.parametrize("which", ["both", "cond", "semantic"])
@pytest.mark.parametrize("eps", [0.1, 0.0])
def test_score_cond_lengths(qa_lib, gpu_device, eps, which):
    sd = _weights(SMALL, SMALL_CF, 91)
    m = _custom(SMALL, SMALL_CF, gpu_device, label_smoothing=eps).load_state_dict(sd)
    B, G, T, Tc = 4, 6, 11, 18
    gen = torch.Generator().manual_seed(17)
    g = torch.randint(0, SMALL.global_size, (B, G), generator=gen, dtype=torch.int32)
    s = torch.randint(0, SMALL.semantic_size, (B, T), generator=gen, dtype=torch.int64)
    cond = synth.synth_logmel(13, B, Tc)
    cl = SC_COND if which in ("both", "cond") else None
    sl = SC_SEM if which in ("both", "semantic") else None
    # padding that must never be read: NaN frames, ids outside the vocabulary
    cond_in, s_in = cond.clone(), s.clone()
    if cl is not None:
        cond_in = _nan_behind(cond, cl)
    if sl is not None:
        for b, n in enumerate(sl):
            s_in[b, n:] = SMALL.semantic_size + 5
    dc = cond_in.to(gpu_device)
    m.enable_taps(True)
    loss, acc = m(g, s_in, dc, cond_lengths=cl, semantic_lengths=sl)
    z = m.tap("logits.forced").view(-1, SMALL.vocab).cpu()
    loss_seq, acc_seq = m.score(g, s_in, dc, cond_lengths=cl, semantic_lengths=sl)
    r64 = RR.score(sd, SMALL, SMALL_CF, g, s, cond, cl, sl, eps, dtype=torch.float64)
    r32 = RR.score(sd, SMALL, SMALL_CF, g, s, cond, cl, sl, eps)
    Lt = [G + (T if sl is None else sl[b]) + 1 for b in range(B)]
    assert z.shape[0] == sum(Lt), "logits.forced is not packed over the rows' own target counts"
    off, kl_sum, ok_sum, slack_sum = 0, 0.0, 0.0, 0
    for b in range(B):
        zb = z[off:off + Lt[b]]
        off += Lt[b]
        _check(zb, r64[b]["logits"][0], r32[b]["logits"][0], f"{which} eps={eps} row {b} forced logits ({Lt[b]} rows)")
        rel = abs(float(loss_seq[b]) - float(r64[b]["loss_seq"][0])) / abs(float(r64[b]["loss_seq"][0]))
        print(f"row {b}: per-sequence loss relative error {rel:.3e} (bound 4e-6)")
        assert rel <= 4e-6
        top2 = r64[b]["logits"][0].topk(2, dim=-1).values
        decisive = (top2[..., 0] - top2[..., 1]) > 2e-4
        am = R.SR.first_argmax(zb)
        assert torch.equal(am[decisive], r64[b]["argmax"][0][decisive])
        slack = int((~decisive).sum())
        correct = round(float(acc_seq[b]) * Lt[b])
        assert abs(correct - int(r64[b]["correct"][0])) <= slack
        kl_sum += float(r64[b]["row_kl"].sum())
        ok_sum += float(r64[b]["correct"][0])
        slack_sum += slack
    # pooled over all sum Lt_b target rows
    assert abs(float(loss) - kl_sum / sum(Lt)) <= 4e-6 * abs(kl_sum / sum(Lt))
    assert abs(float(acc) * sum(Lt) - ok_sum) <= slack_sum + 1e-3
    # a row alone == the row in the batch
    for b in (1, 2):
        l1, a1 = m.score(g[b:b + 1], s_in[b:b + 1], dc[b:b + 1], cond_lengths=None if cl is None else [cl[b]],
                         semantic_lengths=None if sl is None else [sl[b]])
        assert torch.equal(l1[0], loss_seq[b]) and torch.equal(a1[0], acc_seq[b]), f"row {b} alone differs from the row in the batch"
    # uniform vectors are the rectangular call
    dfull = cond.to(gpu_device)
    lr, ar = m.score(g, s, dfull)
    zr = m.tap("logits.forced").clone()
    lu, au = m.score(g, s, dfull, cond_lengths=None if cl is None else [Tc] * B, semantic_lengths=None if sl is None else [T] * B)
    assert torch.equal(lu, lr) and torch.equal(au, ar) and torch.equal(m.tap("logits.forced"), zr)


# ------------------------------------------------------------------------------------------------------------ 6  refusals

def test_refusals_name_the_row_and_leave_the_handles_usable(qa_lib, gpu_device):
    import unified_audio_amd as qa
    from unified_audio_amd import _lib, unise

    dev = gpu_device
    sd, m = _gen_model(dev, 91)
    _, enc = _encoder(SMALL_CF, 33, dev)
    B, T, G, S = 3, 20, 4, 5
    cond = synth.synth_logmel(11, B, T).to(dev)
    x = torch.randn(B, T, 64, generator=torch.Generator().manual_seed(1)).to(dev)
    wav = synth.synth_wav(5, B, 1083).to(dev)
    gen = torch.Generator().manual_seed(3)
    g = torch.randint(0, SMALL.global_size, (B, G), generator=gen)
    s = torch.randint(0, SMALL.semantic_size, (B, S), generator=gen)

    def rectangular():
        m.enable_taps(True)
        gi, si = m.generate(cond, global_length=G, semantic_length=S, do_sample=False)
        zg = m.tap("logits.global").clone()
        ls, ac = m.score(g, s, cond)
        return gi, si, zg, ls, ac, m.tap("logits.forced").clone(), enc(x), unise.stft_logmel(wav)

    before = rectangular()

    def good():
        for a, b_ in zip(rectangular(), before):
            assert torch.equal(a, b_), "a refused call changed what the next rectangular call computes"

    def poisoned(shape, dtype=torch.float32):  # an output a refused call must not touch
        return torch.full(shape, NAN if dtype == torch.float32 else -7, dtype=dtype, device=dev)

    stream = torch.cuda.current_stream(dev).cuda_stream
    for bad, text in ((0, "= 0 is outside 1"), (T + 1, f"= {T + 1} is outside 1")):
        lens = [T, bad, 5]
        out = poisoned((B, T, 64))
        st = qa_lib.qa_conformer_forward_ragged(enc._handle, x.data_ptr(), _arr(lens), B, T, out.data_ptr(), stream)
        with pytest.raises(qa.QuarkAudioError, match=r"qa_conformer_forward_ragged: lengths\[1\] " + text):
            _lib.check(st)
        torch.cuda.synchronize()
        assert torch.isnan(out).all(), "a refused call launched something"
        with pytest.raises(qa.QuarkAudioError, match=r"qa_cond_encoder_forward_ragged: lengths\[1\] " + text):
            m.encode_condition(cond, lens)
        gi, si = poisoned((B, G), torch.int64), poisoned((B, S), torch.int64)
        emb = m.encode_condition(cond)
        st = qa_lib.qa_lm_generate_cond_ragged(m.lm._handle, emb.data_ptr(), T, _arr(lens), B, G, S, 0.8, 50, 0.95, gi.data_ptr(), si.data_ptr(),
                                               stream)
        with pytest.raises(qa.QuarkAudioError, match=r"qa_lm_generate_cond_ragged: n_cond\[1\] " + text):
            _lib.check(st)
        torch.cuda.synchronize()
        assert bool((gi == -7).all()) and bool((si == -7).all())
        ls, co, two = poisoned((B,)), poisoned((B,), torch.int64), poisoned((2,))
        gd, sd_ = g.to(dev), s.to(dev)
        st = qa_lib.qa_lm_score_cond_ragged(m.lm._handle, emb.data_ptr(), T, _arr(lens), B, gd.data_ptr(), G, sd_.data_ptr(), S, None, 0.1,
                                            ls.data_ptr(), co.data_ptr(), two.data_ptr(), two[1:].data_ptr(), stream)
        with pytest.raises(qa.QuarkAudioError, match=r"qa_lm_score_cond_ragged: n_cond\[1\] " + text):
            _lib.check(st)
        torch.cuda.synchronize()
        assert torch.isnan(ls).all() and torch.isnan(two).all() and bool((co == -7).all())
        good()
    with pytest.raises(qa.QuarkAudioError, match=r"qa_logmel_ragged: lengths\[2\] = 0 is outside 1 \.\. n = 1083"):
        unise.stft_logmel(wav, lengths=[1083, 5, 0])
    with pytest.raises(qa.QuarkAudioError, match=r"qa_logmel_ragged: lengths\[0\] = 1084 is outside"):
        unise.stft_logmel(wav, lengths=[1084, 5, 7])
    with pytest.raises(qa.QuarkAudioError, match=r"n_semantic\[2\] = 6 is outside 0 \.\. semantic_length_max = 5"):
        m.score(g, s, cond, semantic_lengths=[5, 0, 6])
    with pytest.raises(qa.QuarkAudioError, match=r"n_semantic\[0\] = -1 is outside"):
        m.score(g, s, cond, semantic_lengths=[-1, 0, 5])
    with pytest.raises(qa.QuarkAudioError, match="entries for a batch of 3"):
        enc(x, lengths=[T, 5])
    good()
    # mask with lengths
    with pytest.raises(qa.QuarkAudioError, match="mask and lengths"):
        enc(x, torch.ones(B, T, dtype=torch.bool), lengths=[T, 3, 5])
    # lengths without a condition
    with pytest.raises(qa.QuarkAudioError, match=r"qa_lm_generate_cond_ragged: n_cond given \(n_cond\[0\] = 4\) without a condition"):
        m.generate(None, global_length=G, semantic_length=S, do_sample=False, batch_size=2, cond_lengths=[4, 2])
    with pytest.raises(qa.QuarkAudioError, match=r"qa_lm_score_cond_ragged: n_cond given \(n_cond\[0\] = 4\) without a condition"):
        m.score(g, s, None, cond_lengths=[4, 2, 1])
    good()
    # 4097 positions: 1 + T_max + G + 1 + S in generate, a row's prompt + targets in score
    with pytest.raises(qa.QuarkAudioError, match="4097 positions"):
        m.generate(cond, global_length=G, semantic_length=4096 - 1 - T - G, do_sample=False, cond_lengths=[T, 3, 5])
    long_s = torch.zeros(B, 4097 - (1 + T) - (G + 1), dtype=torch.int64)
    with pytest.raises(qa.QuarkAudioError, match=r"row 0 holds 4097 positions"):
        m.score(g, long_s, cond, cond_lengths=[T, 3, 5])
    good()
    # a caller's stream capture: refused with the reason (the lengths are host data)
    emb = m.encode_condition(cond)
    gd, sd_ = g.to(dev), s.to(dev)
    out, mel_out = poisoned((B, T, 64)), poisoned((B, RR.frames(1083), 80))
    gi, si = poisoned((B, G), torch.int64), poisoned((B, S), torch.int64)
    ls, co, two = poisoned((B,)), poisoned((B,), torch.int64), poisoned((2,))
    lens = _arr([T, 3, 5])
    wlens = _arr([1083, 1, 320])
    calls = {
        "qa_conformer_forward_ragged": lambda st: qa_lib.qa_conformer_forward_ragged(enc._handle, x.data_ptr(), lens, B, T, out.data_ptr(), st),
        "qa_logmel_ragged": lambda st: qa_lib.qa_logmel_ragged(wav.data_ptr(), wlens, B, 1083, 640, 640, 320, 80, 16000, 0.0, 8000.0,
                                                               mel_out.data_ptr(), st),
        "qa_lm_generate_cond_ragged": lambda st: qa_lib.qa_lm_generate_cond_ragged(m.lm._handle, emb.data_ptr(), T, lens, B, G, S, 0.8, 50, 0.95,
                                                                                   gi.data_ptr(), si.data_ptr(), st),
        "qa_lm_score_cond_ragged": lambda st: qa_lib.qa_lm_score_cond_ragged(m.lm._handle, emb.data_ptr(), T, lens, B, gd.data_ptr(), G,
                                                                             sd_.data_ptr(), S, None, 0.1, ls.data_ptr(), co.data_ptr(),
                                                                             two.data_ptr(), two[1:].data_ptr(), st),
    }
    m.enable_taps(False)
    for name, call in calls.items():
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        graph = torch.cuda.CUDAGraph()
        with pytest.raises(qa.QuarkAudioError, match=name + ": refused under a stream capture"):
            with torch.cuda.graph(graph, stream=side):
                _lib.check(call(torch.cuda.current_stream(dev).cuda_stream))
        torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(mel_out).all() and bool((gi == -7).all()) and torch.isnan(ls).all()
    good()
