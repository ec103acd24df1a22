"""The kernels of csrc/bicodec_kernels.hip, each alone through its test hook (qa_debug_*, exported but not in the public header; the
waveform normalisation and the code statistics through the public entry points they already have), against the float64 restatements
of tests/bicodec_kernels_ref.py - at the shapes the kernels themselves branch on: the Res2 chain's time tile TT = 128 - 14 d and halo
7 d (T below the halo, at TT - 1 / TT / TT + 1, several tiles; widths that leave lanes idle), the SE gate's strided time mean (C from 4
to all 1024 threads), the four time slices of the ASTP / frame statistics (T below, at and above 4; C on both sides of the 64-lane
block), rows % 4 of the wave-per-row kernels, D on both sides of the 64-lane strides, the K padding columns, the second by-value chunk
of the ragged waveform lengths and the 64 KiB LDS boundary of the code histogram (K = 16336 / 16384).

Parity.  No tolerance is written down for any input: tol = max(2e-6, 4 x rel_err(the float32 CPU restatement, the float64 truth)) on
that same input (the rule and floor of tests/test_ew_kernels_gpu.py).  The kernel's own result never enters it.  Outputs sit between
sentinel guards (tests.util.guarded_out): nothing outside may change, everything inside is written and finite.  Bitwise (torch.equal):
two runs; a clip / row alone against the same clip inside a batch; row b of a per-clip call against the rectangular call on that clip
at its own length; everything a kernel must not touch; the pure moves against index arithmetic, add_rowvec against torch's fp32 add.
FSQ tokens: digit by digit against the float64 digits, a digit set aside only where the float64 `bounded` lies within m = 16 x
max|float32 restatement - float64| of a k + 0.5 boundary, and at most 0.2 % of the digits (the max_frac of the whole-model audit).
Refusals: bad shapes return a status without launching (the output keeps its NaNs).

What the cases were seen to catch (each change made to a scratch build, never committed; failing tests of this file on an MI355X): a halo
of 6 d in res2_chain_kernel 12 (every C at d = 1 .. 4; d = 9 has TT = 2 and survives alone); the rescale of s1 dropped from
astp_pool_kernel's new-maximum branch 10 (every C at T = 5 and 301, where a slice holds more than one frame); the SE time mean over T - 1
22; mel_frames reflecting about ref_len - 1/2 3; FSQ's basis advanced before the index update 60; adaln's rstd without eps 5 - by the
0 +- 1e-3 input with its constant row, which is here for that: at 0 +- 1 and 100 +- 0.5 an eps of 1e-6 moves the output by less than
the parity floor."""
import ctypes as C
import math

import pytest
import torch

from tests import bicodec_forward_ref as FR
from tests import bicodec_kernels_ref as K
from tests.test_bicodec_forward_gpu import PPL_TOL
from tests.util import check_guarded_out, guarded_out, rel_err, strided_rows

pytestmark = pytest.mark.gpu

HEAD = 64  # floats in front of every guarded output (keeps the 16-byte alignment of the float4 stores)
P, I, L, F = C.c_void_p, C.c_int, C.c_longlong, C.c_float
HOOKS = {
    "qa_debug_gather_rows": (I, [P, P, P, L, I, I, I, P, P]),
    "qa_debug_gather_global": (I, [P, P, P, I, I, I, I, P]),
    "qa_debug_tokens_fill_behind": (I, [P, I, I, P, P]),
    "qa_debug_zero_behind": (I, [P, I, L, P, I, P]),
    "qa_debug_adaln": (I, [P, P, P, L, P, I, I, I, F, P]),
    "qa_debug_add_rowvec": (I, [P, P, I, I, I, P]),
    "qa_debug_l2norm_rows": (I, [P, P, L, I, P]),
    "qa_debug_l2norm_scale": (I, [P, P, P, L, I, F, P]),
    "qa_debug_mel_frames": (I, [P, I, L, L, I, I, P, P, P]),
    "qa_debug_spec_mag": (I, [P, I, I, P, I, L, P]),
    "qa_debug_geglu": (I, [P, I, P, I, L, P]),
    "qa_debug_perceiver_ctx": (I, [P, L, P, P, I, I, I, I, P]),
    "qa_debug_res2_chain": (I, [P, P, P, P, I, I, I, I, P]),
    "qa_debug_se_residual": (I, [P, L, P, P, P, P, P, P, P, L, I, I, I, I, P]),
    "qa_debug_fsq": (I, [P, P, P, C.POINTER(C.c_int), I, I, L, P, P, P]),
    "qa_debug_astp_pool": (I, [P, P, I, I, I, P, P, P, P, P]),
    "qa_debug_frame_stats": (I, [P, I, I, I, P, P]),
    "qa_debug_widen_i32": (I, [P, P, L, P]),
}


@pytest.fixture(scope="module")
def hooks(qa_lib):
    for name, (res, args) in HOOKS.items():
        fn = getattr(qa_lib, name)
        fn.restype, fn.argtypes = res, args
    return qa_lib


def _p(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(dev, *ts):
    return [None if t is None else t.to(dev).contiguous() for t in ts]


def _lens(dev, lens):
    return None if lens is None else torch.tensor(lens, dtype=torch.int32, device=dev)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _finish(lib, status, buf, y, shape, head=HEAD, finite=True):
    """Status 0, guards intact, every element written and (unless the case itself defines a NaN) finite -> the output on the host."""
    assert status == 0, lib.qa_last_error()
    torch.cuda.synchronize()
    out = y.cpu().reshape(shape).clone()
    if finite:
        check_guarded_out(buf, y, head)
        assert torch.isfinite(out).all()
    else:  # NaN is a value here: only the guards are checked
        y.zero_()
        check_guarded_out(buf, y, head)
    return out


def _refused(lib, status, buf, y, head=HEAD):
    """A refusal: non-zero status with a message, and no launch - the output still holds its NaNs, the guards their sentinels."""
    torch.cuda.synchronize()
    assert status != 0 and lib.qa_last_error()
    assert torch.isnan(y).all()
    y.zero_()
    check_guarded_out(buf, y, head)


def _parity(what, y, ref, yard):
    """rel_err(kernel, truth) <= max(2e-6, 4 x rel_err(float32 restatement, truth)), all three on the same input."""
    err, floor = rel_err(y, ref), rel_err(yard, ref)
    tol = max(2e-6, 4.0 * floor)
    print(f"{what}: kernel {err:.3e} float32-cpu {floor:.3e} tol {tol:.3e}")
    assert err <= tol, f"{what}: rel err {err:.3e} > {tol:.3e} (float32 restatement on the same input: {floor:.3e})"


def _int_out(dev, n, words):
    """A guarded output of n integers of `words` 32-bit words each (guarded_out holds float32: the integers are read through a view)."""
    return guarded_out(n, words, words, HEAD, dev)


# ------------------------------------------------------------------------------------------------------------ res2_chain
def _res2(lib, dev, x, wt, bst, d, call=None):
    B, T, Cc = x.shape
    buf, y = guarded_out(B * T, Cc, Cc, HEAD, dev)
    xd, wd, bd = _dev(dev, x, wt, bst)
    st = lib.qa_debug_res2_chain(_p(xd), _p(y), _p(wd), _p(bd), B, T, Cc, d, _stream())
    return (buf, y, st) if call else _finish(lib, st, buf, y, (B, T, Cc))


def _res2_weights(W, g):
    wt = torch.randn(7, 3, W, W, generator=g) / (3 * W) ** 0.5
    bst = torch.stack((0.5 * torch.randn(7, W, generator=g), torch.randn(7, W, generator=g), torch.randn(7, W, generator=g)), 1)  # BN scales of both signs
    return wt, bst.contiguous()


@pytest.mark.parametrize("d", [1, 2, 3, 4, 9])
@pytest.mark.parametrize("Cc", [32, 256, 512])
def test_res2_chain(hooks, gpu_device, Cc, d):
    g = _gen(1000 + Cc + d)
    W, B, H, TT = Cc // 8, 2, 7 * d, 128 - 14 * d
    wt, bst = _res2_weights(W, g)
    assert float(bst[:, 1].min()) < 0 < float(bst[:, 1].max())
    clipped = total = 0
    for T in sorted({t for t in (1, H - 1, TT - 1, TT, TT + 1, 2 * TT + 3) if t >= 1}):
        x = torch.randn(B, T, Cc, generator=g)
        y = _res2(hooks, gpu_device, x, wt, bst, d)
        ref, yard = K.res2_chain_ref(x, wt, bst, d), K.res2_chain_ref(x, wt, bst, d, torch.float32)
        for i in range(7):
            s = slice(i * W, (i + 1) * W)
            _parity(f"res2_chain C {Cc} d {d} T {T} split {i}", y[..., s], ref[..., s], yard[..., s])
        assert torch.equal(y[..., 7 * W:], x[..., 7 * W:]), "the last split is not a bit-exact pass-through"
        hit = ref[..., :7 * W] == bst[:, 2].reshape(7 * W).double()  # ReLU gave 0: the output is the BN shift itself
        clipped, total = clipped + int(hit.sum()), total + hit.numel()
        assert torch.equal(y, _res2(hooks, gpu_device, x, wt, bst, d)), "two runs differ"
        for b in range(B):
            assert torch.equal(y[b:b + 1], _res2(hooks, gpu_device, x[b:b + 1], wt, bst, d)), f"T {T}: clip {b} alone differs from the clip in the batch"
    print(f"res2_chain C {Cc} d {d}: ReLU clips {clipped / total:.3f} of the outputs")
    assert 0.3 < clipped / total < 0.7, "the inputs do not exercise both sides of the ReLU"


@pytest.mark.parametrize("Cc,d", [(32, 10), (40, 1), (1024, 1)], ids=["d=10", "C=40", "C=1024"])
def test_res2_chain_refuses(hooks, gpu_device, Cc, d):
    W = Cc // 8
    buf, y, st = _res2(hooks, gpu_device, torch.randn(1, 3, Cc), torch.zeros(7, 3, W, W), torch.zeros(7, 3, W), d, call=True)
    _refused(hooks, st, buf, y)


# ------------------------------------------------------------------------------------------------------------ se_residual
def _se(lib, dev, x, y, w1t, b1, w2t, b2, ldx=None, call=None):
    """x rides at row stride ldx (default C + 4), out in the middle third of rows of 3 C floats: ([gate], [out]) guarded."""
    B, T, Cc = y.shape
    Hd = b1.numel()
    ldx = Cc + 4 if ldx is None else ldx
    gbuf, gate = guarded_out(B, Cc, Cc, HEAD, dev)
    obuf, out = guarded_out(B * T, Cc, 3 * Cc, HEAD + Cc, dev)
    xs = strided_rows(x.to(dev), ldx, ldx - Cc, generator=_gen(7))
    yd, w1, bb1, w2, bb2 = _dev(dev, y, w1t, b1, w2t, b2)
    st = lib.qa_debug_se_residual(xs.data_ptr(), ldx, _p(yd), _p(w1), _p(bb1), _p(w2), _p(bb2), _p(gate), _p(out), 3 * Cc, B, T, Cc, Hd,
                                  _stream())
    if call:
        return gbuf, gate, obuf, out, st
    return _finish(lib, st, gbuf, gate, (B, Cc)), _finish(lib, st, obuf, out, (B, T, Cc), HEAD + Cc)


@pytest.mark.parametrize("T", [1, 3, 301])
@pytest.mark.parametrize("Hd", [1, 128])
@pytest.mark.parametrize("Cc", [4, 64, 512, 1024])
def test_se_residual(hooks, gpu_device, Cc, Hd, T):
    g = _gen(2000 + Cc + Hd + T)
    B = 3
    x, y = torch.randn(B, T, Cc, generator=g), 0.5 + torch.randn(B, T, Cc, generator=g)
    w = (torch.randn(Cc, Hd, generator=g) / Cc ** 0.5, torch.randn(Hd, generator=g), torch.randn(Hd, Cc, generator=g) / Hd ** 0.5,
         torch.randn(Cc, generator=g))
    gate, out = _se(hooks, gpu_device, x, y, *w)
    (gr, orf), (gy, oy) = K.se_residual_ref(x, y, *w), K.se_residual_ref(x, y, *w, dtype=torch.float32)
    _parity(f"se_residual C {Cc} Hd {Hd} T {T} gate", gate, gr, gy)
    _parity(f"se_residual C {Cc} Hd {Hd} T {T} out", out, orf, oy)
    g2, o2 = _se(hooks, gpu_device, x, y, *w)
    assert torch.equal(gate, g2) and torch.equal(out, o2), "two runs differ"
    for b in (0, B - 1):
        g1, o1 = _se(hooks, gpu_device, x[b:b + 1], y[b:b + 1], *w)
        assert torch.equal(gate[b:b + 1], g1) and torch.equal(out[b:b + 1], o1), f"clip {b} alone differs from the clip in the batch"


@pytest.mark.parametrize("Cc,ldx", [(48, None), (2048, None), (64, 66)], ids=["C=48", "C=2048", "ldx=C+2"])
def test_se_residual_refuses(hooks, gpu_device, Cc, ldx):
    z = torch.zeros(1, 2, Cc)
    gbuf, gate, obuf, out, st = _se(hooks, gpu_device, z, z, torch.zeros(Cc, 8), torch.zeros(8), torch.zeros(8, Cc), torch.zeros(Cc), ldx,
                                    call=True)
    _refused(hooks, st, gbuf, gate)
    _refused(hooks, st, obuf, out, HEAD + Cc)


# ------------------------------------------------------------------------------------------------------------ astp_pool / frame_stats
def _astp(lib, dev, logit, x, bn_s, bn_t, call=None, shape=None):
    B, T, Cc = shape or x.shape
    pbuf, pool = guarded_out(max(B, 1), 2 * Cc, 2 * Cc, HEAD, dev)
    bbuf, bn = guarded_out(max(B, 1), 2 * Cc, 2 * Cc, HEAD, dev)
    ld, xd, sd, td = _dev(dev, logit, x, bn_s, bn_t)
    st = lib.qa_debug_astp_pool(_p(ld), _p(xd), B, T, Cc, _p(sd), _p(td), _p(pool), _p(bn), _stream())
    if call:
        return pbuf, pool, bbuf, bn, st
    return _finish(lib, st, pbuf, pool, (B, 2 * Cc)), _finish(lib, st, bbuf, bn, (B, 2 * Cc))


ASTP_C = [1, 63, 64, 65, 130]


@pytest.mark.parametrize("T", [1, 2, 3, 4, 5, 301])
@pytest.mark.parametrize("Cc", ASTP_C)
def test_astp_pool(hooks, gpu_device, Cc, T):
    g = _gen(3000 + Cc + T)
    B = 2
    bn_s, bn_t = torch.randn(2 * Cc, generator=g), torch.randn(2 * Cc, generator=g)
    ramp = torch.cumsum(0.1 + torch.rand(B, T, Cc, generator=g), 1)  # strictly ascending in time: every frame is a new maximum
    logits = {"10 randn": 10.0 * torch.randn(B, T, Cc, generator=g), "ascending": ramp, "descending": -ramp}
    xs = {"0/1": torch.randn(B, T, Cc, generator=g), "100/0.5": 100.0 + 0.5 * torch.randn(B, T, Cc, generator=g),
          "constant": torch.randn(B, 1, Cc, generator=g).expand(B, T, Cc).contiguous()}
    for ln, logit in logits.items():
        for xn, x in xs.items():
            what = f"astp_pool C {Cc} T {T} logits {ln} x {xn}"
            pool, bn = _astp(hooks, gpu_device, logit, x, bn_s, bn_t)
            (pr, br), (py, by) = K.astp_pool_ref(logit, x, bn_s, bn_t), K.astp_pool_ref(logit, x, bn_s, bn_t, torch.float32)
            _parity(what + " mean", pool[:, :Cc], pr[:, :Cc], py[:, :Cc])
            _parity(what + " std", pool[:, Cc:], pr[:, Cc:], py[:, Cc:])
            _parity(what + " bn", bn, br, by)
            if xn == "constant" or T == 1:  # no variance: the clamp at 1e-7, whatever the float32 restatement makes of the cancellation
                assert rel_err(pool[:, Cc:], torch.full((B, Cc), 1e-7 ** 0.5)) <= 2e-6, what
    p2, b2 = _astp(hooks, gpu_device, logit, x, bn_s, bn_t)
    assert torch.equal(pool, p2) and torch.equal(bn, b2), "two runs differ"
    p1, b1 = _astp(hooks, gpu_device, logit[1:], x[1:], bn_s, bn_t)
    assert torch.equal(pool[1:], p1) and torch.equal(bn[1:], b1), "item 1 alone differs from the item in the batch"


@pytest.mark.parametrize("B,T", [(2, 0), (0, 3)], ids=["T=0", "B=0"])
def test_astp_pool_refuses(hooks, gpu_device, B, T):
    z = torch.zeros(2, 3, 8)
    pbuf, pool, bbuf, bn, st = _astp(hooks, gpu_device, z, z, torch.ones(16), torch.zeros(16), call=True, shape=(B, T, 8))
    _refused(hooks, st, pbuf, pool)
    _refused(hooks, st, bbuf, bn)


def _frame_stats(lib, dev, x, finite=True):
    B, T, Cc = x.shape
    buf, ctx = guarded_out(B, 2 * Cc, 2 * Cc, HEAD, dev)
    (xd,) = _dev(dev, x)
    st = lib.qa_debug_frame_stats(_p(xd), B, T, Cc, _p(ctx), _stream())
    return _finish(lib, st, buf, ctx, (B, 2 * Cc), finite=finite)


@pytest.mark.parametrize("T", [1, 2, 4, 5, 301])
@pytest.mark.parametrize("Cc", ASTP_C)
def test_frame_stats(hooks, gpu_device, Cc, T):
    g = _gen(3500 + Cc + T)
    B = 2
    for dist, x in (("0/1", torch.randn(B, T, Cc, generator=g)), ("100/0.5", 100.0 + 0.5 * torch.randn(B, T, Cc, generator=g))):
        ctx = _frame_stats(hooks, gpu_device, x, finite=T > 1)
        ref, yard = K.frame_stats_ref(x), K.frame_stats_ref(x, torch.float32)
        _parity(f"frame_stats C {Cc} T {T} {dist} mean", ctx[:, :Cc], ref[:, :Cc], yard[:, :Cc])
        if T == 1:  # torch.var of one frame
            assert torch.isfinite(ctx[:, :Cc]).all() and torch.isnan(ctx[:, Cc:]).all() and torch.isnan(ref[:, Cc:]).all()
        else:
            _parity(f"frame_stats C {Cc} T {T} {dist} std", ctx[:, Cc:], ref[:, Cc:], yard[:, Cc:])
        again, alone = _frame_stats(hooks, gpu_device, x, finite=T > 1), _frame_stats(hooks, gpu_device, x[1:], finite=T > 1)
        assert torch.equal(ctx[:, :Cc], again[:, :Cc]) and torch.equal(ctx[1:, :Cc], alone[:, :Cc])
        if T > 1:
            assert torch.equal(ctx, again), "two runs differ"
            assert torch.equal(ctx[1:], alone), "item 1 alone differs from the item in the batch"


# ------------------------------------------------------------------------------------------------------------ fsq
def _fsq(lib, dev, x, w, bias, levels, tap=True, call=None):
    rows, D = x.shape
    nl = len(levels)
    tbuf, tok = _int_out(dev, rows, 1)
    bbuf, bounded = guarded_out(rows, max(nl, 1), max(nl, 1), HEAD, dev)
    xd, wd, bd = _dev(dev, x, w, bias)
    lv = (C.c_int * max(nl, 1))(*levels)
    st = lib.qa_debug_fsq(_p(xd), _p(wd), _p(bd), lv, nl, D, rows, _p(tok), _p(bounded) if tap else None, _stream())
    if call:
        return tbuf, tok, bbuf, bounded, st
    assert st == 0, lib.qa_last_error()
    torch.cuda.synchronize()
    tokens = tok.view(torch.int32).cpu().reshape(rows).long()
    tok.zero_()  # integers are not floats: only the guards of the token buffer are checked
    check_guarded_out(tbuf, tok, HEAD)
    if not tap:
        assert torch.isnan(bounded).all(), "the bounded tap was written without being asked for"
        return tokens, None
    return tokens, _finish(lib, st, bbuf, bounded, (rows, nl))


FSQ_LEVELS = [[4] * 6, [8, 5, 5, 5], [2], [3] * 8]
FSQ_MAX_FRAC = 0.002  # the max_frac of the whole-model audit (_audit_fsq)


@pytest.mark.parametrize("rows", [1, 5, 1031])
@pytest.mark.parametrize("D", [1, 37, 64, 128, 256])
@pytest.mark.parametrize("levels", FSQ_LEVELS, ids=["4x6", "8555", "2", "3x8"])
def test_fsq(hooks, gpu_device, levels, D, rows):
    """For an even L `bounded` is a difference of two values near 0.5 - with L = 2, tanh(z + atanh(0.999)) * 0.5005 - 0.5 = 4e-4 - so a float32
    evaluation is off by 2e-5 .. 7e-5 of the result (half an ulp of that 0.5, and of the constants), and with rows = 1 the float32
    restatement's error is one draw: the kernel evaluates the bound in double (profiles/fsq_bound_double.md)."""
    g = _gen(4000 + 7 * D + rows + len(levels))
    nl = len(levels)
    x, w, bias = torch.randn(rows, D, generator=g), torch.randn(nl, D, generator=g) / D ** 0.5, 0.1 * torch.randn(nl, generator=g)
    b64, d64, t64 = K.fsq_ref(x, w, bias, levels)
    b32, _, _ = K.fsq_ref(x, w, bias, levels, torch.float32)
    m = 16.0 * float((b32.double() - b64).abs().max())
    near = (b64 - (torch.floor(b64) + 0.5)).abs() <= m  # the float64 decision itself sits on a rounding boundary
    frac = float(near.double().mean())
    print(f"fsq levels {levels} D {D} rows {rows}: m {m:.3e}, {int(near.sum())} of {near.numel()} digits set aside")
    assert frac <= FSQ_MAX_FRAC, f"{frac:.4f} of the digits sit within {m:.3e} of a boundary: the case cannot judge the tokens"
    tokens, bounded = _fsq(hooks, gpu_device, x, w, bias, levels)
    _parity(f"fsq levels {levels} D {D} rows {rows} bounded", bounded, b64, b32)
    assert int(tokens.min()) >= 0 and int(tokens.max()) < math.prod(levels)
    digits = K.fsq_digits_of(tokens, levels)
    wrong = (digits != d64) & ~near
    assert int(wrong.sum()) == 0, f"{int(wrong.sum())} digits differ from the float64 digits away from a rounding boundary"
    assert torch.equal(tokens[~near.any(1)], t64[~near.any(1)])
    assert torch.equal(tokens, _fsq(hooks, gpu_device, x, w, bias, levels, tap=False)[0]), "the tokens depend on the bounded tap"
    assert torch.equal(tokens, _fsq(hooks, gpu_device, x, w, bias, levels)[0]), "two runs differ"


@pytest.mark.parametrize("nl", [0, 9])
def test_fsq_refuses(hooks, gpu_device, nl):
    tbuf, tok, bbuf, bounded, st = _fsq(hooks, gpu_device, torch.randn(3, 8), torch.randn(max(nl, 1), 8), torch.zeros(max(nl, 1)), [3] * nl,
                                        call=True)
    _refused(hooks, st, tbuf, tok)
    _refused(hooks, st, bbuf, bounded)


# ------------------------------------------------------------------------------------------------------------ adaln / add_rowvec
def _adaln(lib, dev, x, cond, ld_cond, eps, call=None):
    """scale = cond[:, :C], shift = cond[:, C:2C] of conditioning rows of ld_cond floats, as vocos passes them."""
    B, T, Cc = x.shape
    buf, y = guarded_out(B * T, Cc, Cc, HEAD, dev)
    xd, cd = _dev(dev, x, cond)
    st = lib.qa_debug_adaln(_p(xd), cd.data_ptr(), cd.data_ptr() + 4 * Cc, ld_cond, _p(y), B, T, Cc, eps, _stream())
    return (buf, y, st) if call else _finish(lib, st, buf, y, (B, T, Cc))


@pytest.mark.parametrize("Cc", [4, 252, 256, 260, 1024])
def test_adaln(hooks, gpu_device, Cc):
    g = _gen(5000 + Cc)
    B, T, eps = 3, 5, 1e-6
    ld = 2 * Cc + 4
    cond = torch.randn(B, ld, generator=g)
    flat = 1e-3 * torch.randn(B, T, Cc, generator=g)  # variance ~ eps: the eps under the root counts
    flat[1, 2] = 0.25                                  # a constant row: rstd = eps^-1/2, the output is the shift
    for dist, x in (("0/1", torch.randn(B, T, Cc, generator=g)), ("100/0.5", 100.0 + 0.5 * torch.randn(B, T, Cc, generator=g)),
                    ("0/1e-3", flat)):
        y = _adaln(hooks, gpu_device, x, cond, ld, eps)
        args = (cond[:, :Cc], cond[:, Cc:2 * Cc], eps)
        _parity(f"adaln C {Cc} {dist}", y, K.adaln_ref(x, *args), K.adaln_ref(x, *args, dtype=torch.float32))
        assert torch.equal(y, _adaln(hooks, gpu_device, x, cond, ld, eps)), "two runs differ"
        for b, t in ((0, 0), (1, 2), (B - 1, T - 1)):
            alone = _adaln(hooks, gpu_device, x[b:b + 1, t:t + 1], cond[b:b + 1], ld, eps)
            assert torch.equal(y[b:b + 1, t:t + 1], alone), f"row ({b}, {t}) alone differs from the row in the batch"
    assert torch.equal(y[1, 2], cond[1, Cc:2 * Cc]), "a constant row is not exactly the shift"


@pytest.mark.parametrize("Cc,ld", [(6, 16), (8, 18)], ids=["C=6", "ld=2C+2"])
def test_adaln_refuses(hooks, gpu_device, Cc, ld):
    buf, y, st = _adaln(hooks, gpu_device, torch.randn(1, 2, Cc), torch.randn(1, ld), ld, 1e-6, call=True)
    _refused(hooks, st, buf, y)


@pytest.mark.parametrize("Cc", [4, 260])
def test_add_rowvec(hooks, gpu_device, Cc):
    g = _gen(5500 + Cc)
    B, T = 3, 5
    x, v = torch.randn(B, T, Cc, generator=g), torch.randn(B, Cc, generator=g)
    buf, y = guarded_out(B * T, Cc, Cc, HEAD, gpu_device)
    y.copy_(x.reshape(B * T, Cc))
    (vd,) = _dev(gpu_device, v)
    out = _finish(hooks, hooks.qa_debug_add_rowvec(_p(y), _p(vd), B, T, Cc, _stream()), buf, y, (B, T, Cc))
    assert torch.equal(out, x + v[:, None]), "one rounded fp32 add per element"
    buf, y = guarded_out(2, 6, 6, HEAD, gpu_device)
    _refused(hooks, hooks.qa_debug_add_rowvec(_p(y), _p(vd), 1, 2, 6, _stream()), buf, y)


# ------------------------------------------------------------------------------------------------------------ l2norm_rows / l2norm_scale
def _l2norm(lib, dev, x, gamma=None, scale=1.0, call=None, D=None):
    rows, width = x.shape
    D = width if D is None else D
    buf, y = guarded_out(rows, width, width, HEAD, dev)
    xd, gd = _dev(dev, x, gamma)
    if gamma is None:
        st = lib.qa_debug_l2norm_rows(_p(xd), _p(y), rows, D, _stream())
    else:
        st = lib.qa_debug_l2norm_scale(_p(xd), _p(gd), _p(y), rows, D, scale, _stream())
    return (buf, y, st) if call else _finish(lib, st, buf, y, (rows, D))


def _l2norm_case(lib, dev, what, D, rows, with_gamma):
    g = _gen(6000 + D + rows)
    x = torch.randn(rows, D, generator=g)
    x[rows // 2] = 0.0  # an all-zero row: 0 / max(0, 1e-12) = 0
    gamma, scale = (torch.randn(D, generator=g), D ** 0.5) if with_gamma else (None, 1.0)
    y = _l2norm(lib, dev, x, gamma, scale)
    if with_gamma:
        ref, yard = K.l2norm_scale_ref(x, gamma, scale), K.l2norm_scale_ref(x, gamma, scale, torch.float32)
    else:
        ref, yard = K.l2norm_rows_ref(x), K.l2norm_rows_ref(x, torch.float32)
    if rows > 1:
        _parity(f"{what} D {D} rows {rows}", y, ref, yard)
    assert torch.equal(y[rows // 2], torch.zeros(D)), "an all-zero row does not give zeros"
    assert torch.equal(y, _l2norm(lib, dev, x, gamma, scale)), "two runs differ"
    x[rows // 2] = torch.randn(D, generator=g)
    y = _l2norm(lib, dev, x, gamma, scale)
    ref, yard = ((K.l2norm_scale_ref(x, gamma, scale), K.l2norm_scale_ref(x, gamma, scale, torch.float32)) if with_gamma else
                 (K.l2norm_rows_ref(x), K.l2norm_rows_ref(x, torch.float32)))
    _parity(f"{what} D {D} rows {rows} (no zero row)", y, ref, yard)
    for r in {0, rows - 1}:
        assert torch.equal(y[r:r + 1], _l2norm(lib, dev, x[r:r + 1], gamma, scale)), f"row {r} alone differs from the row in the batch"


@pytest.mark.parametrize("rows", [1, 5, 130])
@pytest.mark.parametrize("D", [1, 8, 63, 64])
def test_l2norm_rows(hooks, gpu_device, D, rows):
    _l2norm_case(hooks, gpu_device, "l2norm_rows", D, rows, False)


@pytest.mark.parametrize("rows", [1, 5, 130])
@pytest.mark.parametrize("D", [1, 64, 65, 128, 255, 256])
def test_l2norm_scale(hooks, gpu_device, D, rows):
    _l2norm_case(hooks, gpu_device, "l2norm_scale", D, rows, True)


@pytest.mark.parametrize("D,with_gamma", [(0, False), (65, False), (257, True)], ids=["rows D=0", "rows D=65", "scale D=257"])
def test_l2norm_refuses(hooks, gpu_device, D, with_gamma):
    buf, y, st = _l2norm(hooks, gpu_device, torch.randn(2, max(D, 1)), torch.ones(max(D, 1)) if with_gamma else None, 1.0, call=True, D=D)
    _refused(hooks, st, buf, y)


# ------------------------------------------------------------------------------------------------------------ geglu / spec_mag
@pytest.mark.parametrize("rows", [1, 33])
@pytest.mark.parametrize("Fh,ldo", [(341, 344), (4, 4), (1, 4)])
def test_geglu(hooks, gpu_device, Fh, ldo, rows):
    g = _gen(7000 + Fh + rows)
    h = torch.randn(rows, 2 * Fh, generator=g)
    h[:, Fh:] = 12.0 * torch.rand(rows, Fh, generator=g) - 6.0  # the gate, out to +-6
    h[0, Fh], h[-1, 2 * Fh - 1] = 6.0, -6.0
    outs = []
    for _ in range(2):
        buf, y = guarded_out(rows, ldo, ldo, HEAD, gpu_device)
        (hd,) = _dev(gpu_device, h)
        outs.append(_finish(hooks, hooks.qa_debug_geglu(_p(hd), Fh, _p(y), ldo, rows, _stream()), buf, y, (rows, ldo)))
    y = outs[0]
    _parity(f"geglu F {Fh} ldo {ldo} rows {rows}", y[:, :Fh], K.geglu_ref(h, Fh, ldo)[:, :Fh], K.geglu_ref(h, Fh, ldo, torch.float32)[:, :Fh])
    assert torch.equal(y[:, Fh:], torch.zeros(rows, ldo - Fh)), "padding columns are not exactly 0"
    assert torch.equal(y, outs[1]), "two runs differ"


@pytest.mark.parametrize("rows", [3, 65])
@pytest.mark.parametrize("nbp,nb,ldm", [(8, 5, 8), (12, 9, 16), (520, 513, 520)])
def test_spec_mag(hooks, gpu_device, nbp, nb, ldm, rows):
    g = _gen(7500 + nb + rows)
    ri = torch.full((rows, 2 * nbp), float("nan"))  # the padding bins of the DFT rows are never read
    ri[:, :nb], ri[:, nbp:nbp + nb] = torch.randn(rows, nb, generator=g), torch.randn(rows, nb, generator=g)
    ri[0, 0] = ri[0, nbp] = 0.0
    outs = []
    for _ in range(2):
        buf, y = guarded_out(rows, ldm, ldm, HEAD, gpu_device)
        (rd,) = _dev(gpu_device, ri)
        outs.append(_finish(hooks, hooks.qa_debug_spec_mag(_p(rd), nbp, nb, _p(y), ldm, rows, _stream()), buf, y, (rows, ldm)))
    y = outs[0]
    _parity(f"spec_mag nbp {nbp} nb {nb} ldm {ldm} rows {rows}", y[:, :nb], K.spec_mag_ref(ri, nbp, nb, ldm)[:, :nb],
            K.spec_mag_ref(ri, nbp, nb, ldm, torch.float32)[:, :nb])
    assert torch.equal(y[:, nb:], torch.zeros(rows, ldm - nb)), "padding columns are not exactly 0"
    assert float(y[0, 0]) == 0.0 and torch.equal(y, outs[1])


# ------------------------------------------------------------------------------------------------------------ mel_frames
def _mel_frames(lib, dev, wav, ref_len, hop, lens=None, call=None):
    B, T = wav.shape
    nf = ref_len // hop + 1
    n_out = (nf + 1) * hop
    buf, Pm = guarded_out(B, n_out, n_out, HEAD, dev)
    (wd,) = _dev(dev, wav)
    ld = _lens(dev, lens)
    st = lib.qa_debug_mel_frames(_p(wd), B, T, ref_len, hop, nf, _p(Pm), _p(ld), _stream())
    return (buf, Pm, st) if call else _finish(lib, st, buf, Pm, (B, n_out))


@pytest.mark.parametrize("ref_len", [9, 61, 64])
def test_mel_frames(hooks, gpu_device, ref_len):
    g = _gen(8000 + ref_len)
    hop, B = 8, 3
    nf = ref_len // hop + 1
    for T in sorted({t for t in (1, ref_len - 3, ref_len, ref_len + 5) if t >= 1}):  # the clip tiles (T < ref_len) or is cut
        wav = torch.randn(B, T, generator=g)
        Pm = _mel_frames(hooks, gpu_device, wav, ref_len, hop)
        assert torch.equal(Pm, K.mel_frames_ref(wav, ref_len, hop, nf)), f"T {T}: not the reflect-padded reference clip"
        assert torch.equal(Pm, _mel_frames(hooks, gpu_device, wav, ref_len, hop))
        assert torch.equal(Pm[1:2], _mel_frames(hooks, gpu_device, wav[1:2], ref_len, hop)), "row 1 alone differs"
        lens = [T, max(T // 2, 1), 1]
        rag = wav.clone()
        for b, n in enumerate(lens):
            rag[b, n:] = float("nan")  # a NaN in the output proves a read behind the clip's end (_finish: all finite)
        Pr = _mel_frames(hooks, gpu_device, rag, ref_len, hop, lens)
        assert torch.equal(Pr, K.mel_frames_ref(wav, ref_len, hop, nf, lens)), f"T {T} lens {lens}: a row does not tile by its own length"
        for b, n in enumerate(lens):
            assert torch.equal(Pr[b:b + 1], _mel_frames(hooks, gpu_device, wav[b:b + 1, :n], ref_len, hop)), f"clip {b} alone at T = {n} differs"


def test_mel_frames_refuses(hooks, gpu_device):
    hop = 8
    n_out = (hop // hop + 2) * hop
    buf, Pm = guarded_out(1, n_out, n_out, HEAD, gpu_device)
    (wd,) = _dev(gpu_device, torch.randn(1, 20))
    _refused(hooks, hooks.qa_debug_mel_frames(_p(wd), 1, 20, hop, hop, hop // hop + 1, _p(Pm), None, _stream()), buf, Pm)


# ------------------------------------------------------------------------------------------------------------ gathers, tails, moves
def _gather_rows(lib, dev, tok, table, T=0, lens=None, call=None):
    n, (V, D) = tok.numel(), table.shape
    buf, y = guarded_out(n, D, D, HEAD, dev)
    td, tb = _dev(dev, tok.reshape(-1), table)
    ld = _lens(dev, lens)
    st = lib.qa_debug_gather_rows(_p(td), _p(tb), _p(y), n, V, D, T, _p(ld), _stream())
    return (buf, y, st) if call else _finish(lib, st, buf, y, (n, D))


@pytest.mark.parametrize("D", [4, 8])
def test_gather_rows(hooks, gpu_device, D):
    g = _gen(9000 + D)
    V, B, T = 5, 3, 7
    table = torch.randn(V, D, generator=g)
    tok = torch.randint(0, V, (B, T), generator=g)
    tok[0, 1], tok[0, 4], tok[1, 0] = -3, V + 2, V  # the clamp: rows 0 and V - 1
    y = _gather_rows(hooks, gpu_device, tok, table)
    assert torch.equal(y, K.gather_rows_ref(tok.reshape(-1), table))
    assert torch.equal(y[1], table[0]) and torch.equal(y[4], table[V - 1]) and torch.equal(y[T], table[V - 1])
    lens = [7, 3, 1]
    wild = tok.clone()
    for b, n in enumerate(lens):
        wild[b, n:] = 2 ** 40  # behind a clip's length the tokens are never loaded, let alone used as an index
    rag = _gather_rows(hooks, gpu_device, wild, table, T, lens)
    assert torch.equal(rag, K.gather_rows_ref(tok.reshape(-1), table, T, lens))
    for b, n in enumerate(lens):
        rows = rag.reshape(B, T, D)[b]
        assert torch.equal(rows[n:], torch.zeros(T - n, D)), f"clip {b}: rows behind its length are not exact zeros"
        assert torch.equal(rows[:n], _gather_rows(hooks, gpu_device, tok[b, :n], table)), f"clip {b}: rows before its length differ"


def test_gather_rows_refuses(hooks, gpu_device):
    tok = torch.zeros(20, dtype=torch.int64)
    buf, y, st = _gather_rows(hooks, gpu_device, tok, torch.randn(5, 6), call=True)
    _refused(hooks, st, buf, y)
    buf, y, st = _gather_rows(hooks, gpu_device, tok, torch.randn(5, 8), 7, [7, 7, 6], call=True)  # 20 rows are not B * 7
    _refused(hooks, st, buf, y)


def test_gather_global(hooks, gpu_device):
    g = _gen(9100)
    B, N, V, Ld = 3, 4, 6, 5
    table = torch.randn(V, Ld, generator=g)
    tok = torch.randint(0, V, (B, N), generator=g)
    tok[0, 0], tok[2, 3] = -1, V + 7
    buf, y = guarded_out(B, N * Ld, N * Ld, HEAD, gpu_device)
    td, tb = _dev(gpu_device, tok, table)
    out = _finish(hooks, hooks.qa_debug_gather_global(_p(td), _p(tb), _p(y), B, N, V, Ld, _stream()), buf, y, (B, N * Ld))
    assert torch.equal(out, K.gather_global_ref(tok, table)), "not out[b, c * N + n] = table[clamp(tok[b, n]), c]"
    assert out[0, 0] == table[0, 0] and out[2, 4 * N + 3] == table[V - 1, 4] and out[1, 2 * N + 1] == table[tok[1, 1], 2]


def test_tails_of_a_per_clip_call(hooks, gpu_device):
    g = _gen(9200)
    B, N, T, mul, lens = 3, 300, 1000, 320, [3, 1, 0]
    ld = _lens(gpu_device, lens)
    tok = torch.randint(0, 8192, (B, N), generator=g)
    tbuf, ty = _int_out(gpu_device, B * N, 2)
    ty.view(torch.int64).copy_(tok.reshape(-1, 1))
    assert hooks.qa_debug_tokens_fill_behind(_p(ty), B, N, _p(ld), _stream()) == 0, hooks.qa_last_error()
    torch.cuda.synchronize()
    got = ty.view(torch.int64).cpu().reshape(B, N).clone()
    assert torch.equal(got, K.tokens_fill_behind_ref(tok, lens))
    assert all(torch.equal(got[b, :n], tok[b, :n]) and bool((got[b, n:] == -1).all()) for b, n in enumerate(lens))
    ty.zero_()
    check_guarded_out(tbuf, ty, HEAD)
    x = torch.randn(B, T, generator=g)
    xbuf, xy = guarded_out(B, T, T, HEAD, gpu_device)
    xy.copy_(x)
    out = _finish(hooks, hooks.qa_debug_zero_behind(_p(xy), B, T, _p(ld), mul, _stream()), xbuf, xy, (B, T))
    assert torch.equal(out, K.zero_behind_ref(x, lens, mul))
    assert all(torch.equal(out[b, :n * mul], x[b, :n * mul]) and bool((out[b, n * mul:] == 0).all()) for b, n in enumerate(lens))
    # without lengths there is nothing to do: a refusal, and every bit stays
    xy.copy_(x)
    assert hooks.qa_debug_zero_behind(_p(xy), B, T, None, mul, _stream()) != 0 and hooks.qa_last_error()
    ty.view(torch.int64).copy_(tok.reshape(-1, 1))
    assert hooks.qa_debug_tokens_fill_behind(_p(ty), B, N, None, _stream()) != 0 and hooks.qa_last_error()
    torch.cuda.synchronize()
    assert torch.equal(xy.cpu(), x) and torch.equal(ty.view(torch.int64).cpu().reshape(B, N), tok)


def test_perceiver_ctx(hooks, gpu_device):
    """The three call forms of csrc/bicodec.cpp."""
    g = _gen(9300)
    B, n_lat, T, D = 3, 5, 7, 12
    learned, per_item = torch.randn(n_lat, D, generator=g), torch.randn(B, n_lat, D, generator=g)
    x = torch.randn(B, T, D, generator=g)
    ld, pd, xd = _dev(gpu_device, learned, per_item, x)
    buf, ctx = guarded_out(B * (n_lat + T), D, D, HEAD, gpu_device)  # learned latents (batch stride 0) with x: cat(latents, x)
    first = _finish(hooks, hooks.qa_debug_perceiver_ctx(_p(ld), 0, _p(xd), _p(ctx), B, n_lat, T, D, _stream()), buf, ctx, (B, n_lat + T, D))
    assert torch.equal(first, torch.cat((learned.expand(B, -1, -1), x), 1))
    # per-item latents, x = null, T > 0: only the latent rows of the same buffer change
    assert hooks.qa_debug_perceiver_ctx(_p(pd), n_lat * D, None, _p(ctx), B, n_lat, T, D, _stream()) == 0, hooks.qa_last_error()
    third = _finish(hooks, 0, buf, ctx, (B, n_lat + T, D))
    assert torch.equal(third, K.perceiver_ctx_ref(first, per_item, None, T)) and torch.equal(third[:, n_lat:], x)
    buf, lat = guarded_out(B * n_lat, D, D, HEAD, gpu_device)  # learned latents, x = null, T = 0: the broadcast alone
    second = _finish(hooks, hooks.qa_debug_perceiver_ctx(_p(ld), 0, None, _p(lat), B, n_lat, 0, D, _stream()), buf, lat, (B, n_lat, D))
    assert torch.equal(second, learned.expand(B, -1, -1))


@pytest.mark.parametrize("n", [1, 257, 1000])
def test_widen_i32(hooks, gpu_device, n):
    src = torch.randint(-2 ** 31, 2 ** 31 - 1, (n,), generator=_gen(9400 + n), dtype=torch.int64).to(torch.int32)
    src[0] = -1
    buf, y = _int_out(gpu_device, n, 2)
    (sd,) = _dev(gpu_device, src)
    assert hooks.qa_debug_widen_i32(_p(sd), _p(y), n, _stream()) == 0, hooks.qa_last_error()
    torch.cuda.synchronize()
    assert torch.equal(y.view(torch.int64).cpu().reshape(n), src.long()), "not a sign-extending copy"
    y.zero_()
    check_guarded_out(buf, y, HEAD)


# ------------------------------------------------------------------------------------------------------------ wav_normalize (public)
def _wav_normalize(lib, dev, wav, eps, lens=None):
    B, T = wav.shape
    buf, y = guarded_out(B, T, T, HEAD, dev)
    (wd,) = _dev(dev, wav)
    if lens is None:
        st = lib.qa_wav_normalize(_p(wd), B, T, _p(y), eps, _stream())
    else:
        st = lib.qa_wav_normalize_ragged(_p(wd), B, T, (C.c_int64 * B)(*lens), _p(y), eps, _stream())
    return _finish(lib, st, buf, y, (B, T))


@pytest.mark.parametrize("T", [1, 255, 256, 257, 16000])
def test_wav_normalize(qa_lib, gpu_device, T):
    g = _gen(9500 + T)
    wav, eps = 0.3 + 0.01 * torch.randn(2, T, generator=g), 1e-7
    y = _wav_normalize(qa_lib, gpu_device, wav, eps)
    if T == 1:
        assert torch.equal(y, torch.zeros(2, 1))  # (x - x) / sqrt(0 + eps)
    else:
        _parity(f"wav_normalize T {T}", y, K.wav_normalize_ref(wav, eps), K.wav_normalize_ref(wav, eps, dtype=torch.float32))
    assert torch.equal(y, _wav_normalize(qa_lib, gpu_device, wav, eps)), "two runs differ"
    assert torch.equal(y[1:], _wav_normalize(qa_lib, gpu_device, wav[1:], eps)), "row 1 alone differs"


def test_wav_normalize_ragged_second_chunk(qa_lib, gpu_device):
    """B = 257: the lengths of row 256 travel in the second by-value chunk of the launch."""
    g = _gen(9600)
    B, T, eps = 257, 300, 1e-7
    wav = 0.3 + 0.01 * torch.randn(B, T, generator=g)
    lens = torch.randint(2, T + 1, (B,), generator=g).tolist()
    lens[0], lens[1], lens[255], lens[256] = T, 2, 255, 257
    rag = wav.clone()
    for b, n in enumerate(lens):
        rag[b, n:] = float("nan")  # nothing behind a clip's length is read
    y = _wav_normalize(qa_lib, gpu_device, rag, eps, lens)
    _parity("wav_normalize ragged [257, 300]", y, K.wav_normalize_ref(wav, eps, lens), K.wav_normalize_ref(wav, eps, lens, torch.float32))
    assert torch.equal(y, _wav_normalize(qa_lib, gpu_device, rag, eps, lens)), "two runs differ"
    for b, n in enumerate(lens):
        assert torch.equal(y[b, n:], torch.zeros(T - n)), f"row {b}: samples behind its length are not exactly 0"
    for b in (0, 1, 2, 128, 255, 256):
        alone = _wav_normalize(qa_lib, gpu_device, wav[b:b + 1, :lens[b]], eps)
        assert torch.equal(y[b:b + 1, :lens[b]], alone), f"row {b} of the ragged call differs from the clip alone at T = {lens[b]}"


# ------------------------------------------------------------------------------------------------------------ code_usage (public)
def _code_usage(lib, dev, idx, Kc, n=None):
    buf, out = guarded_out(1, 2, 2, HEAD, dev)
    (idd,) = _dev(dev, idx)
    st = lib.qa_code_usage(_p(idd), idx.numel() if n is None else n, Kc, out[0, 0:1].data_ptr(), out[0, 1:2].data_ptr(), _stream())
    return buf, out, st


@pytest.mark.parametrize("n", [1, 1023, 1025, 5000])
@pytest.mark.parametrize("Kc", [1, 1000, 1024, 1025, 16336, 16384])
def test_code_usage(qa_lib, gpu_device, Kc, n):
    """K = 16336 is the last codebook whose histogram fits beside the kernel's static LDS in 64 KiB; K = 16384 (65,728 bytes) needs the
    raised dynamic limit."""
    g = _gen(9700 + Kc + n)
    clean = torch.randint(0, Kc, (n,), generator=g)
    dirty = clean.clone()
    dirty[0] = -1          # left out of the counts, kept in n
    dirty[n // 2] = Kc
    for what, idx in (("clean", clean), ("with -1 and K", dirty)):
        if what != "clean" and n == 1:
            continue  # the second write replaces the first: one index, K, and an empty histogram (perplexity 1, nothing active)
        buf, out, st = _code_usage(qa_lib, gpu_device, idx, Kc)
        ppl, active = _finish(qa_lib, st, buf, out, (2,)).tolist()
        p64, a64 = K.code_usage_ref(idx, Kc)
        print(f"code_usage K {Kc} n {n} {what}: perplexity {ppl:.6f} (float64 {float(p64):.6f}), active {active:.0f}")
        assert abs(ppl - float(p64)) <= PPL_TOL * float(p64) and active == float(a64)
        if what == "clean":
            exact = FR.perplexity_exact(idx, Kc)
            assert abs(ppl - exact) <= PPL_TOL * exact and active == len(torch.unique(idx))
            if n * Kc <= 1 << 23:  # the one-hot matrix of code_stats itself; above, through code_usage_ref (pinned to it on the CPU)
                ps, as_ = FR.code_stats(idx, Kc)
                assert abs(ppl - float(ps)) <= PPL_TOL * float(ps) and active == float(as_)
        buf2, out2, st2 = _code_usage(qa_lib, gpu_device, idx, Kc)
        assert torch.equal(_finish(qa_lib, st2, buf2, out2, (2,)), torch.tensor([ppl, active])), "two runs differ"


@pytest.mark.parametrize("Kc,n", [(16385, 10), (8192, 0)], ids=["K=16385", "n=0"])
def test_code_usage_refuses(qa_lib, gpu_device, Kc, n):
    buf, out, st = _code_usage(qa_lib, gpu_device, torch.zeros(10, dtype=torch.int64), Kc, n)
    _refused(qa_lib, st, buf, out)
