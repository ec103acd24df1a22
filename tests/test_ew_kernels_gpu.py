"""The HBM-bound float kernels of csrc/ew.hip, each alone through its test hook (qa_debug_*, exported but not in the public header),
against the float64 restatements of tests/ew_ref.py - at the shapes the kernels themselves branch on: C % 256 != 0, C = 2048 (MAX_V4),
rows % 4 != 0, cpg % 4 != 0 (gn_apply's per-element group lookup), C > 1024 (second trip of gn_partial's channel loop), T no multiple
of gn_partial's chunk (32 frames; 64 before the sums became double: both are covered), the 64-block cap of gn_apply's grid, causal
pad_left, rot_heads / interleaved / pos0, and the per-clip ClipLens paths.

Parity.  No tolerance is written down for any input: tol = max(2e-6, 4 x rel_err(torch's own fp32 CPU operator, float64 truth)) on that
same input.  2e-6 is the fp32 convention of tests/test_kernels_gpu.py; the second term is the floor any fp32 implementation has once a
mean rounded to fp32 is subtracted from offset data, times 4 for another summation order.  The kernel's own result never enters it.
Outputs sit between sentinel guards (tests.util.guarded_out): nothing outside may change, everything inside is written and finite.
Bitwise (torch.equal): two runs agree; a row / clip alone equals the same row / clip inside a batch; below a clip's length a ragged call
equals the clip run alone at T = len; behind len * hop the overlap-add is exactly 0; RoPE leaves v, the heads >= rot_heads and the
padding columns of ld untouched.  Refusals: bad shapes return a status without launching (the output keeps its NaNs)."""
import ctypes as C

import pytest
import torch

from tests import ew_ref as E
from tests.util import check_guarded_out, guarded_out, rel_err

pytestmark = pytest.mark.gpu

HEAD = 64  # floats in front of every guarded output (keeps the 16-byte alignment of the float4 stores)
P, I, L, F = C.c_void_p, C.c_int, C.c_longlong, C.c_float
HOOKS = {
    "qa_debug_rownorm": (I, [I, P, P, P, P, L, I, F, P]),
    "qa_debug_dwconv": (I, [P, P, P, P, P, P, I, I, I, I, F, I, P, I, P]),
    "qa_debug_groupnorm_scratch_bytes": (L, [I, I, I]),
    "qa_debug_groupnorm": (I, [P, P, P, P, P, I, I, I, I, F, I, P, I, P]),
    "qa_debug_conv_in": (I, [P, P, P, P, I, I, I, I, I, P, I, P]),
    "qa_debug_rope": (I, [P, P, I, I, I, I, L, I, I, I, P]),
    "qa_debug_istft_spec": (I, [P, P, L, I, I, I, P]),
    "qa_debug_stft_post": (I, [P, P, L, I, I, I, P]),
    "qa_debug_istft_ola": (I, [P, P, P, I, I, I, I, P, I, P]),
    "qa_debug_to_channel_last": (I, [P, L, L, L, P, I, I, I, P]),
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


def _finish(lib, status, buf, y, shape):
    """Status 0, guards intact, every element written and finite -> the output on the host."""
    assert status == 0, lib.qa_last_error()
    torch.cuda.synchronize()
    check_guarded_out(buf, y, HEAD)
    assert torch.isfinite(y).all()
    return y.cpu().reshape(shape).clone()


def _refused(lib, status, buf, y):
    """A refusal: non-zero status with a message, and no launch - the output still holds its NaNs, the guards their sentinels."""
    torch.cuda.synchronize()
    assert status != 0 and lib.qa_last_error()
    assert torch.isnan(y).all()
    y.zero_()
    check_guarded_out(buf, y, HEAD)


def _parity(what, y, ref, yard):
    """rel_err(kernel, truth) <= max(2e-6, 4 x rel_err(torch fp32, truth)) over the frames the truth defines (NaN = behind a clip's end)."""
    live = ~torch.isnan(ref)
    err, floor = rel_err(y[live], ref[live]), rel_err(yard[live], ref[live])
    tol = max(2e-6, 4.0 * floor)
    print(f"{what}: kernel {err:.3e} torch-fp32 {floor:.3e} tol {tol:.3e}")
    assert err <= tol, f"{what}: rel err {err:.3e} > {tol:.3e} (torch fp32 on the same input: {floor:.3e})"


# ------------------------------------------------------------------------------------------------------------ rownorm
def _rownorm(lib, dev, mode, x, w, b, eps, call=None):
    rows, Cc = x.shape
    buf, y = guarded_out(rows, Cc, Cc, HEAD, dev)
    xd, wd, bd = _dev(dev, x, w, b)
    st = lib.qa_debug_rownorm(mode, _p(xd), _p(wd), _p(bd), _p(y), rows, Cc, eps, _stream())
    return (buf, y, st) if call else _finish(lib, st, buf, y, (rows, Cc))


@pytest.mark.parametrize("rows", [1, 5, 130])
@pytest.mark.parametrize("Cc", [4, 64, 252, 256, 260, 1536, 2048])
@pytest.mark.parametrize("mode", [0, 1], ids=["rms", "ln"])
def test_rownorm(hooks, gpu_device, mode, Cc, rows):
    g = _gen(100 + Cc + rows)
    w, b = torch.randn(Cc, generator=g), torch.randn(Cc, generator=g)
    inputs = [("0/1", torch.randn(rows, Cc, generator=g))]
    if rows == 5:
        inputs.append(("100/0.5", 100.0 + 0.5 * torch.randn(rows, Cc, generator=g)))
    for dist, x in inputs:
        for eps in (1e-6, 1e-5):
            for bias in ((None, b) if mode else (None,)):
                y = _rownorm(hooks, gpu_device, mode, x, w, bias, eps)
                _parity(f"rownorm mode {mode} C {Cc} rows {rows} {dist} eps {eps} bias {bias is not None}", y,
                        E.rownorm_ref(x, w, bias, eps, mode), E.rownorm_torch(x, w, bias, eps, mode))
        assert torch.equal(y, _rownorm(hooks, gpu_device, mode, x, w, bias, eps)), "two runs differ"
        for r in {0, rows - 1}:
            assert torch.equal(y[r:r + 1], _rownorm(hooks, gpu_device, mode, x[r:r + 1], w, bias, eps)), f"row {r} alone differs"


@pytest.mark.parametrize("Cc", [6, 2052])
@pytest.mark.parametrize("mode", [0, 1], ids=["rms", "ln"])
def test_rownorm_refuses(hooks, gpu_device, mode, Cc):
    buf, y, st = _rownorm(hooks, gpu_device, mode, torch.randn(2, Cc), torch.ones(Cc), torch.zeros(Cc), 1e-6, call=True)
    _refused(hooks, st, buf, y)


# ------------------------------------------------------------------------------------------------------------ dwconv
def _dwconv(lib, dev, x, w, bias, lnw, lnb, eps, pad_left, lens=None, mul=0, call=None):
    B, T, Cc = x.shape
    buf, y = guarded_out(B * T, Cc, Cc, HEAD, dev)
    xd, wd, bd, lw, lb = _dev(dev, x, w, bias, lnw, lnb)
    ld = _lens(dev, lens)
    st = lib.qa_debug_dwconv(_p(xd), _p(wd), _p(bd), _p(lw), _p(lb), _p(y), B, T, Cc, w.shape[0], eps, pad_left, _p(ld), mul, _stream())
    return (buf, y, st) if call else _finish(lib, st, buf, y, (B, T, Cc))


DW_CASES = [(2, 1, 64, 7, None, 0), (3, 37, 260, 5, None, 0), (1, 130, 1024, 7, None, 0), (2, 9, 2048, 3, None, 0),
            (3, 37, 260, 5, (37, 5, 1), 1), (3, 37, 260, 5, (18, 2, 1), 2)]


@pytest.mark.parametrize("causal", [0, 1], ids=["same", "causal"])
@pytest.mark.parametrize("ln", [0, 1], ids=["plain", "ln"])
@pytest.mark.parametrize("B,T,Cc,k,lens,mul", DW_CASES)
def test_dwconv(hooks, gpu_device, B, T, Cc, k, lens, mul, ln, causal):
    g = _gen(200 + Cc + T)
    x = torch.randn(B, T, Cc, generator=g)
    w, bias = torch.randn(k, Cc, generator=g) / k ** 0.5, torch.randn(Cc, generator=g)
    lnw, lnb = (torch.randn(Cc, generator=g), torch.randn(Cc, generator=g)) if ln else (None, None)
    pad_left, eps = (k - 1 if causal else -1), 1e-6
    frames = None if lens is None else [n * mul for n in lens]
    y = _dwconv(hooks, gpu_device, x, w, bias, lnw, lnb, eps, pad_left, lens, mul)
    _parity(f"dwconv {(B, T, Cc, k)} ln {ln} pad_left {pad_left} lens {lens} x {mul}", y,
            E.dwconv_ref(x, w, bias, lnw, lnb, eps, pad_left, frames), E.dwconv_torch(x, w, bias, lnw, lnb, eps, pad_left, frames))
    assert torch.equal(y, _dwconv(hooks, gpu_device, x, w, bias, lnw, lnb, eps, pad_left, lens, mul)), "two runs differ"
    for b in range(B):
        n = T if frames is None else frames[b]
        alone = _dwconv(hooks, gpu_device, x[b:b + 1, :n], w, bias, lnw, lnb, eps, pad_left)
        assert torch.equal(y[b:b + 1, :n], alone), f"clip {b} alone at T = {n} differs from the clip in the batch"


@pytest.mark.parametrize("Cc,k", [(6, 3), (2052, 3), (64, 4)], ids=["C%4", "C=2052", "even-k"])
def test_dwconv_refuses(hooks, gpu_device, Cc, k):
    buf, y, st = _dwconv(hooks, gpu_device, torch.randn(1, 4, Cc), torch.ones(k, Cc), torch.zeros(Cc), torch.ones(Cc), torch.zeros(Cc),
                         1e-6, -1, call=True)
    _refused(hooks, st, buf, y)


# ------------------------------------------------------------------------------------------------------------ groupnorm
def _groupnorm(lib, dev, x, w, bias, G, eps, swish, lens=None, mul=0, call=None):
    B, T, Cc = x.shape
    buf, y = guarded_out(B * T, Cc, Cc, HEAD, dev)
    xd, wd, bd = _dev(dev, x, w, bias)
    ld = _lens(dev, lens)
    n = int(lib.qa_debug_groupnorm_scratch_bytes(B, T, G))
    assert n > 0 and n % 8 == 0
    scratch = torch.full((n // 8 + 16,), float("nan"), dtype=torch.float64, device=dev)  # 8 NaN doubles on either side
    st = lib.qa_debug_groupnorm(_p(xd), _p(wd), _p(bd), _p(y), scratch[8:].data_ptr(), B, T, Cc, G, eps, swish, _p(ld), mul, _stream())
    if call:
        return buf, y, st
    out = _finish(lib, st, buf, y, (B, T, Cc))
    assert torch.isnan(scratch[:8]).all() and torch.isnan(scratch[-8:]).all(), "groupnorm wrote outside its scratch"
    assert torch.isfinite(scratch[8:-8]).all(), "groupnorm_scratch_bytes covers words the kernels never write"
    return out


GN_DISTS = {"0/1": (0.0, 1.0, False), "3/1": (3.0, 1.0, False), "30/1": (30.0, 1.0, False), "100/0.5": (100.0, 0.5, False),
            "+-30/1": (30.0, 1.0, True), "+-100/0.5": (100.0, 0.5, True)}  # offset / std; True: the sign alternates from group to group
GN_CASES = [(2, 1, 32, 32, None, 0), (2, 33, 64, 32, None, 0), (3, 66, 64, 32, None, 0), (2, 64, 96, 8, None, 0), (1, 200, 768, 32, None, 0),
            (2, 129, 1280, 32, None, 0), (3, 66, 64, 32, (66, 64, 1), 1), (2, 66, 64, 32, (33, 3), 2)]


@pytest.mark.parametrize("swish", [0, 1])
@pytest.mark.parametrize("dist", list(GN_DISTS))
@pytest.mark.parametrize("B,T,Cc,G,lens,mul", GN_CASES)
def test_groupnorm(hooks, gpu_device, B, T, Cc, G, lens, mul, dist, swish):
    g = _gen(300 + Cc + T)
    off, std, alt = GN_DISTS[dist]
    sign = torch.where((torch.arange(Cc) // (Cc // G)) % 2 == 1, -1.0, 1.0) if alt else torch.ones(Cc)
    x = off * sign + std * torch.randn(B, T, Cc, generator=g)
    w, bias = torch.randn(Cc, generator=g), torch.randn(Cc, generator=g)
    eps = 1e-6
    frames = None if lens is None else [n * mul for n in lens]
    y = _groupnorm(hooks, gpu_device, x, w, bias, G, eps, swish, lens, mul)
    _parity(f"groupnorm {(B, T, Cc, G)} {dist} swish {swish} lens {lens} x {mul}", y,
            E.groupnorm_ref(x, w, bias, G, eps, swish, frames), E.groupnorm_torch(x, w, bias, G, eps, swish, frames))
    assert torch.equal(y, _groupnorm(hooks, gpu_device, x, w, bias, G, eps, swish, lens, mul)), "two runs differ"
    for b in range(B):
        n = T if frames is None else frames[b]
        alone = _groupnorm(hooks, gpu_device, x[b:b + 1, :n], w, bias, G, eps, swish)
        assert torch.equal(y[b:b + 1, :n], alone), f"clip {b} alone at T = {n} differs from the clip in the batch"


@pytest.mark.parametrize("Cc,G", [(6, 3), (64, 3)], ids=["C%4", "C%G"])
def test_groupnorm_refuses(hooks, gpu_device, Cc, G):
    buf, y, st = _groupnorm(hooks, gpu_device, torch.randn(1, 4, Cc), torch.ones(Cc), torch.zeros(Cc), G, 1e-6, 0, call=True)
    _refused(hooks, st, buf, y)


# ------------------------------------------------------------------------------------------------------------ conv_in
def _conv_in(lib, dev, x, w, bias, pad_left, lens=None, mul=0, call=None):
    B, T = x.shape
    k, Cout = w.shape
    buf, y = guarded_out(B * T, Cout, Cout, HEAD, dev)
    xd, wd, bd = _dev(dev, x, w, bias)
    ld = _lens(dev, lens)
    st = lib.qa_debug_conv_in(_p(xd), _p(wd), _p(bd), _p(y), B, T, Cout, k, pad_left, _p(ld), mul, _stream())
    return (buf, y, st) if call else _finish(lib, st, buf, y, (B, T, Cout))


@pytest.mark.parametrize("has_bias", [0, 1])
@pytest.mark.parametrize("pad_left", [-1, 6])
@pytest.mark.parametrize("T,lens", [(1, None), (3, None), (4, None), (300, None), (9, (9, 3, 1, 7, 4))])  # clips of 3 and 1 <= the pad (3 | 3, causal 6 | 0)
@pytest.mark.parametrize("Cout", [4, 32, 68])
def test_conv_in(hooks, gpu_device, Cout, T, lens, pad_left, has_bias):
    g = _gen(400 + Cout + T)
    B, k = (len(lens) if lens else 2), 7
    x = torch.randn(B, T, generator=g)
    w = torch.randn(k, Cout, generator=g) / k ** 0.5
    bias = torch.randn(Cout, generator=g) if has_bias else None
    mul = 1 if lens else 0
    y = _conv_in(hooks, gpu_device, x, w, bias, pad_left, lens, mul)
    _parity(f"conv_in Cout {Cout} T {T} pad_left {pad_left} bias {has_bias} lens {lens}", y,
            E.conv_in_ref(x, w, bias, pad_left, lens), E.conv_in_torch(x, w, bias, pad_left, lens))
    assert torch.equal(y, _conv_in(hooks, gpu_device, x, w, bias, pad_left, lens, mul)), "two runs differ"
    for b in range(B):
        n = lens[b] if lens else T
        alone = _conv_in(hooks, gpu_device, x[b:b + 1, :n], w, bias, pad_left)
        assert torch.equal(y[b:b + 1, :n], alone), f"clip {b} alone at T = {n} differs from the clip in the batch"


def test_conv_in_refuses(hooks, gpu_device):
    buf, y, st = _conv_in(hooks, gpu_device, torch.randn(1, 8), torch.ones(7, 6), torch.zeros(6), -1, call=True)
    _refused(hooks, st, buf, y)


# ------------------------------------------------------------------------------------------------------------ rope
def _rope(lib, dev, qkv, cs, H, hd, pos0, interleaved, rot_heads):
    B, N, ld = qkv.shape
    buf, y = guarded_out(B * N, ld, ld, HEAD, dev)
    y.copy_(qkv.reshape(B * N, ld))
    (csd,) = _dev(dev, cs)
    st = lib.qa_debug_rope(_p(y), _p(csd), B, N, H, hd, ld, pos0, interleaved, rot_heads, _stream())
    return _finish(lib, st, buf, y, (B, N, ld))


@pytest.mark.parametrize("rot_heads", [0, 1, 5])
@pytest.mark.parametrize("interleaved", [0, 1])
@pytest.mark.parametrize("pos0", [0, 7])
@pytest.mark.parametrize("slack", [0, 8])
@pytest.mark.parametrize("hd", [8, 64])
def test_rope(hooks, gpu_device, hd, slack, pos0, interleaved, rot_heads):
    g = _gen(500 + hd)
    B, N, H = 2, 5, 3
    d = H * hd
    qkv = torch.randn(B, N, 3 * d + slack, generator=g)
    ang = torch.rand(pos0 + N, hd // 2, generator=g, dtype=torch.float64) * 40.0  # several turns; each position its own angles
    cs = torch.stack((ang.cos(), ang.sin()), -1).float()
    y = _rope(hooks, gpu_device, qkv, cs, H, hd, pos0, interleaved, rot_heads)
    args = (cs, H, hd, pos0, interleaved, rot_heads)
    _parity(f"rope hd {hd} ld 3d+{slack} pos0 {pos0} interleaved {interleaved} rot_heads {rot_heads}", y, E.rope_ref(qkv, *args),
            E.rope_torch(qkv, *args))
    Hr = H if rot_heads == 0 else min(rot_heads, H)
    for part in range(2):  # q and k on their own, so that an error in one of them is not averaged away by the untouched columns
        lo, hi = part * d, part * d + Hr * hd
        _parity(f"rope {'qk'[part]}", y[..., lo:hi], E.rope_ref(qkv, *args)[..., lo:hi], E.rope_torch(qkv, *args)[..., lo:hi])
    for lo, hi, what in ((Hr * hd, d, "q heads >= rot_heads"), (d + Hr * hd, 2 * d, "k heads >= rot_heads"), (2 * d, 3 * d + slack, "v / padding")):
        assert torch.equal(y[..., lo:hi], qkv[..., lo:hi]), f"{what} changed"
    assert torch.equal(y, _rope(hooks, gpu_device, qkv, cs, H, hd, pos0, interleaved, rot_heads)), "two runs differ"
    for b in range(B):
        assert torch.equal(y[b:b + 1], _rope(hooks, gpu_device, qkv[b:b + 1], cs, H, hd, pos0, interleaved, rot_heads)), f"item {b} alone differs"


# ------------------------------------------------------------------------------------------------------------ istft_spec / stft_post
def _rows_op(fn, lib, dev, src, nb, ld_out, call=None):
    rows, ld_in = src.shape
    buf, y = guarded_out(rows, ld_out, ld_out, HEAD, dev)
    (sd,) = _dev(dev, src)
    st = fn(_p(sd), _p(y), rows, nb, ld_in, ld_out, _stream())
    return (buf, y, st) if call else _finish(lib, st, buf, y, (rows, ld_out))


@pytest.mark.parametrize("ld_out", [10, 16])
@pytest.mark.parametrize("ld_in", [10, 12])
def test_istft_spec(hooks, gpu_device, ld_in, ld_out):
    g = _gen(600)
    rows, nb = 3, 5
    src = torch.full((rows, ld_in), float("nan"))  # the padding columns of the input are never read
    src[:, :nb] = torch.linspace(2.0, 7.0, rows * nb).view(rows, nb)  # exp() on both sides of the clip at 100 (log 100 = 4.6)
    src[:, nb:2 * nb] = torch.randn(rows, nb, generator=g) * 20.0      # phases over several turns
    S = _rows_op(hooks.qa_debug_istft_spec, hooks, gpu_device, src, nb, ld_out)
    _parity(f"istft_spec ldy {ld_in} ldS {ld_out}", S, E.istft_spec_ref(src, nb, ld_out), E.istft_spec_torch(src, nb, ld_out))
    assert torch.equal(S[:, 2 * nb:], torch.zeros(rows, ld_out - 2 * nb)), "padding columns are not exactly 0"
    mag = S[:, :nb].double().pow(2).add(S[:, nb:2 * nb].double().pow(2)).sqrt()
    assert float(mag.max()) <= 100.0 * (1 + 1e-6) and 0 < int((mag > 99.99).sum()) < rows * nb
    assert torch.equal(S, _rows_op(hooks.qa_debug_istft_spec, hooks, gpu_device, src, nb, ld_out)), "two runs differ"
    assert torch.equal(S[1:2], _rows_op(hooks.qa_debug_istft_spec, hooks, gpu_device, src[1:2], nb, ld_out)), "row 1 alone differs"


@pytest.mark.parametrize("ld_out", [10, 16])
@pytest.mark.parametrize("ld_in", [10, 12])
def test_stft_post(hooks, gpu_device, ld_in, ld_out):
    g = _gen(601)
    rows, nb = 3, 5
    src = torch.full((rows, ld_in), float("nan"))
    src[:, :2 * nb] = torch.randn(rows, 2 * nb, generator=g)
    src[0, 0] = src[0, nb] = 0.0                      # |X| = 0: log of the clip at 1e-5, angle 0
    src[1, 1], src[1, nb + 1] = -2.0, 0.0             # the negative real axis: +1
    src[1, 2], src[1, nb + 2] = -2.0, -0.0            # ... approached from below: -1
    src[2, 3], src[2, nb + 3] = 3e-6, -4e-6           # 0 < |X| < 1e-5: clipped magnitude, live phase
    out = _rows_op(hooks.qa_debug_stft_post, hooks, gpu_device, src, nb, ld_out)
    _parity(f"stft_post ldi {ld_in} ldo {ld_out}", out, E.stft_post_ref(src, nb, ld_out), E.stft_post_torch(src, nb, ld_out))
    assert float(out[0, nb]) == 0.0 and float(out[1, nb + 1]) > 0.999 and float(out[1, nb + 2]) < -0.999  # the sign of im = -0.0 counts
    assert torch.equal(out[:, 2 * nb:], torch.zeros(rows, ld_out - 2 * nb)), "padding columns are not exactly 0"
    assert torch.equal(out, _rows_op(hooks.qa_debug_stft_post, hooks, gpu_device, src, nb, ld_out)), "two runs differ"
    assert torch.equal(out[1:2], _rows_op(hooks.qa_debug_stft_post, hooks, gpu_device, src[1:2], nb, ld_out)), "row 1 alone differs"


@pytest.mark.parametrize("name", ["qa_debug_istft_spec", "qa_debug_stft_post"])
def test_spectrum_rows_refuse_a_short_leading_dimension(hooks, gpu_device, name):
    buf, y, st = _rows_op(getattr(hooks, name), hooks, gpu_device, torch.zeros(3, 10), 5, 9, call=True)
    _refused(hooks, st, buf, y)


# ------------------------------------------------------------------------------------------------------------ istft_ola
def _ola(lib, dev, frames, win, hop, lens=None, mul=0):
    B, T, n_fft = frames.shape
    buf, y = guarded_out(B, T * hop, T * hop, HEAD, dev)
    fd, wd = _dev(dev, frames, win)
    ld = _lens(dev, lens)
    st = lib.qa_debug_istft_ola(_p(fd), _p(wd), _p(y), B, T, n_fft, hop, _p(ld), mul, _stream())
    return _finish(lib, st, buf, y, (B, T * hop))


@pytest.mark.parametrize("B,T,n_fft,hop,lens", [(2, 1, 16, 4, None), (2, 9, 16, 4, None), (1, 6, 64, 16, None), (2, 9, 16, 4, (9, 1))])
def test_istft_ola(hooks, gpu_device, B, T, n_fft, hop, lens):
    g = _gen(700 + T)
    win = torch.hann_window(n_fft)
    frames = torch.randn(B, T, n_fft, generator=g) * win
    mul = 1 if lens else 0
    y = _ola(hooks, gpu_device, frames, win, hop, lens, mul)
    _parity(f"istft_ola {(B, T, n_fft, hop)} lens {lens}", y, E.istft_ola_ref(frames, win, hop, lens), E.istft_ola_torch(frames, win, hop, lens))
    assert torch.equal(y, _ola(hooks, gpu_device, frames, win, hop, lens, mul)), "two runs differ"
    for b in range(B):
        n = lens[b] if lens else T
        assert torch.equal(y[b, n * hop:], torch.zeros((T - n) * hop)), f"clip {b}: samples behind len * hop are not exactly 0"
        assert torch.equal(y[b:b + 1, :n * hop], _ola(hooks, gpu_device, frames[b:b + 1, :n], win, hop)), f"clip {b} alone at T = {n} differs"


# ------------------------------------------------------------------------------------------------------------ to_channel_last
@pytest.mark.parametrize("source", ["bct", "btc", "slice"])
def test_to_channel_last(hooks, gpu_device, source):
    g = _gen(800)
    B, Cc, T = 2, 33, 35
    if source == "bct":
        view = torch.randn(B, Cc, T, generator=g).to(gpu_device)
    elif source == "btc":
        view = torch.randn(B, T, Cc, generator=g).to(gpu_device).transpose(1, 2)
    else:  # channels 3 .. 35 and every second frame from 5 on of a larger [B, 40, 80] tensor
        view = torch.randn(B, 40, 80, generator=g).to(gpu_device)[:, 3:3 + Cc, 5:5 + 2 * T:2]
    assert view.shape == (B, Cc, T)
    outs = []
    for _ in range(2):
        buf, y = guarded_out(B * T, Cc, Cc, HEAD, gpu_device)
        st = hooks.qa_debug_to_channel_last(view.data_ptr(), view.stride(0), view.stride(1), view.stride(2), _p(y), B, Cc, T, _stream())
        outs.append(_finish(hooks, st, buf, y, (B, T, Cc)))
    assert torch.equal(outs[0], view.cpu().transpose(1, 2)), "a copy: every bit of the source, transposed"
    assert torch.equal(outs[0], outs[1])
