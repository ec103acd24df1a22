"""The kernels of csrc/seanet_front.hip, csrc/ssl_kernels.hip and csrc/conformer_kernels.hip, each alone through its test hook
(qa_debug_*, exported but not in the public header), against the float64 restatements of tests/front_kernels_ref.py - at the shapes
the kernels themselves branch on: the 128-frame tiles of the fused SEANet front with L % 128 in {0, 1, 2}, L at the L >= 8 floor, the
causal paddings, hid < 16 and a launch of more than 2 x 768 tiles (grid-stride loop, both wav-window buffers reused); the 64-frame chunks
of the SSL layer 0 with C0 > 256 (second trip of the channel loop), every ksize / stride pair, offset input (the double-precision
statistics) and per-clip lengths; the wave-per-job gate with hd below / no multiple of 64 and a partial last workgroup; the 64 x 64
tiles of the Conformer convolution module with clamped halos and channels and shorter reference kernels centred into the 31 taps.

Parity.  No tolerance is written down for any input: tol = max(2e-6, 4 x rel_err(torch's own fp32 CPU operators, float64 truth)) on that
same input.  2e-6 is the suite's fp32 convention; the second term is the floor any fp32 implementation has on that input, times 4 for
another summation order.  The kernel's own result never enters it.  Outputs sit between sentinel guards (tests.util.guarded_out):
nothing outside may change, everything inside is written and finite.  Bitwise (torch.equal): two runs agree; a clip / row alone equals
the same clip / row inside a batch; below a clip's length a ragged call equals the clip run alone at T = wav_len; a tile grid shifted
along the frames gives the same interior frames.  Refusals: bad shapes return a status without launching (the output keeps its NaNs)."""
import ctypes as C

import pytest
import torch

from tests import front_kernels_ref as K
from tests.test_front_kernels_ref_cpu import seanet_weights
from tests.util import check_guarded_out, guarded_out, rel_err, with_knob

pytestmark = pytest.mark.gpu

HEAD = 64  # floats in front of every guarded output (keeps the 16-byte alignment of the float4 stores)
NAN = float("nan")
P, I, L, F = C.c_void_p, C.c_int, C.c_longlong, C.c_float
HOOKS = {
    "qa_debug_seanet_front_supported": (I, [I, I, I]),
    "qa_debug_seanet_front": (I, [P] * 10 + [I, I, I, I, I, P]),
    "qa_debug_ssl_conv0_scratch_bytes": (L, [I, I, I]),
    "qa_debug_ssl_conv0": (I, [P] * 7 + [I, I, I, I, I, I, I, I, F, I, P, P, P]),
    "qa_debug_ssl_gate": (I, [P, P, P, P, P, I, I, I, I, P]),
    "qa_debug_ssl_accumulate": (I, [P, P, L, I, P]),
    "qa_debug_ssl_act": (I, [P, L, I, P]),
    "qa_debug_ssl_compress": (I, [P, P, L, F, F, P, I, I, P]),
    "qa_debug_glu_dwconv_bn_silu": (I, [P, P, P, P, P, P, I, I, I, P]),
    "qa_debug_masked_add": (I, [P, P, P, L, I, P]),
    "qa_debug_mask_count": (I, [P, I, I, P, P]),
    "qa_debug_logmel_frames": (I, [P, I, L, I, L, P, P]),
    "qa_debug_log_eps": (I, [P, L, F, P]),
    "qa_debug_cond_prompt": (I, [P, P, P, I, I, I, P]),
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


# ------------------------------------------------------------------------------------------------------------ seanet_front
def _seanet(lib, dev, wav, W, hid, causal, Cc=32, null=None, call=None):
    """W: the eight reference-layout tensors of tests.test_front_kernels_ref_cpu.seanet_weights (float32)."""
    B, Ls = wav.shape
    w0, b0, w3, b3, wsc, bsc, wpw, bpw = W
    w3p, b3p = K.pack_k3(w3, b3)
    ops = _dev(dev, wav, K.pack_conv0(w0), b0, w3p, b3p, K.pack_shortcut(wsc), bsc, K.pack_pw(wpw), bpw)
    buf, y = guarded_out(B * Ls, Cc, Cc, HEAD, dev)
    ptrs = [_p(t) for t in ops]
    if null is not None:
        ptrs[null] = None
    st = lib.qa_debug_seanet_front(*ptrs, _p(y), B, Ls, Cc, hid, causal, _stream())
    return (buf, y, st) if call else _finish(lib, st, buf, y, (B, Ls, Cc))


@pytest.mark.parametrize("causal", [0, 1], ids=["same", "causal"])
@pytest.mark.parametrize("hid", [16, 5])
@pytest.mark.parametrize("Ls", [8, 9, 127, 128, 129, 130, 257, 300])
def test_seanet_front(hooks, gpu_device, Ls, hid, causal):
    """The plain parity rule holds: no absolute term for elu_f's exp(x) - 1 (<= 6e-8 per ELU, csrc/common.h) is added to it."""
    g = _gen(1000 + Ls + hid)
    B = 3
    W = seanet_weights(g, 32, hid, torch.float32)
    assert hooks.qa_debug_seanet_front_supported(32, hid, Ls) == 1
    for dist, wav in (("0/1", torch.randn(B, Ls, generator=g)), ("3/0.5", 3.0 + 0.5 * torch.randn(B, Ls, generator=g))):
        y = _seanet(hooks, gpu_device, wav, W, hid, causal)
        ref = K.seanet_front_ref(wav, *W, causal)
        assert 0.02 < float((ref < 0).double().mean()) < 0.98, "the last ELU is used on one side only"
        _parity(f"seanet_front L {Ls} hid {hid} causal {causal} B {B} {dist}", y, ref, K.seanet_front_torch(wav, *W, causal))
        assert torch.equal(y, _seanet(hooks, gpu_device, wav, W, hid, causal)), "two runs differ"
        for b in range(B):  # B = 1
            alone = _seanet(hooks, gpu_device, wav[b:b + 1], W, hid, causal)
            assert torch.equal(y[b:b + 1], alone), f"clip {b} alone differs from the clip in the batch"
            _parity(f"seanet_front L {Ls} hid {hid} causal {causal} B 1 clip {b} {dist}", alone, ref[b:b + 1],
                    K.seanet_front_torch(wav[b:b + 1], *W, causal))


@pytest.mark.parametrize("causal", [0, 1], ids=["same", "causal"])
def test_seanet_front_persistent_trips(hooks, gpu_device, causal):
    """13 x 120 = 1560 tiles on the 768 persistent workgroups: workgroups 0 .. 23 make three trips (both wav-window buffers are
    reused, the second one fetched while the first is computed on); a clip alone is 120 tiles, one trip each."""
    g = _gen(1100)
    B, Ls, hid = 13, 128 * 119 + 1, 16
    assert B * ((Ls + 127) // 128) > 1536
    W = seanet_weights(g, 32, hid, torch.float32)
    wav = torch.randn(B, Ls, generator=g)
    y = _seanet(hooks, gpu_device, wav, W, hid, causal)
    _parity(f"seanet_front persistent B {B} L {Ls} causal {causal}", y, K.seanet_front_ref(wav, *W, causal), K.seanet_front_torch(wav, *W, causal))
    for b in range(B):
        assert torch.equal(y[b:b + 1], _seanet(hooks, gpu_device, wav[b:b + 1], W, hid, causal)), f"clip {b} alone differs from the clip in the batch"


@pytest.mark.parametrize("case", ["C=64", "hid=0", "hid=17", "L=7", "null", "knob"])
def test_seanet_front_refuses(hooks, gpu_device, case):
    g = _gen(1200)
    Cc, hid, Ls, null = 32, 16, 16, None
    if case == "C=64":
        Cc = 64
    elif case.startswith("hid="):
        hid = int(case[4:])
    elif case == "L=7":
        Ls = 7
    elif case == "null":
        null = 3  # the k3 weight
    W = seanet_weights(g, Cc, max(1, min(hid, 16)), torch.float32)
    wav = torch.randn(2, Ls, generator=g)
    if case == "knob":
        assert hooks.qa_debug_seanet_front_supported(Cc, hid, Ls) == 1
        with with_knob("QA_SEANET_FUSED", 0):
            assert hooks.qa_debug_seanet_front_supported(Cc, hid, Ls) == 0
            buf, y, st = _seanet(hooks, gpu_device, wav, W, hid, 0, call=True)
            _refused(hooks, st, buf, y)
        assert hooks.qa_debug_seanet_front_supported(Cc, hid, Ls) == 1
        return
    if null is None:
        assert hooks.qa_debug_seanet_front_supported(Cc, hid, Ls) == 0
    buf, y, st = _seanet(hooks, gpu_device, wav, W, hid, 0, Cc=Cc, null=null, call=True)
    _refused(hooks, st, buf, y)


# ------------------------------------------------------------------------------------------------------------ ssl_conv0
def _conv0(lib, dev, wav, w, bias, gamma, beta, T1, stride, pad, norm, act, wav_len=None, l0_len=None, eps=1e-5, ksize=None, call=None):
    B, T = wav.shape
    C0, _, k = w.shape
    buf, y = guarded_out(B * T1, C0, C0, HEAD, dev)
    wd, wpk, bd, gd, bed = _dev(dev, wav, K.pack_conv0(w), bias, gamma, beta)
    wl, ll = _lens(dev, wav_len), _lens(dev, l0_len)
    n = int(lib.qa_debug_ssl_conv0_scratch_bytes(B, T1, C0))
    n_partial = B * ((T1 + 63) // 64) * C0 * 2
    assert n == n_partial * 8 + B * C0 * 2 * 4 and n % 8 == 0
    scratch = torch.full((n // 8 + 16,), NAN, dtype=torch.float64, device=dev)  # 8 NaN doubles on either side
    st = lib.qa_debug_ssl_conv0(_p(wd), _p(wpk), _p(bd), _p(gd), _p(bed), _p(y), scratch[8:].data_ptr(), B, T, T1, C0, ksize or k, stride,
                                pad, norm, eps, act, _p(wl), _p(ll), _stream())
    if call:
        return buf, y, st
    out = _finish(lib, st, buf, y, (B, T1, C0))
    assert torch.isnan(scratch[:8]).all() and torch.isnan(scratch[-8:]).all(), "ssl_conv0 wrote outside its scratch"
    if norm:
        assert torch.isfinite(scratch[8:8 + n_partial]).all(), "chunk partials that no workgroup wrote"
        assert torch.isfinite(scratch[8 + n_partial:-8].view(torch.float32)).all(), "statistics that ssl_gn_finalize never wrote"
    return out


def _conv0_Ts(T1, k, stride, pad):
    """Signal lengths for a call of T1 frames: the length whose padded convolution has exactly T1 frames, where that signal holds at
    least one window of samples; and, with padding, T1 stride + k samples of which only the first T1 frames are asked for (the
    launcher takes T1 as given), so that real data lies under every frame behind the front padding whatever T1 is."""
    natural = (T1 - 1) * stride + k - 2 * pad
    return sorted(({natural} if natural >= k else set()) | ({T1 * stride + k} if pad else set()))


@pytest.mark.parametrize("C0", [4, 256, 260, 512])
@pytest.mark.parametrize("k,stride", [(10, 5), (16, 4), (1, 1), (3, 2)])
def test_ssl_conv0(hooks, gpu_device, k, stride, C0):
    """T1 = 1 .. 130 frames (one chunk, a chunk less one, exactly one, one more, three) at the signal lengths of _conv0_Ts: no call is
    padding only.  Every (norm, bias) form is run twice (same bits).  B = 1 is every first and last clip run alone, bit-equal to the
    clip in the batch of 3."""
    g = _gen(2000 + 16 * k + C0)
    B = 3
    w = torch.randn(C0, 1, k, generator=g) * (2.0 / k) ** 0.5
    cb, gamma, beta = torch.randn(C0, generator=g) * 0.3, 1.0 + 0.1 * torch.randn(C0, generator=g), 0.3 * torch.randn(C0, generator=g)
    for T1 in (1, 63, 64, 65, 130):
        for pad, T in [(pad, T) for pad in (0, 160) for T in _conv0_Ts(T1, k, stride, pad)]:
            assert T >= k, "a signal shorter than one window"
            for dist, wav in (("0/1", torch.randn(B, T, generator=g)), ("100/0.5", 100.0 + 0.5 * torch.randn(B, T, generator=g))):
                for norm, act, bias in ((1, K.ACT_GELU, None), (1, K.ACT_GELU, cb), (0, K.ACT_NONE, cb), (0, K.ACT_NONE, None)):
                    args = ((gamma, beta) if norm else (None, None)) + (T1, stride, pad, norm, 1e-5, act)
                    y = _conv0(hooks, gpu_device, wav, w, bias, *args[:6], args[7])
                    _parity(f"ssl_conv0 k {k} s {stride} C0 {C0} T1 {T1} T {T} pad {pad} B {B} norm {norm} bias {bias is not None} {dist}", y,
                            K.ssl_conv0_ref(wav, w, bias, *args), K.ssl_conv0_torch(wav, w, bias, *args))
                    assert torch.equal(y, _conv0(hooks, gpu_device, wav, w, bias, *args[:6], args[7])), f"two runs differ (norm {norm})"
                    if bias is None:
                        continue
                    for b in (0, B - 1):  # B = 1
                        alone = _conv0(hooks, gpu_device, wav[b:b + 1], w, cb, *args[:6], args[7])
                        assert torch.equal(y[b:b + 1], alone), f"clip {b} alone differs from the clip in the batch (norm {norm})"


@pytest.mark.parametrize("norm,act", [(1, K.ACT_GELU), (0, K.ACT_NONE)], ids=["group-gelu", "plain"])
@pytest.mark.parametrize("C0,T1,pad,l0", [(260, 130, 0, (130, 100, 64, 10)), (8, 200, 160, (200, 130, 128, 65))])
def test_ssl_conv0_ragged(hooks, gpu_device, C0, T1, pad, l0, norm, act):
    """One full clip, one ending inside a chunk, one on a chunk boundary, one in the first chunk (with pad = 160 the shortest clip the
    padding allows: 65 frames).  Samples behind wav_len[b] hold NaN: a single load of one would show in a frame or a statistic."""
    g = _gen(2100 + C0)
    k, stride, B = 10, 5, len(l0)
    T = (T1 - 1) * stride + k - 2 * pad + 3
    wav_len = [T] + [(n - 1) * stride + k - 2 * pad + 2 for n in l0[1:]]
    assert all(1 <= n <= T and (n + 2 * pad - k) // stride + 1 == f for n, f in zip(wav_len, l0))
    w = torch.randn(C0, 1, k, generator=g) * (2.0 / k) ** 0.5
    cb, gamma, beta = torch.randn(C0, generator=g) * 0.3, 1.0 + 0.1 * torch.randn(C0, generator=g), 0.3 * torch.randn(C0, generator=g)
    gb = (gamma, beta) if norm else (None, None)
    for dist, wav in (("0/1", torch.randn(B, T, generator=g)), ("100/0.5", 100.0 + 0.5 * torch.randn(B, T, generator=g))):
        poisoned = wav.clone()
        for b, n in enumerate(wav_len):
            poisoned[b, n:] = NAN
        y = _conv0(hooks, gpu_device, poisoned, w, cb, *gb, T1, stride, pad, norm, act, wav_len, l0)  # finite everywhere (_finish)
        assert torch.equal(y, _conv0(hooks, gpu_device, poisoned, w, cb, *gb, T1, stride, pad, norm, act, wav_len, l0)), "two runs differ"
        ref, yard = torch.full((B, T1, C0), NAN, dtype=torch.float64), torch.zeros(B, T1, C0)
        for b, (n, f) in enumerate(zip(wav_len, l0)):
            ref[b, :f] = K.ssl_conv0_ref(wav[b:b + 1, :n], w, cb, *gb, f, stride, pad, norm, 1e-5, act)[0]
            yard[b, :f] = K.ssl_conv0_torch(wav[b:b + 1, :n], w, cb, *gb, f, stride, pad, norm, 1e-5, act)[0]
            alone = _conv0(hooks, gpu_device, wav[b:b + 1, :n], w, cb, *gb, f, stride, pad, norm, act)
            assert torch.equal(y[b:b + 1, :f], alone), f"clip {b}: frames < l0_len differ from the clip alone at T = wav_len"
        _parity(f"ssl_conv0 ragged C0 {C0} T1 {T1} pad {pad} l0 {l0} norm {norm} {dist}", y, ref, yard)


@pytest.mark.parametrize("case", ["ksize=17", "C0%4", "wav_len-only", "l0_len-only", "lds"])
def test_ssl_conv0_refuses(hooks, gpu_device, case):
    C0, k, stride, ksize, wl, ll = 8, 10, 5, None, None, None
    if case == "ksize=17":
        k, ksize = 16, 17  # the filter buffer holds 16 taps; the launcher returns before anything reads it
    elif case == "C0%4":
        C0 = 6
    elif case == "wav_len-only":
        wl = [100, 100]
    elif case == "l0_len-only":
        ll = [4, 4]
    elif case == "lds":
        stride = 300  # (64 x 300 + 16 + 10 x 8) floats > 64 KB
    T1 = 4
    wav = torch.randn(2, (T1 - 1) * stride + 17)
    buf, y, st = _conv0(hooks, gpu_device, wav, torch.ones(C0, 1, k), torch.zeros(C0), torch.ones(C0), torch.zeros(C0), T1, stride, 0, 1,
                        K.ACT_GELU, wl, ll, ksize=ksize, call=True)
    _refused(hooks, st, buf, y)


# ------------------------------------------------------------------------------------------------------------ ssl_gate
def _gate(lib, dev, hidden, w8, b8, cst, H):
    B, N, d = hidden.shape
    wab, bab = K.pack_gate(w8, b8)
    buf, y = guarded_out(B * H, N, N, HEAD, dev)
    hd_, wd, bd, cd = _dev(dev, hidden, wab, bab, cst)
    st = lib.qa_debug_ssl_gate(_p(hd_), _p(wd), _p(bd), _p(cd), _p(y), B, N, H, d // H, _stream())
    return _finish(lib, st, buf, y, (B, H, N))


@pytest.mark.parametrize("B,N", [(2, 4), (1, 5), (3, 5), (1, 1)])
@pytest.mark.parametrize("H", [1, 3, 12])
@pytest.mark.parametrize("hd", [32, 64, 96, 128])
def test_ssl_gate(hooks, gpu_device, hd, H, B, N):
    """B N H % 4 over the (B, N) list: H = 1 -> 0, 1, 3, 1; H = 3 -> 0, 3, 1, 3; H = 12 -> 0 (a full last workgroup) every time."""
    g = _gen(3000 + hd + H)
    hidden = torch.randn(B, N, H * hd, generator=g)
    w8, b8 = torch.randn(8, hd, generator=g) * (2.0 / hd) ** 0.5, torch.randn(8, generator=g) * 0.3
    cst = 1.0 + 0.3 * torch.randn(H, generator=g)
    y = _gate(hooks, gpu_device, hidden, w8, b8, cst, H)
    ref = K.ssl_gate_ref(hidden, w8, b8, cst, H)
    assert y.shape == ref.shape == (B, H, N)
    _parity(f"ssl_gate hd {hd} H {H} B {B} N {N} (jobs % 4 = {B * N * H % 4})", y, ref, K.ssl_gate_torch(hidden, w8, b8, cst, H))
    assert torch.equal(y, _gate(hooks, gpu_device, hidden, w8, b8, cst, H)), "two runs differ"
    for b, i in {(0, 0), (B - 1, N - 1)}:
        alone = _gate(hooks, gpu_device, hidden[b:b + 1, i:i + 1], w8, b8, cst, H)
        assert torch.equal(y[b:b + 1, :, i:i + 1], alone), f"row ({b}, {i}) alone differs from the row in the batch"


# ------------------------------------------------------------------------------------------------------------ ssl tail
def _flat(fn, lib, dev, n, fill, *args, call=None):
    """An in-place / destination buffer of n floats between guards, filled with `fill` (a tensor, or None to keep the NaNs)."""
    buf, y = guarded_out(1, n, n, HEAD, dev)
    if fill is not None:
        y.copy_(fill.reshape(1, n))
    st = fn(_p(y), *args, _stream())
    return (buf, y, st) if call else _finish(lib, st, buf, y, (n,))


@pytest.mark.parametrize("n", [4, 1036, 5000])
def test_ssl_accumulate(hooks, gpu_device, n):
    g = _gen(4000 + n)
    assert n % 4 == 0 and n % 256 != 0
    src, dst = torch.randn(n, generator=g), torch.randn(n, generator=g)
    (sd,) = _dev(gpu_device, src)
    first = _flat(hooks.qa_debug_ssl_accumulate, hooks, gpu_device, n, None, _p(sd), n, 1)  # the destination's NaNs must not leak
    assert torch.equal(first, src), "first = 1 is a copy"
    for _ in range(2):
        assert torch.equal(_flat(hooks.qa_debug_ssl_accumulate, hooks, gpu_device, n, dst, _p(sd), n, 0), dst + src), "dst += src, one fp32 add"


@pytest.mark.parametrize("n", [4, 1036, 5000])
def test_ssl_act(hooks, gpu_device, n):
    g = _gen(4100 + n)
    x = torch.randn(n, generator=g) * 3.0
    y = _flat(hooks.qa_debug_ssl_act, hooks, gpu_device, n, x, n, K.ACT_GELU)
    _parity(f"ssl_act gelu n {n}", y, K._gelu(x.double()), torch.nn.functional.gelu(x))
    assert torch.equal(y, _flat(hooks.qa_debug_ssl_act, hooks, gpu_device, n, x, n, K.ACT_GELU)), "two runs differ"
    assert torch.equal(_flat(hooks.qa_debug_ssl_act, hooks, gpu_device, n, x, n, K.ACT_NONE), x), "ACT_NONE changes bits"


def _compress(lib, dev, s, scale, expo, lens=None, N=0, d=0, call=None):
    n = s.numel()
    buf, y = guarded_out(1, n, n, HEAD, dev)
    (sd,) = _dev(dev, s)
    ld = _lens(dev, lens)
    st = lib.qa_debug_ssl_compress(_p(sd), _p(y), n, scale, expo, _p(ld), N, d, _stream())
    return (buf, y, st) if call else _finish(lib, st, buf, y, tuple(s.shape))


@pytest.mark.parametrize("expo", [0.3, 0.0])
def test_ssl_compress(hooks, gpu_device, expo):
    g = _gen(4200)
    B, N, d = 2, 37, 7
    assert B * N * d % 256 != 0
    s = torch.randn(B, N, d, generator=g) * 3.0
    tiny = torch.tensor([0.0, -0.0, 1e-30, -1e-30, 3e-37, -3e-37, 1e-20])
    s[0, 0] = tiny
    scale = 1.0 / 3.0
    y = _compress(hooks, gpu_device, s, scale, expo)
    _parity(f"ssl_compress expo {expo}", y, K.ssl_compress_ref(s, scale, expo), K.ssl_compress_torch(s, scale, expo))
    _parity(f"ssl_compress expo {expo} tiny inputs", y[0, 0, 2:], K.ssl_compress_ref(s, scale, expo)[0, 0, 2:],
            K.ssl_compress_torch(s, scale, expo)[0, 0, 2:])
    assert torch.equal(y[0, 0, :2].abs(), torch.zeros(2)), "+-0 does not stay 0"
    if expo > 0:
        assert bool((y[s > 0] > 0).all()) and bool((y[s < 0] < 0).all()), "the sign of the input is lost"
    assert torch.equal(y, _compress(hooks, gpu_device, s, scale, expo)), "two runs differ"
    lens = [N, 5]
    holes = s.clone()
    holes[1, 5:] = NAN
    yl = _compress(hooks, gpu_device, holes, scale, expo, lens, N, d)
    assert torch.equal(yl[1, 5:], torch.zeros(N - 5, d)), "rows behind n_len are not exactly 0"
    assert torch.equal(yl[0], y[0]) and torch.equal(yl[1, :5], y[1, :5]), "rows below n_len differ from the plain call"


@pytest.mark.parametrize("name", ["qa_debug_ssl_accumulate", "qa_debug_ssl_act"])
def test_ssl_flat_kernels_refuse_n_not_a_multiple_of_4(hooks, gpu_device, name):
    n = 1034
    (sd,) = _dev(gpu_device, torch.randn(n))
    args = (_p(sd), n, 1) if name.endswith("accumulate") else (n, K.ACT_GELU)
    buf, y, st = _flat(getattr(hooks, name), hooks, gpu_device, n, None, *args, call=True)
    _refused(hooks, st, buf, y)


def test_ssl_compress_refuses_lengths_without_a_shape(hooks, gpu_device):
    buf, y, st = _compress(hooks, gpu_device, torch.randn(2, 5, 4), 1.0, 0.3, [5, 2], 0, 0, call=True)
    _refused(hooks, st, buf, y)


# ------------------------------------------------------------------------------------------------------------ glu_dwconv_bn_silu
def _glu_dw(lib, dev, u, w, bias, bn, B=None, T=None, Cc=None, call=None):
    Bu, Tu, C2 = u.shape
    B, T, Cc = Bu if B is None else B, Tu if T is None else T, C2 // 2 if Cc is None else Cc
    sc, sh = K.pack_batchnorm(*bn)
    buf, y = guarded_out(max(B * T, 1), max(Cc, 1), max(Cc, 1), HEAD, dev)
    ud, wd, bd, scd, shd = _dev(dev, u, K.pack_dw31(w), bias, sc, sh)
    st = lib.qa_debug_glu_dwconv_bn_silu(_p(ud), _p(wd), _p(bd), _p(scd), _p(shd), _p(y), B, T, Cc, _stream())
    return (buf, y, st) if call else _finish(lib, st, buf, y, (B, T, Cc))


def _glu_dw_operands(g, B, T, Cc, k):
    u = torch.randn(B, T, 2 * Cc, generator=g)
    u[..., Cc:] *= torch.where(torch.arange(Cc) % 3 == 0, 40.0, 1.0)  # every third channel: gates of +-40 and more
    u[:, 0, Cc], u[:, -1, 2 * Cc - 1] = 50.0, -100.0                   # sigmoid = 1 and = 0 exactly in fp32
    w, bias = torch.randn(Cc, 1, k, generator=g) / k ** 0.5, torch.randn(Cc, generator=g) * 0.3
    bn = (1.0 + 0.1 * torch.randn(Cc, generator=g), 0.3 * torch.randn(Cc, generator=g), 0.2 * torch.randn(Cc, generator=g),
          0.3 + 1.5 * torch.rand(Cc, generator=g))
    return u, w, bias, bn


@pytest.mark.parametrize("Cc", [4, 60, 64, 68, 256])
@pytest.mark.parametrize("T", [1, 15, 63, 64, 65, 130])
def test_glu_dwconv_bn_silu(hooks, gpu_device, T, Cc):
    B = 3
    for k in (31, 15, 7, 1):
        g = _gen(5000 + 7 * T + Cc + k)
        u, w, bias, bn = _glu_dw_operands(g, B, T, Cc, k)
        sig = torch.sigmoid(u[..., Cc:])
        assert bool((sig == 0).any()) and bool((sig == 1).any()), "no gate saturates"
        y = _glu_dw(hooks, gpu_device, u, w, bias, bn)
        _parity(f"glu_dwconv T {T} C {Cc} B {B} k {k}", y, K.glu_dwconv_bn_silu_ref(u, w, bias, *bn), K.glu_dwconv_bn_silu_torch(u, w, bias, *bn))
        assert torch.equal(y, _glu_dw(hooks, gpu_device, u, w, bias, bn)), "two runs differ"
        for b in (0, B - 1):  # B = 1
            assert torch.equal(y[b:b + 1], _glu_dw(hooks, gpu_device, u[b:b + 1], w, bias, bn)), f"clip {b} alone differs from the clip in the batch"


@pytest.mark.parametrize("t0", [7, 40])
@pytest.mark.parametrize("Cc", [64, 68])
def test_glu_dwconv_tile_grid_shift(hooks, gpu_device, Cc, t0):
    """Frames [64, 128) of a T = 130 run are the tile [64, 128); run on frames [t0, T) alone they straddle two tiles.  They lie >= 15
    frames from the cut at t0 (and the other end is the same end), so the zero padding makes it the same operation: same bits."""
    g = _gen(5100 + Cc)
    T, k = 130, 31
    assert 64 - t0 >= k // 2
    u, w, bias, bn = _glu_dw_operands(g, 2, T, Cc, k)
    full = _glu_dw(hooks, gpu_device, u, w, bias, bn)
    cut = _glu_dw(hooks, gpu_device, u[:, t0:], w, bias, bn)
    assert torch.equal(full[:, 64:128], cut[:, 64 - t0:128 - t0])
    assert not torch.equal(full[:, t0:t0 + 15], cut[:, :15]), "the cut is not seen at all"


@pytest.mark.parametrize("zero", ["B", "T", "C"])
def test_glu_dwconv_refuses_an_empty_shape(hooks, gpu_device, zero):
    u, w, bias, bn = _glu_dw_operands(_gen(5200), 1, 4, 8, 31)
    shape = dict(B=1, T=4, Cc=8)
    shape["Cc" if zero == "C" else zero] = 0
    buf, y, st = _glu_dw(hooks, gpu_device, u, w, bias, bn, call=True, **shape)
    _refused(hooks, st, buf, y)


# ------------------------------------------------------------------------------------------------------------ masked_add / mask_count
def _masked_add(lib, dev, x, y, valid, rows=None, Cc=None, call=None):
    r, c = x.shape
    bx, xd = guarded_out(r, c, c, HEAD, dev)
    by, yd = guarded_out(r, c, c, HEAD, dev)
    if not call:
        xd.copy_(x)
    yd.copy_(y)
    vd = None if valid is None else valid.to(torch.uint8).to(dev)
    st = lib.qa_debug_masked_add(_p(xd), _p(yd), _p(vd), r if rows is None else rows, c if Cc is None else Cc, _stream())
    if call:
        return bx, xd, st
    return _finish(lib, st, bx, xd, (r, c)), _finish(lib, st, by, yd, (r, c))


@pytest.mark.parametrize("rows,Cc", [(1, 4), (37, 12), (300, 8)])
@pytest.mark.parametrize("mask", ["null", "ones", "mixed"])
def test_masked_add(hooks, gpu_device, mask, rows, Cc):
    g = _gen(6000 + rows)
    x, y = torch.randn(rows, Cc, generator=g), torch.randn(rows, Cc, generator=g)
    valid = {"null": None, "ones": torch.ones(rows, dtype=torch.bool), "mixed": torch.rand(rows, generator=g) < 0.6}[mask]
    if mask == "mixed":
        valid[0] = False
    want_y = y if valid is None else torch.where(valid[:, None], y, torch.zeros_like(y))
    for _ in range(2):
        gx, gy = _masked_add(hooks, gpu_device, x, y, valid)
        assert torch.equal(gy, want_y), "y is not zeroed in place on exactly the masked rows"
        assert torch.equal(gx, x + want_y), "x += y is one fp32 add"


@pytest.mark.parametrize("rows,Cc", [(3, 6), (0, 8)], ids=["C%4", "rows=0"])
def test_masked_add_refuses(hooks, gpu_device, rows, Cc):
    buf, xd, st = _masked_add(hooks, gpu_device, torch.zeros(3, 8), torch.ones(3, 8), None, rows, Cc, call=True)
    _refused(hooks, st, buf, xd)


@pytest.mark.parametrize("T", [1, 63, 64, 65, 1000])
def test_mask_count(hooks, gpu_device, T):
    g = _gen(6100 + T)
    valid = torch.stack((torch.zeros(T), torch.ones(T), (torch.rand(T, generator=g) < 0.5).float(), (torch.rand(T, generator=g) < 0.9).float()))
    B = valid.shape[0]
    vd = valid.to(torch.uint8).to(gpu_device)
    for _ in range(2):
        counts = torch.full((B + 16,), -7, dtype=torch.int32, device=gpu_device)
        assert hooks.qa_debug_mask_count(_p(vd), B, T, counts[8:].data_ptr(), _stream()) == 0, hooks.qa_last_error()
        torch.cuda.synchronize()
        assert counts[8:8 + B].tolist() == valid.sum(1).long().tolist()
        assert counts[:8].tolist() == counts[-8:].tolist() == [-7] * 8, "mask_count wrote outside counts [B]"


# ------------------------------------------------------------------------------------------------------------ logmel_frames / log_eps / cond_prompt
def _logmel_frames(lib, dev, wav, pad, n_out, n=None, call=None):
    B = wav.shape[0]
    buf, y = guarded_out(B, n_out, n_out, HEAD, dev)
    (wd,) = _dev(dev, wav)
    st = lib.qa_debug_logmel_frames(_p(wd), B, wav.shape[1] if n is None else n, pad, n_out, _p(y), _stream())
    return (buf, y, st) if call else _finish(lib, st, buf, y, (B, n_out))


@pytest.mark.parametrize("extra", [-50, 0, 333], ids=["shorter", "equal", "longer"])
@pytest.mark.parametrize("pad", [0, 320])
@pytest.mark.parametrize("n", [1, 700])
def test_logmel_frames(hooks, gpu_device, n, pad, extra):
    n_out = max(1, n + pad + extra)
    wav = torch.randn(2, n, generator=_gen(7000 + n))
    for _ in range(2):
        P_ = _logmel_frames(hooks, gpu_device, wav, pad, n_out)
        assert torch.equal(P_, K.logmel_frames_torch(wav, pad, n_out)) and torch.equal(P_, K.logmel_frames_ref(wav, pad, n_out))


def test_logmel_frames_refuses_an_empty_signal(hooks, gpu_device):
    buf, y, st = _logmel_frames(hooks, gpu_device, torch.randn(2, 8), 4, 16, n=0, call=True)
    _refused(hooks, st, buf, y)


@pytest.mark.parametrize("n", [1, 777, 4096])
def test_log_eps(hooks, gpu_device, n):
    x = torch.rand(n, generator=_gen(7100 + n)) * 10.0
    x[::7] = 0.0  # log(0 + eps)
    x[1::7] *= 1e-9
    y = _flat(hooks.qa_debug_log_eps, hooks, gpu_device, n, x, n, 1e-10)
    _parity(f"log_eps n {n}", y, K.log_eps_ref(x, 1e-10), K.log_eps_torch(x, 1e-10))
    _parity(f"log_eps n {n} x = 0", y[::7], K.log_eps_ref(x, 1e-10)[::7], K.log_eps_torch(x, 1e-10)[::7])
    assert torch.equal(y, _flat(hooks.qa_debug_log_eps, hooks, gpu_device, n, x, n, 1e-10)), "two runs differ"


@pytest.mark.parametrize("B,T,d", [(1, 1, 6), (3, 1, 5), (3, 5, 6), (2, 40, 130)])
def test_cond_prompt(hooks, gpu_device, B, T, d):
    g = _gen(7200 + T)
    sos, cond = torch.randn(d, generator=g), torch.randn(B, T, d, generator=g)
    sd, cd = _dev(gpu_device, sos, cond)
    for _ in range(2):
        buf, y = guarded_out(B * (T + 1), d, d, HEAD, gpu_device)
        st = hooks.qa_debug_cond_prompt(_p(y), _p(sd), _p(cd), B, T, d, _stream())
        assert torch.equal(_finish(hooks, st, buf, y, (B, T + 1, d)), K.cond_prompt_ref(sos, cond))
