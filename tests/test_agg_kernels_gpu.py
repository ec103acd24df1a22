"""The second half of csrc/ew.hip - the H-Codec 1.5 adaptive-frame-rate kernels, the code layout, the length mask and the ring cache
append - each alone through its test hook (qa_debug_*, exported but not in the public header; codes_check through the public
qa_codes_check / qa_codes_check_async), against the plain restatements of tests/agg_ref.py, which tests/test_agg_ref_cpu.py pins to the
oracle.

Almost everything here is integer indexing, so almost everything is compared EXACTLY (torch.equal).  The align inputs are built with
chosen similarities (agg_ref.chosen_frames): tests/test_agg_ref_cpu.py shows for every case that the closest similarity is >= 0.01 from
the threshold and that the oracle groups alike in float32 and float64, so no case is skipped for a near-tie.  One case sits ON its
threshold, exactly representable, and holds `sim <= thr` against `<`.

Outputs.  Float outputs sit between sentinel guards (tests.util.guarded_out) and start as NaN.  Integer and byte outputs get the same
treatment (_ibuf): GUARD elements on either side and the output itself hold agg_ref.UNWRITTEN (0xAB for bytes); the references mark
what a kernel leaves unwritten with that same value, so one torch.equal checks what is written, what is not, and - gmax / tmax start as
UNWRITTEN too - that the launcher owns their reset.

Parity of the query rows of agg_build (mean of a group's frames + query embedding), the only arithmetic here: the rule of
test_ew_kernels_gpu._parity unchanged, tol = max(2e-6, 4 x rel_err(torch fp32 mean + embedding on the same input, float64 truth)).
Measured on the MI355X over the 54 agg_build cases: kernel at most 3.58e-8, torch fp32 at most 3.57e-8 (tol 2e-6 throughout).

Bitwise besides: two launches agree; an item alone equals the item in its batch; a per-clip call equals the clip alone at T = lens[b]
and writes exact zeros (or nothing, for seg) behind.  Refusals stop on the host: status, message, output untouched."""
import ctypes as C

import pytest
import torch

from tests import agg_ref as A
from tests.test_ew_kernels_gpu import HEAD, _dev, _finish, _gen, _lens, _p, _parity, _refused, _stream
from tests.util import guarded_out

pytestmark = pytest.mark.gpu

GUARD = 64
BYTE_FILL = 0xAB
I32, I64, U8 = torch.int32, torch.int64, torch.uint8
P, I, L, F = C.c_void_p, C.c_int, C.c_longlong, C.c_float
HOOKS = {
    "qa_debug_align": (I, [P, I, I, I, F, I, P, P, P, P, P, P, P]),
    "qa_debug_agg_build": (I, [P, P, P, P, P, P, P, I, I, I, I, P, P]),
    "qa_debug_agg_key_mask": (I, [P, I, I, I, P, P, P]),
    "qa_debug_agg_gather": (I, [P, P, P, P, P, I, I, I, I, P]),
    "qa_debug_agg_query_rows": (I, [P, P, P, P, P, P, P, I, I, I, I, P]),
    "qa_debug_agg_zero_padded": (I, [P, P, I, I, I, P]),
    "qa_debug_codes_inject": (I, [P, P, P, I, I, I, I, I, I, P]),
    "qa_debug_adaptive_frames": (I, [P, I, I, I, I, P, P, P]),
    "qa_debug_token_lengths": (I, [P, P, I, I, I, I, P]),
    "qa_debug_deaggregate": (I, [P, P, P, I, I, I, I, I, P, P]),
    "qa_debug_codes_bqn": (I, [I, P, P, I, I, I, P, P]),
    "qa_debug_len_mask": (I, [P, I, I, P, I, P]),
    "qa_debug_ring_append": (I, [P, P, L, P, P, I, I, I, I, I, P]),
}


@pytest.fixture(scope="module")
def hooks(qa_lib):
    for name, (res, args) in HOOKS.items():
        fn = getattr(qa_lib, name)
        fn.restype, fn.argtypes = res, args
    return qa_lib


def _fill(dtype):
    return BYTE_FILL if dtype == U8 else A.UNWRITTEN


def _ibuf(n, dtype, dev):
    """(buffer, out): out [n] sits GUARD elements into the buffer; all of it holds the fill."""
    buf = torch.full((n + 2 * GUARD,), _fill(dtype), dtype=dtype, device=dev)
    return buf, buf[GUARD:GUARD + n]


def _iout(lib, status, buf, out, shape):
    """Status 0 and nothing outside the output changed -> the output on the host (int64, bytes as they are)."""
    assert status == 0, lib.qa_last_error()
    torch.cuda.synchronize()
    n = out.numel()
    assert bool((buf[:GUARD] == _fill(buf.dtype)).all()) and bool((buf[GUARD + n:] == _fill(buf.dtype)).all()), "wrote outside the output"
    host = out.cpu().reshape(shape).clone()
    return host if buf.dtype == U8 else host.to(I64)


def _irefused(lib, status, *bufs):
    """A refusal: non-zero status with a message, and no launch - every integer buffer still holds its fill."""
    torch.cuda.synchronize()
    assert status != 0 and lib.qa_last_error()
    for buf in bufs:
        assert bool((buf == _fill(buf.dtype)).all()), "a refused call wrote to its output"
    return lib.qa_last_error().decode()


def _i32(dev, t):
    return t.to(I32).to(dev).contiguous()


# ------------------------------------------------------------------------------------------------------------ align
class Aligned:
    """align's five outputs: on the host as int64 (seg, start, len [B, T], nseg [B], gmax) and on the device as the kernel left them."""


def _align(lib, dev, h, thr, mt, lens=None, gmax=None, call=False):
    B, T, D = h.shape
    (hd,) = _dev(dev, h)
    ld = _lens(dev, lens)
    bufs = {k: _ibuf(B * T, I32, dev) for k in ("seg", "start", "len")}
    bufs["nseg"] = _ibuf(B, I32, dev)
    bufs["gmax"] = gmax or _ibuf(1, I32, dev)
    v = {k: b[1] for k, b in bufs.items()}
    st = lib.qa_debug_align(_p(hd), B, T, D, thr, mt, _p(v["seg"]), _p(v["start"]), _p(v["len"]), _p(v["nseg"]), _p(v["gmax"]), _p(ld), _stream())
    if call:
        return st, [b[0] for b in bufs.values()]
    r = Aligned()
    r.dev, r.bufs, r.lens_dev = v, bufs, ld
    r.seg, r.start, r.len = (_iout(lib, st, *bufs[k], (B, T)) for k in ("seg", "start", "len"))
    r.nseg = _iout(lib, st, *bufs["nseg"], (B,))
    r.gmax = int(_iout(lib, st, *bufs["gmax"], (1,)))
    return r


def _same_align(a, b):
    return all(torch.equal(getattr(a, k), getattr(b, k)) for k in ("seg", "start", "len", "nseg")) and a.gmax == b.gmax


def _check_align(r, h, thr, mt, lens):
    seg, start, ln, nseg, gmax = A.align_ref(h, thr, mt, lens)
    assert torch.equal(r.nseg, nseg), (r.nseg.tolist(), nseg.tolist())
    assert torch.equal(r.seg, seg), "seg (group of each frame; UNWRITTEN behind lens[b])"
    assert torch.equal(r.start, start) and torch.equal(r.len, ln), "start / len (T / 0 behind nseg[b])"
    assert r.gmax == gmax
    return seg, start, ln, nseg, gmax


@pytest.mark.parametrize("case", A.ALIGN_CASES, ids=[c["id"] for c in A.ALIGN_CASES])
def test_align(hooks, gpu_device, case):
    h, thr, mt, lens = A.align_input(case), case["thr"], case["mt"], case["lens"]
    B, T, _ = h.shape
    r = _align(hooks, gpu_device, h, thr, mt, lens)
    _, _, _, nseg, _ = _check_align(r, h, thr, mt, lens)
    assert _same_align(r, _align(hooks, gpu_device, h, thr, mt, lens)), "two runs differ"
    for b in range(B):
        n, G = A.clip_len(lens, b, T), int(nseg[b])
        a = _align(hooks, gpu_device, h[b:b + 1, :n], thr, mt)
        assert torch.equal(a.seg[0], r.seg[b, :n]) and torch.equal(a.start[0, :G], r.start[b, :G]) and torch.equal(a.len[0, :G], r.len[b, :G])
        assert int(a.nseg[0]) == G == a.gmax, f"clip {b} alone at T = {n} differs from the clip in the batch"


def test_align_tie_is_a_boundary(hooks, gpu_device):
    """sim == thr exactly (two identical frames of one power-of-two component, thr = 1.0): `sim <= thr` opens a new group."""
    (case,) = [c for c in A.ALIGN_CASES if c["kind"] == "tie"]
    r = _align(hooks, gpu_device, A.align_input(case), 1.0, 8)
    assert r.seg.tolist() == [[0, 1]] and r.nseg.tolist() == [2] and r.start.tolist() == [[0, 1]] and r.len.tolist() == [[1, 1]]


def test_align_resets_gmax(hooks, gpu_device):
    """The launcher owns gmax: a second launch on a batch with fewer groups brings it down."""
    h = A.align_input(dict(kind="chosen", shape=(3, 41, 8), thr=1.0, lens=None))
    gmax = _ibuf(1, I32, gpu_device)
    assert _align(hooks, gpu_device, h, 1.0, 3, gmax=gmax).gmax == 41
    assert _align(hooks, gpu_device, h, -1.0, 8, gmax=gmax).gmax == 6
    assert _align(hooks, gpu_device, h[:1, :5], -1.0, 8, gmax=gmax).gmax == 1


@pytest.mark.parametrize("shape,mt,word", [((1, 4, 6), 8, "align"), ((1, 8193, 4), 8, "8192"), ((1, 4, 8), 0, "align")], ids=["D%4", "T>8192", "max_tokens=0"])
def test_align_refuses(hooks, gpu_device, shape, mt, word):
    st, bufs = _align(hooks, gpu_device, torch.ones(shape), 0.6, mt, call=True)
    assert word in _irefused(hooks, st, *bufs)


# ------------------------------------------------------------------------------------------------------------ agg_build / key_mask / gather
def _feats(case, seed):
    """Features [B, T, D] and a query embedding [D]; behind lens[b] the features are NaN: never to be read."""
    B, T, D = case["shape"]
    g = _gen(seed)
    feats, qemb = 0.5 + torch.randn(B, T, D, generator=g), torch.randn(D, generator=g)
    if case["lens"] is not None:
        for b, n in enumerate(case["lens"]):
            feats[b, n:] = float("nan")
    return feats, qemb


def _agg_build(lib, dev, feats, r, qemb, G, lens_dev=None, call=False):
    B, T, D = feats.shape
    buf, y = guarded_out(B * (T + G), D, D, HEAD, dev)
    fd, qd = _dev(dev, feats, qemb)
    v = r.dev
    st = lib.qa_debug_agg_build(_p(fd), _p(v["seg"]), _p(v["start"]), _p(v["len"]), _p(v["nseg"]), _p(qd), _p(y), B, T, G, D, _p(lens_dev), _stream())
    return (buf, y, st) if call else _finish(lib, st, buf, y, (B, T + G, D))


def _query_rows(start, ln, nseg, T, G):
    rows = torch.zeros(nseg.numel(), T + G, dtype=torch.bool)
    for b in range(nseg.numel()):
        for g in range(min(G, int(nseg[b]))):
            rows[b, int(start[b, g]) + int(ln[b, g]) + g] = True
    return rows


@pytest.mark.parametrize("extra", [0, 3], ids=["G=gmax", "G=gmax+3"])
@pytest.mark.parametrize("case", A.AGG_CASES, ids=[c["id"] for c in A.AGG_CASES])
def test_agg_build(hooks, gpu_device, case, extra):
    h, thr, mt, lens = A.align_input(case), case["thr"], case["mt"], case["lens"]
    B, T, D = h.shape
    r = _align(hooks, gpu_device, h, thr, mt, lens)
    seg, start, ln, nseg, gmax = _check_align(r, h, thr, mt, lens)
    G = gmax + extra
    feats, qemb = _feats(case, 900 + T + D)
    y = _agg_build(hooks, gpu_device, feats, r, qemb, G, r.lens_dev)
    truth = A.agg_build_ref(feats, seg, start, ln, nseg, qemb, G, lens)
    yard = A.agg_build_ref(feats, seg, start, ln, nseg, qemb, G, lens, dtype=torch.float32)
    q = _query_rows(start, ln, nseg, T, G)
    assert int(q.sum()) == int(nseg.sum())
    assert torch.equal(y[~q], truth[~q].float()), "frame rows and padded-group rows are copies; positions behind a clip's row are exactly 0"
    _parity(f"agg_build {case['id']} G {G} query rows", y[q], truth[q], yard[q])
    assert torch.equal(y, _agg_build(hooks, gpu_device, feats, r, qemb, G, r.lens_dev)), "two runs differ"
    for b in range(B):
        n, k = A.clip_len(lens, b, T), int(nseg[b])
        a = _align(hooks, gpu_device, h[b:b + 1, :n], thr, mt)
        Ga = G if lens is None else k  # the rectangular form keeps its padded groups; a per-clip row is the clip alone, and zeros behind
        alone = _agg_build(hooks, gpu_device, feats[b:b + 1, :n], a, qemb, Ga)
        assert torch.equal(y[b, :n + Ga], alone[0]), f"clip {b} alone at T = {n} differs from the clip in the batch"
        assert lens is None or not y[b, n + k:].any()
    if lens is not None:
        mbuf, m = _ibuf(B * (T + G), U8, gpu_device)
        st = hooks.qa_debug_agg_key_mask(_p(m), B, T, G, _p(r.lens_dev), _p(r.dev["nseg"]), _stream())
        mask = _iout(hooks, st, mbuf, m, (B, T + G))
        assert torch.equal(mask, A.agg_key_mask_ref(B, T, G, lens, nseg)), "mask bytes: 1 for the lens[b] + nseg[b] positions of the row, else 0"


def _gather(lib, dev, x, r, G, call=False):
    B, S, D = x.shape
    buf, y = guarded_out(B * G, D, D, HEAD, dev)
    (xd,) = _dev(dev, x)
    v = r.dev
    st = lib.qa_debug_agg_gather(_p(xd), _p(v["start"]), _p(v["len"]), _p(v["nseg"]), _p(y), B, S - G, G, D, _stream())
    return (buf, y, st) if call else _finish(lib, st, buf, y, (B, G, D))


@pytest.mark.parametrize("extra", [0, 3], ids=["G=gmax", "G=gmax+3"])
@pytest.mark.parametrize("case", A.AGG_CASES, ids=[c["id"] for c in A.AGG_CASES])
def test_agg_readout(hooks, gpu_device, case, extra):
    """agg_gather, and agg_query_rows + agg_zero_padded, on a random [B, T + G, D] transformer output with align's grouping."""
    h, thr, mt, lens = A.align_input(case), case["thr"], case["mt"], case["lens"]
    B, T, D = h.shape
    r = _align(hooks, gpu_device, h, thr, mt, lens)
    _, start, ln, nseg, gmax = _check_align(r, h, thr, mt, lens)
    G = gmax + extra
    g = _gen(950 + T + D)
    x = torch.randn(B, T + G, D, generator=g)
    want = A.agg_gather_ref(x, start, ln, nseg, G)
    got = _gather(hooks, gpu_device, x, r, G)
    assert torch.equal(got, want), "valid groups are copies of the query-position rows, padded groups exactly 0"
    assert torch.equal(got, _gather(hooks, gpu_device, x, r, G)), "two runs differ"
    qkv = torch.full((B, T + G, 3 * D), float("nan"))  # k and v columns are never read
    qkv[..., :D] = torch.randn(B, T + G, D, generator=g)
    xd, qd = _dev(gpu_device, x, qkv)
    (bx, xq), (bq, qq) = guarded_out(B * G, D, D, HEAD, gpu_device), guarded_out(B * G, D, D, HEAD, gpu_device)
    v = r.dev
    st = hooks.qa_debug_agg_query_rows(_p(xd), _p(qd), _p(v["start"]), _p(v["len"]), _p(v["nseg"]), _p(xq), _p(qq), B, T, G, D, _stream())
    assert st == 0, hooks.qa_last_error()
    for out in (xq, qq):
        assert hooks.qa_debug_agg_zero_padded(_p(v["nseg"]), _p(out), B, G, D, _stream()) == 0, hooks.qa_last_error()
    assert torch.equal(_finish(hooks, 0, bx, xq, (B, G, D)), want), "xq: agg_gather of x"
    assert torch.equal(_finish(hooks, 0, bq, qq, (B, G, D)), A.agg_gather_ref(qkv[..., :D].contiguous(), start, ln, nseg, G)), "qq: the q columns of the same rows"


@pytest.mark.parametrize("kernel", ["agg_build", "agg_gather", "agg_query_rows", "agg_zero_padded"])
def test_agg_refuses_a_width_that_is_no_multiple_of_4(hooks, gpu_device, kernel):
    B, T, D = 1, 4, 6
    h = torch.ones(B, T, 8)
    r = _align(hooks, gpu_device, h, -1.0, 2)
    G = r.gmax
    assert G == 2
    if kernel == "agg_build":
        buf, y, st = _agg_build(hooks, gpu_device, torch.ones(B, T, D), r, torch.ones(D), G, call=True)
    elif kernel == "agg_gather":
        buf, y, st = _gather(hooks, gpu_device, torch.ones(B, T + G, D), r, G, call=True)
    else:
        buf, y = guarded_out(B * G, D, D, HEAD, gpu_device)
        xd, qd = _dev(gpu_device, torch.ones(B, T + G, D), torch.ones(B, T + G, 3 * D))
        v = r.dev
        if kernel == "agg_query_rows":
            b2, y2 = guarded_out(B * G, D, D, HEAD, gpu_device)
            st = hooks.qa_debug_agg_query_rows(_p(xd), _p(qd), _p(v["start"]), _p(v["len"]), _p(v["nseg"]), _p(y), _p(y2), B, T, G, D, _stream())
            _refused(hooks, st, b2, y2)
        else:
            (nz,) = _dev(gpu_device, torch.zeros(B, dtype=I32))  # every group padded: a launch would zero the output
            st = hooks.qa_debug_agg_zero_padded(_p(nz), _p(y), B, G, D, _stream())
    _refused(hooks, st, buf, y)
    assert kernel in hooks.qa_last_error().decode()


# ------------------------------------------------------------------------------------------------------------ length-injected codes
def _inject(lib, dev, idx, ln_rows, K, pad, call=False):
    """idx [B, G, Q], ln_rows [B, T] (T >= G: the kernel reads len with align's row stride T)."""
    B, G, Q = idx.shape
    T = ln_rows.shape[1]
    buf, out = _ibuf(B * Q * G, I64, dev)
    (idd,) = _dev(dev, idx)
    lnd = _i32(dev, ln_rows)
    st = lib.qa_debug_codes_inject(_p(idd), _p(lnd), _p(out), B, T, G, Q, K, pad, _stream())
    return (st, buf) if call else _iout(lib, st, buf, out, (B, Q, G))


def _token_lengths(lib, dev, codes, K):
    B, Q, G = codes.shape
    buf, out = _ibuf(B * G, I64, dev)
    (cd,) = _dev(dev, codes)
    st = lib.qa_debug_token_lengths(_p(cd), _p(out), B, Q, G, K, _stream())
    return _iout(lib, st, buf, out, (B, G))


def _adaptive_frames(lib, dev, codes, K, tmax=None):
    B, Q, G = codes.shape
    tbuf, tot = _ibuf(B, I32, dev)
    mbuf, mx = tmax or _ibuf(1, I32, dev)
    (cd,) = _dev(dev, codes)
    st = lib.qa_debug_adaptive_frames(_p(cd), B, Q, G, K, _p(tot), _p(mx), _stream())
    return _iout(lib, st, tbuf, tot, (B,)), int(_iout(lib, st, mbuf, mx, (1,)))


@pytest.mark.parametrize("pad", [0, 1], ids=["pad=code-K", "pad=-1"])
@pytest.mark.parametrize("Q", [1, 4])
@pytest.mark.parametrize("K", [3, 1024])
def test_codes_inject_and_lengths(hooks, gpu_device, K, Q, pad):
    B, G, T = 3, 37, 41  # B * Q * G = 111 / 444: no multiple of 256, and a second block
    idx, ln = A.random_codes(20 + K + Q, B, Q, G, K)
    ln[0, :9] = torch.arange(9)  # every length 0 ... 8
    rows = torch.full((B, T), A.UNWRITTEN, dtype=I64)  # len behind G is never read
    rows[:, :G] = ln
    codes = _inject(hooks, gpu_device, idx, rows, K, pad)
    assert torch.equal(codes, A.codes_inject_ref(idx, ln, K, pad))
    padded = (ln == 0).unsqueeze(1).expand(-1, Q, -1)
    assert torch.equal(codes[padded], idx.transpose(1, 2)[padded] - K if pad == 0 else torch.full_like(codes[padded], -1))
    assert torch.equal(codes, _inject(hooks, gpu_device, idx, rows, K, pad)), "two runs differ"
    for b in range(B):
        assert torch.equal(codes[b:b + 1], _inject(hooks, gpu_device, idx[b:b + 1], rows[b:b + 1], K, pad)), f"item {b} alone differs"
    # round trip: the lengths come back, 0 for padded groups in either form
    assert torch.equal(_token_lengths(hooks, gpu_device, codes, K), ln)
    totals, tmax = _adaptive_frames(hooks, gpu_device, codes, K)
    assert torch.equal(totals, ln.sum(1)) and tmax == int(ln.sum(1).max())
    # hand-built codes below -K: length -1 (floor division), which contributes no frame
    low = codes.clone()
    low[:, 0, 5] = -K - 1
    low[1, 0, 0] = -2 * K
    tl = _token_lengths(hooks, gpu_device, low, K)
    assert torch.equal(tl, A.token_lengths_ref(low, K)) and tl[:, 5].tolist() == [-1] * B and int(tl[1, 0]) == -1
    want, wmax = A.adaptive_frames_ref(low, K)
    totals, tmax = _adaptive_frames(hooks, gpu_device, low, K)
    assert torch.equal(totals, want) and tmax == wmax and torch.equal(want, tl.clamp_min(0).sum(1))


def test_adaptive_frames_resets_tmax(hooks, gpu_device):
    K, Q = 3, 4
    idx, ln = A.random_codes(31, 70, Q, 37, K)  # 70 items: a second block of the 64-thread grid
    codes = A.codes_inject_ref(idx, ln, K, 1)
    tmax = _ibuf(1, I32, gpu_device)
    totals, m = _adaptive_frames(hooks, gpu_device, codes, K, tmax)
    assert torch.equal(totals, ln.sum(1)) and m == int(ln.sum(1).max())
    small = A.codes_inject_ref(idx[:2, :3], ln[:2, :3], K, 1)
    totals, m = _adaptive_frames(hooks, gpu_device, small, K, tmax)
    assert torch.equal(totals, ln[:2, :3].sum(1)) and m == int(ln[:2, :3].sum(1).max()) < int(ln.sum(1).max())


def test_codes_inject_refuses_more_groups_than_len_has_rows(hooks, gpu_device):
    st, buf = _inject(hooks, gpu_device, torch.zeros(1, 5, 1, dtype=I64), torch.ones(1, 4, dtype=I64), 3, 0, call=True)
    assert "codes_inject" in _irefused(hooks, st, buf)


# ------------------------------------------------------------------------------------------------------------ deaggregate
def _deaggregate(lib, dev, codes, len_codes, T, K, cap=None, call=False):
    B, Q, G = codes.shape
    buf, out = _ibuf(B * T * Q, I64, dev)
    cd, lcd = _dev(dev, codes, len_codes)
    capd = _lens(dev, cap)
    st = lib.qa_debug_deaggregate(_p(cd), _p(lcd), _p(out), B, Q, G, T, K, _p(capd), _stream())
    return (st, buf) if call else _iout(lib, st, buf, out, (B, T, Q))


@pytest.mark.parametrize("K,Q", [(3, 1), (1024, 4)])
@pytest.mark.parametrize("G", [1, 7, 64, 65, 1024])
def test_deaggregate(hooks, gpu_device, G, K, Q):
    B = 3
    idx, ln = A.random_codes(40 + G, B, Q, G, K)
    other, _ = A.random_codes(41 + G, B, Q, G, K)
    totals = ln.sum(1)
    tmax = int(totals.max())
    own = ln.clone()  # this stream dropped groups the other stream kept: negative codes (code - K, -1) that ARE repeated, as code % K
    own[:, 0] = 0
    own[1, G // 2] = 0
    for pad in (0, 1):
        codes = A.codes_inject_ref(idx, own, K, pad)              # this stream's codes ...
        codes[2, :, min(1, G - 1)] = -K - 1                       # ... one of them below -K
        len_codes = A.codes_inject_ref(other, ln, K, 1 - pad)     # ... repeated by the OTHER stream's lengths (the acoustic call)
        for T in sorted({tmax, tmax + 5, max(tmax - 7, 1)}):
            out = _deaggregate(hooks, gpu_device, codes, len_codes, T, K)
            assert torch.equal(out, A.deaggregate_ref(codes, len_codes, T, K)), f"T {T} (largest total {tmax}) pad form {pad}"
        assert torch.equal(out, _deaggregate(hooks, gpu_device, codes, len_codes, T, K)), "two runs differ"
        for b in range(B):
            assert torch.equal(out[b:b + 1], _deaggregate(hooks, gpu_device, codes[b:b + 1], len_codes[b:b + 1], T, K)), f"item {b} alone differs"
        cap = [0, max(int(totals[1]) - 3, 0), tmax + 5]
        capped = _deaggregate(hooks, gpu_device, codes, len_codes, tmax, K, cap)
        assert torch.equal(capped, A.deaggregate_ref(codes, len_codes, tmax, K, cap)), f"cap {cap}"
        assert not capped[0].any() and not capped[1, cap[1]:].any()


def test_deaggregate_refuses_more_than_1024_groups(hooks, gpu_device):
    codes = torch.zeros(1, 1, 1025, dtype=I64)
    st, buf = _deaggregate(hooks, gpu_device, codes, codes, 4, 3, call=True)
    assert "1024" in _irefused(hooks, st, buf)


# ------------------------------------------------------------------------------------------------------------ code layout, length mask
def _bqn(lib, dev, direction, src, lens=None):
    B, a, b = src.shape
    N, Q = (a, b) if direction == 0 else (b, a)
    buf, out = _ibuf(B * N * Q, I64, dev)
    (sd,) = _dev(dev, src)
    ld = _lens(dev, lens)
    st = lib.qa_debug_codes_bqn(direction, _p(sd), _p(out), B, N, Q, _p(ld), _stream())
    return _iout(lib, st, buf, out, (B, Q, N) if direction == 0 else (B, N, Q))


@pytest.mark.parametrize("B,N,Q,lens", [(1, 1, 1, (1,)), (3, 37, 4, (37, 5, 1)), (2, 300, 8, (131, 300))])
def test_codes_bqn(hooks, gpu_device, B, N, Q, lens):
    src = torch.randint(1024, (B, N, Q), generator=_gen(50 + N))
    for use in (None, lens):
        x = src.clone()
        if use is not None:
            for b, n in enumerate(use):
                x[b, n:] = 777777  # poison: behind lens[b] the entries become -1 whatever the source holds
        to = _bqn(hooks, gpu_device, 0, x, use)
        assert torch.equal(to, A.codes_bqn_ref(x, 0, use))
        back = _bqn(hooks, gpu_device, 1, x.transpose(1, 2).contiguous(), use)
        assert torch.equal(back, A.codes_bqn_ref(x.transpose(1, 2).contiguous(), 1, use))
        trip = _bqn(hooks, gpu_device, 1, to, use)
        for b in range(B):
            n = N if use is None else use[b]
            assert torch.equal(trip[b, :n], src[b, :n]) and (trip[b, n:] == -1).all(), "from(to(x)) == x on the live part, -1 behind"
            assert torch.equal(to[b:b + 1], _bqn(hooks, gpu_device, 0, x[b:b + 1], None if use is None else use[b:b + 1])), f"item {b} alone differs"
        assert torch.equal(to, _bqn(hooks, gpu_device, 0, x, use)), "two runs differ"


@pytest.mark.parametrize("mul,lens", [(1, (3, 10, 12, 1)), (2, (2, 5, 7, 1))])  # lens * mul below, equal to and above N
def test_len_mask(hooks, gpu_device, mul, lens):
    B, N = 4, 10
    outs = []
    for _ in range(2):
        buf, m = _ibuf(B * N, U8, gpu_device)
        st = hooks.qa_debug_len_mask(_p(m), B, N, _p(_lens(gpu_device, lens)), mul, _stream())
        outs.append(_iout(hooks, st, buf, m, (B, N)))
    assert torch.equal(outs[0], A.len_mask_ref(B, N, lens, mul)) and torch.equal(outs[0], outs[1])
    assert set(outs[0].flatten().tolist()) == {0, 1}


def test_len_mask_refuses_a_call_without_lengths(hooks, gpu_device):
    buf, m = _ibuf(8, U8, gpu_device)
    _irefused(hooks, hooks.qa_debug_len_mask(_p(m), 2, 4, None, 1, _stream()), buf)


# ------------------------------------------------------------------------------------------------------------ codes_check / codes_count
@pytest.mark.parametrize("n", [1, 255, 257, 262221])  # 262221 > 1024 blocks x 256: the grid-stride loop runs
def test_codes_check(hooks, gpu_device, n):
    limit = 1024
    codes = torch.randint(limit, (n,), generator=_gen(60 + n))
    spots = sorted({0, n // 2, n - 1})
    codes[spots[0]] = limit            # first
    codes[spots[-1]] = -2              # last
    codes[spots[len(spots) // 2]] = -1 if n > 2 else codes[spots[len(spots) // 2]]  # middle: the dropped code, legal only with lo = -1
    want0 = int(((codes < 0) | (codes >= limit)).sum())
    want1 = int(((codes < -1) | (codes >= limit)).sum())
    assert want0 == len(spots) and want1 == len(spots) - (1 if n > 2 else 0)
    (cd,) = _dev(gpu_device, codes)
    bad = C.c_int64(-7)
    for _ in range(2):  # the synchronous call resets its count
        assert hooks.qa_codes_check(_p(cd), n, limit, C.byref(bad), _stream()) == 0, hooks.qa_last_error()
        assert bad.value == want0
    buf, cnt = _ibuf(1, I64, gpu_device)
    cnt.zero_()
    for calls, lo, want in ((1, 0, want0), (2, 0, 2 * want0), (3, -1, 2 * want0 + want1)):  # no reset: the count accumulates
        assert hooks.qa_codes_check_async(_p(cd), n, lo, limit, _p(cnt), _stream()) == 0, hooks.qa_last_error()
        assert int(_iout(hooks, 0, buf, cnt, (1,))) == want, f"after {calls} asynchronous calls"


# ------------------------------------------------------------------------------------------------------------ ring_append
def _ring(lib, dev, fused, kc, vc, d, pos0, call=False):
    """fused [B, T, 3 d] = (q | k | v) rows as the QKV projection leaves them; kc, vc [B, cap, d]."""
    B, T, ld = fused.shape
    cap = kc.shape[1]
    (fd,) = _dev(dev, fused)
    outs = []
    for cache in (kc, vc):
        buf, y = guarded_out(B * cap, d, d, HEAD, dev)
        if not call:
            y.copy_(cache.reshape(B * cap, d))
        outs.append((buf, y))
    st = lib.qa_debug_ring_append(fd.data_ptr() + 4 * d, fd.data_ptr() + 8 * d, ld, _p(outs[0][1]), _p(outs[1][1]), B, T, d, cap, pos0, _stream())
    if call:
        return st, outs
    return [_finish(lib, st, buf, y, (B, cap, d)) for buf, y in outs]


@pytest.mark.parametrize("pos", ["0", "cap-1", "7cap+2", "1e6+3"])
@pytest.mark.parametrize("chunk", ["1", "3", "cap"])
@pytest.mark.parametrize("cap", [5, 32])
def test_ring_append(hooks, gpu_device, cap, chunk, pos):
    B, d = 2, 12
    T = {"1": 1, "3": 3, "cap": cap}[chunk]
    pos0 = {"0": 0, "cap-1": cap - 1, "7cap+2": 7 * cap + 2, "1e6+3": 10 ** 6 + 3}[pos]
    g = _gen(70 + cap + T)
    fused = torch.randn(B, T, 3 * d, generator=g)
    fused[..., :d] = float("nan")  # the q part is never read
    kc, vc = torch.randn(B, cap, d, generator=g), torch.randn(B, cap, d, generator=g)
    got = _ring(hooks, gpu_device, fused, kc, vc, d, pos0)
    want = A.ring_append_ref(fused[..., d:2 * d], fused[..., 2 * d:], kc, vc, pos0)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), "rows land at (pos0 + t) % cap, every other cache row is untouched"
    again = _ring(hooks, gpu_device, fused, kc, vc, d, pos0)
    assert torch.equal(got[0], again[0]) and torch.equal(got[1], again[1]), "two runs differ"
    alone = _ring(hooks, gpu_device, fused[1:], kc[1:], vc[1:], d, pos0)
    assert torch.equal(got[0][1:], alone[0]) and torch.equal(got[1][1:], alone[1]), "item 1 alone differs"


@pytest.mark.parametrize("T,cap,d", [(6, 5, 12), (2, 5, 6)], ids=["T>cap", "d%4"])
def test_ring_append_refuses(hooks, gpu_device, T, cap, d):
    st, outs = _ring(hooks, gpu_device, torch.ones(1, T, 3 * d), torch.ones(1, cap, d), torch.ones(1, cap, d), d, 0, call=True)
    for buf, y in outs:
        _refused(hooks, st, buf, y)
        assert "ring_append" in hooks.qa_last_error().decode()
