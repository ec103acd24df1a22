"""conv_gemm's source-frame table on tile-relative 32-bit offsets: an entry is (clip - clip0) * T_in * ldx +
frame * ldx from the FIRST clip of the row tile, the main loop adds it to one base pointer per thread, and the padding flag of the staged
rows is one mask register that SELECTS +0.  Through qa_conv1d_cl like tests/test_conv_gemm_mfma_shape_gpu.py (dilation and per-clip
lengths, which qa_conv_args does not carry, through the hook qa_debug_conv1d_cl_ex onto the same launch_conv_gemm), on the smallest shapes
at which the addressing can go wrong.

Row grids: B = 5, T_out = 30 (M = 150: the first 128-row tile crosses four clip bases, the second is clamped past M); B = 2, T_out = 130
(a clip boundary inside a tile); B = 1, T_out = 17.  N in {20, 132}.  Every x lies in rows of C_in + 16 floats with other numbers between.
Geometries, each with C_in in {16, 32, 48} on the 5 x 30 grid (16 and 48: the two halves of a 32-wide k group come from different taps):
ksize 3 stride 1 zero "same"; ksize 4 stride 2; ksize 7 reflect; ksize 3 dilation 3; ksize 3 with in_rep 2; ksize 16 stride 8 reflect (the
TAP_WIN rebuild); causal left padding (ksize 4); per-clip lengths {T, 2, T / 3, 1, T - 5} under ksize-7 reflect padding (clips shorter than
the padding: the short-input rule) and under zero padding.  The other grids and N = 20 run a subset (PROBLEMS).
Instances, all of them for every problem: forced tiles QA_GEMM_CFG 0 .. 4 x QA_GEMM_BK16_MIN_TILES 1 / 2^30 (one / two LDS buffers) x
QA_GEMM_PRESPLIT 1 / 0 (weight image attached) x ELU prologue off / on x QA_GEMM_MATH 0, 1, 2, 3 (the fp32 chain, 0, where its
contract admits the problem: C_in % 32 != 0 only with N > 32 and no ELU).

(1) sparse 0 / 1 activations, ones one window apart at another phase in every clip and on the channels in turn, against random weights,
    over as many times the grid's clips as it takes until every (tap, channel) is the one 1 of some window (asserted; with in_rep 2 only
    the first and the last tap can be alone in a window, the middle one is left to (2) and (3)): every output whose
    window holds one 1 equals that weight w[n, tap, channel] - in modes 2 / 3 its first two / one bf16 planes - bit for bit (ELU(1) = 1,
    ELU(0) = 0), every output whose window holds none is +0 (a reflection can show a frame to two taps; such rows are left to (2) and (3)).
    A wrong clip base, tap, half or padding flag fails at its k.
(2) fp64 parity of random problems: QA_GEMM_MATH 0 and 1 under C_PARITY * max(e_cpu32, E_FLOOR) of tests/test_conv_gemm_gpu.py, with and
    without ELU; 2 and 3 under the rounded-operand bounds of tests/test_conv_gemm_modes_gpu.py without ELU (with a signed ELU input that
    file needs another bound; the ELU launches of 2 and 3 are held by (1) and (3)).  Under ksize-7 reflect padding with per-clip lengths
    the rows of a clip's own length are compared - what lies behind them is not defined by the reference.
(3) per problem, prologue and mode every instance gives the same bits, all rows.
(4) padding: with -1.0 in the frames next to the padding, the kernel's own padding, an explicitly padded buffer of +0 and one of -0 give the
    same bits - the sign of a staged zero reaches no output bit - and fp64 parity holds; with inf there, exactly the outputs fp64 leaves
    finite are finite and meet the bound: a padded position is a select, not (frame 0 of the tile's first clip) x 0.

Measured on MI355X: 45 cases in 7.6 s; largest e of (2) 2.9e-7 on the fp32 chain, 2.6e-7 on split-6, against bounds >= 6.0e-7.
"""
import ctypes as C
import functools
import zlib

import pytest
import torch

from tests import test_conv_gemm_gpu as G
from tests import test_conv_gemm_modes_gpu as MD
from tests.gemm_modes_ref import planes, rounded
from tests.util import conv1d_cl, conv_ref, scaled_err, strided_rows

pytestmark = pytest.mark.gpu

TILES = (0, 1, 2, 3, 4)
FORMS = (1, 1 << 30)  # QA_GEMM_BK16_MIN_TILES: one LDS buffer wherever the instance exists; two
MODES = (0, 1, 2, 3)
PLANES = {0: 3, 1: 3, 2: 2, 3: 1}  # bf16 planes of an operand that reach the products (0: all of fp32)

# geometry: T_in and the paddings follow from T_out (_case)
GEOS = {
    "k3_same": dict(k=3, pad=(1, 1)),
    "k4_s2": dict(k=4, stride=2, pad=(1, 1)),
    "k7_reflect": dict(k=7, pad=(3, 3), pad_mode=1),
    "k3_dil3": dict(k=3, pad=(3, 3), dil=3),
    "k3_rep2": dict(k=3, in_rep=2),
    "k16_s8_reflect": dict(k=16, stride=8, pad=(4, 4), pad_mode=1),
    "k4_causal": dict(k=4, pad=(3, 0)),
    "k7_reflect_lens": dict(k=7, pad=(3, 3), pad_mode=1, lens=True),
    "k3_same_lens": dict(k=3, pad=(1, 1), lens=True),
}
PROBLEMS = [(g, 5, 30, 132, c) for g in GEOS for c in (16, 32, 48)] + [
    ("k3_same", 2, 130, 20, 16), ("k4_s2", 2, 130, 132, 48), ("k7_reflect_lens", 2, 130, 132, 32), ("k7_reflect", 1, 17, 20, 48),
    ("k3_same", 1, 17, 132, 32), ("k3_same", 5, 30, 20, 48), ("k7_reflect_lens", 5, 30, 20, 16), ("k16_s8_reflect", 2, 130, 20, 16)]
IDS = [f"{g}-{b}x{t}-N{n}-C{c}" for g, b, t, n, c in PROBLEMS]


def _case(geo, B, T_out):
    c = dict(stride=1, pad=(0, 0), pad_mode=0, dil=1, in_rep=1, lens=None)
    c.update(GEOS[geo])
    c["B"], c["T_out"] = B, T_out
    if c["in_rep"] > 1:  # T_in * in_rep virtual frames + (1, 0 or 1) zeros
        c["T"] = -(-T_out // c["in_rep"])
        c["pad"] = (1, T_out + c["k"] - 2 - c["T"] * c["in_rep"])
    else:
        c["T"] = (T_out - 1) * c["stride"] + (c["k"] - 1) * c["dil"] + 1 - sum(c["pad"])
    if c["lens"]:
        c["lens"] = [c["T"], 2, max(c["T"] // 3, 1), 1, c["T"] - 5][:B]
    return c


def _conv(lib, c, x, w, bias, elu):
    """y [B * T_out, N] of case c; x [B, T, C_in] (a view with row stride ldx), w [N, k, C_in], bias [N] or None: on the device."""
    if c["dil"] == 1 and not c["lens"]:
        return conv1d_cl(lib, x, w, bias, stride=c["stride"], pad=c["pad"], pad_mode=c["pad_mode"], prologue=int(elu), T_out=c["T_out"],
                         in_rep=c["in_rep"]).reshape(-1, w.shape[0])
    from unified_audio_amd import _lib

    fn = lib.qa_debug_conv1d_cl_ex
    fn.restype, fn.argtypes = C.c_int, [C.POINTER(_lib.qa_conv_args), C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    B, T, Cin = x.shape
    N = w.shape[0]
    y = torch.full((B * c["T_out"], N), float("nan"), device=x.device)
    a = _lib.qa_conv_args()
    a.x, a.w, a.y, a.bias = x.data_ptr(), w.data_ptr(), y.data_ptr(), bias.data_ptr() if bias is not None else None
    a.B, a.T_in, a.C_in, a.T_out, a.N = B, T, Cin, c["T_out"], N
    a.ldx, a.ldy, a.ldr, a.ldg = x.stride(1), N, N, N
    a.ksize, a.stride, a.pad_left, a.pad_right, a.pad_mode = c["k"], c["stride"], c["pad"][0], c["pad"][1], c["pad_mode"]
    a.prologue, a.in_rep = int(elu), c["in_rep"]
    lens = torch.tensor(c["lens"], dtype=torch.int32, device=x.device) if c["lens"] else None
    _lib.check(fn(C.byref(a), c["dil"], lens.data_ptr() if lens is not None else None, 1, torch.cuda.current_stream().cuda_stream))
    return y


def _ref(c, x, w, bias, elu, dtype):
    """(y [M, N], scale [M, N], rows [M] bool) on the CPU through tests/util.conv_ref: a dilated kernel (zero padding) as the Linear layer
    over its gathered windows - not as a wider kernel with zero weights between the taps, which would make NaN of an inf the kernel never
    reads; per-clip lengths under zero padding as zeros from the clip's length on; under reflect padding clip by
    clip at its own length, `rows` naming the rows that convolution has (every row otherwise)."""
    k, dil = c["k"], c["dil"]
    case = dict(stride=c["stride"], pad=c["pad"], pad_mode=c["pad_mode"], prologue=int(elu), in_rep=c["in_rep"], T_out=c["T_out"])
    if dil > 1:
        assert c["pad_mode"] == 0 and c["in_rep"] == 1 and not c["lens"]
        xp = torch.nn.functional.pad(x.transpose(1, 2), c["pad"]).transpose(1, 2)  # [B, pad_left + T + pad_right, C_in]
        idx = torch.arange(c["T_out"])[:, None] * c["stride"] + torch.arange(k)[None, :] * dil
        x = xp[:, idx].reshape(x.shape[0], c["T_out"], k * x.shape[2])  # ELU(0) = 0: the prologue may follow the padding
        w = w.reshape(w.shape[0], 1, -1)
        case = dict(stride=1, pad=(0, 0), pad_mode=0, prologue=int(elu), in_rep=1, T_out=c["T_out"])
    M = c["B"] * c["T_out"]
    rows = torch.ones(M, dtype=torch.bool)
    if c["lens"] and c["pad_mode"] == 1:
        y, scale = torch.zeros(M, w.shape[0], dtype=dtype), torch.ones(M, w.shape[0], dtype=dtype)
        rows[:] = False
        for b, L in enumerate(c["lens"]):  # stride 1, pads k - 1 in all: L rows
            yb, sb = conv_ref(x[b:b + 1, :L], w, bias, {**case, "T_out": L}, dtype)
            y[b * c["T_out"]:b * c["T_out"] + L], scale[b * c["T_out"]:b * c["T_out"] + L] = yb, sb
            rows[b * c["T_out"]:b * c["T_out"] + L] = True
        return y, scale, rows
    if c["lens"]:
        x = x.clone()
        for b, L in enumerate(c["lens"]):
            x[b, L:] = 0.0
    y, scale = conv_ref(x, w, bias, case, dtype)
    return y, scale, rows


class _Problem:
    def __init__(self, geo, B, T_out, N, Cin, dev):
        self.c = c = _case(geo, B, T_out)
        g = torch.Generator().manual_seed(zlib_seed(geo, B, T_out, N, Cin))
        T, k = c["T"], c["k"]
        self.x = torch.randn(B, T, Cin, generator=g)
        self.w = torch.randn(N, k, Cin, generator=g) / (k * Cin) ** 0.5
        self.bias = torch.randn(N, generator=g)
        # (1): ones one window apart - so every window holds one, up to reflections - clip b shifted by b, channels in turn; as many times
        # the B clips (the same T_out: the tiles cross clip bases the same way) as it takes to show every (tap, channel) to some window
        span = (k - 1) * c["dil"] + 1
        code = (torch.arange(k * Cin, dtype=torch.float64) + 1.0).view(1, k, Cin)  # the (tap, channel) a window's 1 meets, as a weight
        for R in (1, 2, 4, 8, 16, 32, 64, 128):
            self.ch = {**c, "B": B * R, "lens": c["lens"] * R if c["lens"] else None}
            self.hot = torch.zeros(B * R, T, Cin)
            n, first = 0, torch.randint(Cin, (B * R,), generator=torch.Generator().manual_seed(R)).tolist()
            for b in range(B * R):
                for f in range(b % span, T, span):
                    self.hot[b, f, (n + first[b]) % Cin] = 1.0
                    n += 1
            _, self.hot_exact = self.hot_ref(3)
            met, _, _ = _ref(self.ch, self.hot, code, None, False, torch.float64)
            # in_rep > 1 shows a frame to in_rep neighbouring taps: only the first and the last tap can be alone in a window
            taps = range(k) if c["in_rep"] == 1 else (0, k - 1)
            if set(met[self.hot_exact, 0].long().tolist()) >= {j * Cin + ch + 1 for j in taps for ch in range(Cin)}:
                break
        else:
            raise AssertionError(f"{geo}: the sparse activations do not reach every (tap, channel)")
        self.xd = strided_rows(self.x.to(dev), Cin + 16, 8, generator=g)
        self.hd = strided_rows(self.hot.to(dev), Cin + 16, 8, generator=g)
        self.wd, self.bd = self.w.to(dev), self.bias.to(dev)

    @functools.lru_cache(maxsize=None)
    def parity_ref(self, elu):
        y64, scale, rows = _ref(self.c, self.x, self.w, self.bias, elu, torch.float64)
        y32, _, _ = _ref(self.c, self.x, self.w, self.bias, elu, torch.float32)
        return y64[rows], scale[rows], scaled_err(y32[rows], y64[rows], scale[rows]), rows

    @functools.lru_cache(maxsize=None)
    def rounded_ref(self, n):
        """tests/test_conv_gemm_modes_gpu._oracle_of on this file's geometries: no ELU"""
        xn, wn = rounded(self.x, n), rounded(self.w, n)
        y64, scale, rows = _ref(self.c, xn, wn, self.bias, False, torch.float64)
        y32, _, _ = _ref(self.c, xn, wn, self.bias, False, torch.float32)
        dropped, mm = torch.zeros_like(y64), torch.zeros_like(y64)
        if n == 2:
            mx, mw = planes(self.x, 2)[1], planes(self.w, 2)[1]
            dropped, _, _ = _ref(self.c, mx.abs(), mw.abs(), None, False, torch.float64)
            mm, _, _ = _ref(self.c, mx, mw, None, False, torch.float64)
        return (y64[rows], scale[rows], scaled_err(y32[rows], y64[rows], scale[rows]), dropped[rows], mm[rows]), rows

    def hot_ref(self, n):
        """(want [M, N] float32, exact [M] bool): the outputs of the sparse activations against the weight's first n planes, and the rows
        whose window holds at most one 1 (a reflection can show a frame to two taps of one window)."""
        wn = rounded(self.w, n) if n < 3 else self.w
        y, _, rows = _ref(self.ch, self.hot, wn, None, False, torch.float64)
        hits, _, _ = _ref(self.ch, self.hot, torch.ones_like(self.w[:1]), None, False, torch.float64)
        return y.float(), (hits[:, 0] <= 1.0) & rows  # `rows`: what the reference defines (_ref)


def zlib_seed(*key):
    return zlib.crc32(repr(key).encode())


@functools.lru_cache(maxsize=None)
def _problem(geo, B, T_out, N, Cin, dev):
    return _Problem(geo, B, T_out, N, Cin, dev)


def _instances(knob, lib, mode):
    """Every (tile, buffers, weight source) of a mode in turn: yields its label with the knobs set."""
    for tile in TILES:
        for form in FORMS:
            for presplit in ((1, 0) if mode else (1,)):  # the fp32 chain reads no image
                G._pin_defaults(lib, knob)
                knob("QA_GEMM_MATH", mode)
                knob("QA_GEMM_CFG", tile)
                knob("QA_GEMM_BK16_MIN_TILES", form)
                knob("QA_GEMM_PRESPLIT", presplit)
                yield f"math{mode} cfg{tile} {'one' if form == 1 else 'two'} buffer(s) {'image' if presplit else 'loop'}"


E_MAX = {}


@pytest.mark.parametrize("geo,B,T_out,N,Cin", PROBLEMS, ids=IDS)
def test_every_instance_on_tile_relative_offsets(qa_lib, gpu_device, knob, geo, B, T_out, N, Cin):
    p = _problem(geo, B, T_out, N, Cin, gpu_device)
    c = p.c
    with MD._attached(qa_lib, p.wd):
        for mode in MODES:
            for elu in (False, True):
                if mode == 0 and Cin % 32 and (elu or N <= 32):
                    continue  # the fp32 chain's contract (launch_conv_gemm): C_in % 32 != 0 only for N > 32 without the ELU prologue
                labels, hot, rnd = [], [], []
                for label in _instances(knob, qa_lib, mode):
                    labels.append(f"{label}{' ELU' if elu else ''}")
                    hot.append(_conv(qa_lib, p.ch, p.hd, p.wd, None, elu))
                    rnd.append(_conv(qa_lib, c, p.xd, p.wd, p.bd, elu))
                hot, rnd = torch.stack(hot), torch.stack(rnd)  # compared on the device: only the verdicts and one result come back
                # (3) one result per (problem, prologue, mode), all rows
                for i, label in enumerate(labels):
                    for what, ys in (("sparse", hot), ("random", rnd)):
                        same = ys[i].view(torch.int32) == ys[0].view(torch.int32)
                        assert bool(same.all()), f"{label}: {what} activations, {int((~same).sum())} elements differ from {labels[0]}, " \
                                                 f"first (m, n) = {(~same).nonzero()[0].tolist()}"
                # (1) on the first instance (the others hold the same bits)
                want, exact = p.hot_ref(PLANES[mode])
                bad = (hot[0].view(torch.int32) != want.to(gpu_device).view(torch.int32))[exact.to(gpu_device)].nonzero()
                assert bad.numel() == 0, f"{labels[0]}: sparse activations, {bad.shape[0]} outputs are not the weight their window meets, " \
                                         f"first (row among the exact ones, n) = {bad[0].tolist()}"
                # (2)
                if mode in (0, 1):
                    y64, scale, e32, rows = p.parity_ref(elu)
                    e = scaled_err(rnd[0].cpu()[rows], y64, scale)
                    bound = G.C_PARITY * max(e32, G.E_FLOOR)
                    E_MAX[mode] = max(E_MAX.get(mode, 0.0), e)
                    print(f"table offsets parity {labels[0]}: e {e:.3e} e_cpu32 {e32:.3e} bound {bound:.3e}")
                    assert e <= bound, f"{labels[0]}: {e:.3e} from the fp64 truth, bound {bound:.3e} (fp32 CPU {e32:.3e})"
                elif not elu:
                    ref, rows = p.rounded_ref(PLANES[mode])
                    MD._check_rounded_parity(labels[0], rnd[0].cpu()[rows], ref)
    print("table offsets parity: largest e so far " + ", ".join(f"math{m}: {v:.3e}" for m, v in sorted(E_MAX.items())))


PAD_GEOS = ["k3_same", "k4_causal", "k7_reflect", "k3_dil3", "k3_same_lens"]


@pytest.mark.parametrize("fill", ["minus_one", "inf"])
@pytest.mark.parametrize("geo", PAD_GEOS)
def test_padding_is_a_select(qa_lib, gpu_device, knob, geo, fill):
    B, T_out, N, Cin = 5, 30, 132, 48
    c = _case(geo, B, T_out)
    T = c["T"]
    g = torch.Generator().manual_seed(zlib_seed("pad", geo))
    x = torch.randn(B, T, Cin, generator=g)
    w = torch.randn(N, c["k"], Cin, generator=g) / (c["k"] * Cin) ** 0.5
    bias = torch.randn(N, generator=g)
    # the frames next to the padding - frame 0 is also what a padded position's unconditional load fetches, from the tile's FIRST clip
    ends = [(b, f) for b in range(B) for f in (0, (c["lens"][b] if c["lens"] else T) - 1)]
    for b, f in ends:
        x[b, f] = -1.0
    if fill == "inf":
        for b, f in ends[::3]:
            x[b, f, (7 * b) % Cin] = float("inf")
        x[0, 0, 1] = float("-inf")
    y64, scale, rows = _ref(c, x, w, bias, False, torch.float64)
    y32, _, _ = _ref(c, x, w, bias, False, torch.float32)
    finite = torch.isfinite(y64)
    e32 = scaled_err(y32[finite], y64[finite], scale[finite])
    bound = G.C_PARITY * max(e32, G.E_FLOOR)
    xd, wd, bd = strided_rows(x.to(gpu_device), Cin + 16, 8, generator=g), w.to(gpu_device), bias.to(gpu_device)
    # the same frames between explicit zeros, for the zero-padded geometries without per-clip lengths: no padding left for the kernel
    explicit = c["pad_mode"] == 0 and not c["lens"] and fill == "minus_one"
    if explicit:
        ce = {**c, "pad": (0, 0), "T": T + sum(c["pad"])}
        xe = [torch.full((B, ce["T"], Cin), z) for z in (0.0, -0.0)]
        for t in xe:
            t[:, c["pad"][0]:c["pad"][0] + T] = x
        xe = [strided_rows(t.to(gpu_device), Cin + 16, 8, generator=g) for t in xe]
    with MD._attached(qa_lib, wd):
        for mode in (0, 1):
            for label in _instances(knob, qa_lib, mode):
                y = _conv(qa_lib, c, xd, wd, bd, False).cpu()
                assert torch.equal(torch.isfinite(y)[rows], finite[rows]), \
                    f"{label}: finite pattern differs from fp64 at (m, n) = {(torch.isfinite(y) != finite)[rows].nonzero()[:4].tolist()}"
                ok = finite & rows[:, None]
                e = scaled_err(y[ok], y64[ok], scale[ok])
                assert e <= bound, f"{label}: {e:.3e} from the fp64 truth, bound {bound:.3e} (fp32 CPU {e32:.3e})"
                if explicit:
                    for sign, t in zip("+-", xe):
                        ye = _conv(qa_lib, ce, t, wd, bd, False).cpu()
                        assert torch.equal(ye.view(torch.int32), y.view(torch.int32)), \
                            f"{label}: an explicit padding of {sign}0 gives other bits in {int((ye.view(torch.int32) != y.view(torch.int32)).sum())} elements"
