"""conv_gemm's reduced arithmetics: split-3 (QA_GEMM_MATH = 2: two bf16 planes per operand, products hm, mh, hh) and bf16 (3: one plane,
one product), both with fp32 accumulation and both opt-in.  Built on the problems, knob paths and bound of tests/test_conv_gemm_gpu.py.

A bf16 x bf16 product is exact in fp32, so a mode that keeps n planes computes, up to its fp32 accumulation, the convolution of the
operands rounded to n planes (tests/gemm_modes_ref.rounded) - minus, for n = 2, the dropped plane product mm.

(1) exact-operand parity: the problems of the geometries ragged, k9, k16, in_rep3, ssl_pos on the paths table_bk16, linear_bk16, cin48 with a
    linear epilogue (bias, gamma, residual; no activation), and one 128-column problem whose weight has a pre-split image, used and ignored
    (QA_GEMM_PRESPLIT = 0).  Oracle: conv_ref in fp64 on the rounded operands.  Bound, mode 3: C_PARITY * max(e_cpu32, E_FLOOR), e_cpu32 the
    fp32 CPU evaluation of the same rounded operands.  Mode 2: elementwise that bound plus the dropped term, |gamma| conv(|m_x|, |m_w|) in
    fp64, over the same scale - and, sharper, the parity bound alone against the oracle minus the signed mm.  On a build where 2 and 3 run split-6 this fails: tests/test_gemm_modes_ref_cpu.py shows the rounded-operand
    oracle of mode 3 is > 100 bounds from the true operands' result.
(2) the ELU prologue: with non-negative inputs it is the identity and (1) applies unchanged; with signed inputs the kernel rounds ELU(x),
    which the oracle cannot restate bit for bit, so the error against the fp64 result of the TRUE operands is held to
    (2u + u^2) conv(|x|, |w|) / scale + the fp32 parity bound, u = 2^-8 (mode 3) / 2^-16 (mode 2): |ELU(x)| <= |x|.
(3) per mode, the problems of tests/test_conv_gemm_gpu.py are bit-identical over every tile, BK 16 / 32, QA_GEMM_LINEAR, QA_GEMM_XCD,
    QA_GEMM_PANEL - the walk of test_conv_gemm_knobs_are_bit_identical, here with a pre-split image attached, so that the 128-column tiles
    read it - over QA_GEMM_PRESPLIT 0 / 1, and over a batch split in two calls.
(4) the modes are what they say: mode 3 equals mode 1 bit for bit on operands that are bf16 already, mode 2 equals mode 1 on a two-plane
    operand (l = 0) against a bf16 one, either way round (every product split-3 leaves out is then exactly zero, and x + 0 = x; with m != 0
    in both operands split-6 also has mm, so l = 0 alone is not enough), and modes 0 and 1 give the same bits before and after a mode-2 /
    mode-3 launch.
(5) the non-finite and cancellation cases of tests/test_conv_gemm_split_gpu.py in modes 2 and 3.

Every check prints its figures (pytest -s).  Measured on MI355X over the 30 parity checks of (1), (2) and (5) per mode: bf16 e = 5.9e-8 .. 3.8e-7;
split-3 1.1e-7 .. 5.8e-7 against the oracle minus the signed mm (0 .. 4.4e-7 beyond the bound on the dropped term); bounds 6.0e-7 .. 2.6e-6.
On the parent's library, where 2 and 3 run split-6, 27 of the 30 cases of (1) fail, and so do the image, ELU, wide-range and (4) cases.
"""
import functools
import zlib

import pytest
import torch

from tests import test_conv_gemm_gpu as G
from tests.gemm_modes_ref import PLANES_OF_MODE, UNIT, planes, rounded
from tests.util import conv1d_cl, conv_ref, scaled_err

pytestmark = pytest.mark.gpu

MODES = (2, 3)
PLAIN = [(g, p) for g in ("ragged", "k9", "k16", "in_rep3", "ssl_pos") for p in ("table_bk16", "linear_bk16", "cin48")]
IMAGE_GEO = dict(B=1, T=300, Cin=96, N=136, k=1, gamma=True)  # 300 x 136 x 96: two column tiles of a forced 128-column tile, ragged in M and N


def _linear_epilogue(c):
    return {k: v for k, v in c.items() if k not in ("act", "post")}


@functools.lru_cache(maxsize=None)
def plain_problem(geo, path, dev, **over):
    """The (geo, path) problem of tests/test_conv_gemm_gpu.py without its activations: bias, gamma and residual only."""
    c = {**_linear_epilogue({**G.GEOS[geo], **G.PATHS[path][1]}), **over}
    return G.Problem(c, dev, zlib.crc32(f"modes/{geo}/{c['Cin']}/{sorted(over.items())}".encode()))


def _oracle_of(x, w, prob, n):
    """(y64, scale, e_cpu32, dropped, mm) of the operands rounded to n planes; dropped [M, N] >= 0 bounds the plane products a mode leaves
    out, mm is their signed sum as it reaches the output (n = 2: gamma conv(m_x, m_w); else zero)."""
    kw = dict(gamma=prob.gamma, residual=prob.res, gate=prob.gate)
    xn, wn = rounded(x, n), rounded(w, n)
    y64, scale = conv_ref(xn, wn, prob.bias, prob.c, torch.float64, **kw)
    y32, _ = conv_ref(xn, wn, prob.bias, prob.c, torch.float32, **kw)
    dropped, mm = torch.zeros_like(y64), torch.zeros_like(y64)
    if n == 2:
        assert prob.gate is None and not prob.c.get("prologue")
        mx, mw = planes(x, 2)[1], planes(w, 2)[1]
        dropped, _ = conv_ref(mx.abs(), mw.abs(), None, prob.c, torch.float64, gamma=None if prob.gamma is None else prob.gamma.abs())
        mm, _ = conv_ref(mx, mw, None, prob.c, torch.float64, gamma=prob.gamma)
    return y64, scale, scaled_err(y32, y64, scale), dropped, mm


@functools.lru_cache(maxsize=None)
def _oracle_cached(prob, n):
    return _oracle_of(prob.x, prob.w, prob, n)


def oracle(prob, n):
    return _oracle_cached(prob, n)


def _check_rounded_parity(label, y, ref):
    y64, scale, e32, dropped, mm = ref
    bound = G.C_PARITY * max(e32, G.E_FLOOR)
    err = (y.cpu().double() - y64).abs()
    e = float(((err - dropped).clamp_min(0) / (scale + 1e-30)).max())
    # sharper than the bound on the dropped term: the kernel's products are exact, so it computes the rounded operands' result MINUS the signed
    # mm, up to its fp32 accumulation - which separates split-3 from a kernel that issued mm as well, or ran split-6
    e_exact = scaled_err(y.cpu(), y64 - mm, scale)
    print(f"modes parity {label}: e {e:.3e} (raw {scaled_err(y.cpu(), y64, scale):.3e}, dropped term up to "
          f"{float((dropped / (scale + 1e-30)).max()):.3e}), against the oracle minus the signed dropped term {e_exact:.3e}; "
          f"e_cpu32 {e32:.3e} bound {bound:.3e}")
    assert e <= bound, f"{label}: {e:.3e} from the fp64 result of the rounded operands beyond the dropped term, bound {bound:.3e}"
    assert e_exact <= bound, f"{label}: {e_exact:.3e} from the fp64 result of the products the mode keeps, bound {bound:.3e}"


def _image(lib, w):
    from unified_audio_amd import _lib

    planes_ = torch.zeros(w.numel() * 6, dtype=torch.uint8, device=w.device)
    _lib.check(lib.qa_weight_planes(w.data_ptr(), w.numel(), planes_.data_ptr(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return planes_


class _attached:
    """A pre-split image of prob.wd, attached for the block."""

    def __init__(self, lib, w):
        self.lib, self.w = lib, w

    def __enter__(self):
        from unified_audio_amd import _lib

        self.planes = _image(self.lib, self.w)
        _lib.check(self.lib.qa_weight_planes_attach(self.w.data_ptr(), self.w.numel(), self.planes.data_ptr()))
        return self.planes

    def __exit__(self, *exc):
        from unified_audio_amd import _lib

        torch.cuda.synchronize()
        _lib.check(self.lib.qa_weight_planes_detach(self.w.data_ptr()))
        return False


# ---------------------------------------------------------------------------------------------------------------------------------
# (1)

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("geo,path", PLAIN, ids=[f"{g}-{p}" for g, p in PLAIN])
def test_reduced_modes_match_fp64_of_the_rounded_operands(qa_lib, gpu_device, knob, geo, path, mode):
    G._pin_defaults(qa_lib, knob)
    prob = plain_problem(geo, path, gpu_device)
    for k, v in G.PATHS[path][0].items():
        knob(k, v)
    knob("QA_GEMM_MATH", mode)
    _check_rounded_parity(f"math{mode} {path} {geo}", prob.run(qa_lib), oracle(prob, PLANES_OF_MODE[mode]))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("tile", [2, 3])
@pytest.mark.parametrize("bk", ["bk16", "bk32"])
def test_reduced_modes_match_fp64_from_a_presplit_image(qa_lib, gpu_device, knob, tile, bk, mode):
    G._pin_defaults(qa_lib, knob)
    prob = plain_problem("ragged", "table_bk16", gpu_device, **IMAGE_GEO)
    ref = oracle(prob, PLANES_OF_MODE[mode])
    knob("QA_GEMM_CFG", tile)
    knob(*(("QA_GEMM_BK16_MIN_TILES", 0) if bk == "bk16" else ("QA_GEMM_BK16", 0)))
    knob("QA_GEMM_MATH", mode)
    with _attached(qa_lib, prob.wd) as image:
        knob("QA_GEMM_PRESPLIT", 1)
        used, launches = G._profiled(qa_lib, lambda: prob.run(qa_lib).clone())
        assert launches == [int(i == tile) for i in range(6)], launches
        knob("QA_GEMM_PRESPLIT", 0)
        ignored = prob.run(qa_lib).clone()
        knob("QA_GEMM_PRESPLIT", 1)
        # only the kept planes are read: garbage in the others changes nothing; a zeroed image shows that the launch reads the rest
        n = PLANES_OF_MODE[mode]
        image.view(-1, 3, 16)[:, n:, :] = 0xFF
        garbage_in_unused = prob.run(qa_lib).clone()
        image.fill_(0)
        poisoned = prob.run(qa_lib).clone()
    _check_rounded_parity(f"math{mode} cfg{tile} {bk} image", used, ref)
    _check_rounded_parity(f"math{mode} cfg{tile} {bk} image ignored", ignored, ref)
    assert torch.equal(used, ignored), "the image path and the in-loop split differ"
    assert torch.equal(garbage_in_unused, used), "the launch read a plane its mode does not keep"
    assert not torch.equal(poisoned, used), "the launch did not read the attached image"


# ---------------------------------------------------------------------------------------------------------------------------------
# (2)

ELU_GEOS = ("ragged", "k9", "k16", "in_rep3", "ssl_pos")


@functools.lru_cache(maxsize=None)
def _elu_problem(geo, dev, signed):
    prob = G.Problem({**_linear_epilogue(G.GEOS[geo]), "prologue": 1}, dev, zlib.crc32(f"modes-elu/{geo}".encode()))
    if not signed:
        prob.x = prob.x.abs()
        prob.xd.copy_(prob.x.to(dev))
    return prob


@functools.lru_cache(maxsize=None)
def _elu_signed_reference(prob):
    kw = dict(gamma=prob.gamma, residual=prob.res)
    y64, scale = conv_ref(prob.x, prob.w, prob.bias, prob.c, torch.float64, **kw)
    y32, _ = conv_ref(prob.x, prob.w, prob.bias, prob.c, torch.float32, **kw)
    plain = {**prob.c, "prologue": 0}
    mag, _ = conv_ref(prob.x.abs(), prob.w.abs(), None, plain, torch.float64, gamma=None if prob.gamma is None else prob.gamma.abs())
    return y64, scale, scaled_err(y32, y64, scale), mag


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("geo", ELU_GEOS)
def test_elu_prologue_of_non_negative_inputs_matches_the_rounded_operands(qa_lib, gpu_device, knob, geo, mode):
    G._pin_defaults(qa_lib, knob)
    prob = _elu_problem(geo, gpu_device, False)
    ref = _oracle_of(prob.x, prob.w, _Plain(prob), PLANES_OF_MODE[mode])
    knob("QA_GEMM_MATH", mode)
    _check_rounded_parity(f"math{mode} elu(x >= 0) {geo}", prob.run(qa_lib), ref)


class _Plain:
    """prob without its ELU prologue: the identity on the non-negative inputs, for the oracle of (1)."""

    def __init__(self, prob):
        self.bias, self.gamma, self.res, self.gate = prob.bias, prob.gamma, prob.res, None
        self.c = {**prob.c, "prologue": 0}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("geo", ELU_GEOS)
def test_elu_prologue_of_signed_inputs_is_within_the_operand_rounding(qa_lib, gpu_device, knob, geo, mode):
    G._pin_defaults(qa_lib, knob)
    prob = _elu_problem(geo, gpu_device, True)
    y64, scale, e32, mag = _elu_signed_reference(prob)
    u = UNIT[PLANES_OF_MODE[mode]]
    knob("QA_GEMM_MATH", mode)
    y = prob.run(qa_lib).cpu().double()
    parity = G.C_PARITY * max(e32, G.E_FLOOR)
    rounding = (2 * u + u * u) * mag
    e = float((((y - y64).abs() - rounding).clamp_min(0) / (scale + 1e-30)).max())
    print(f"modes elu signed math{mode} {geo}: raw e {scaled_err(y, y64, scale):.3e}, operand rounding allows up to "
          f"{float((rounding / (scale + 1e-30)).max()):.3e}, beyond it {e:.3e}, parity bound {parity:.3e}")
    assert e <= parity, f"math {mode} {geo}: {e:.3e} beyond the operand rounding, bound {parity:.3e}"


# ---------------------------------------------------------------------------------------------------------------------------------
# (3)

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("geo,variant", G.INVARIANCE, ids=[f"{g}-{v}" for g, v in G.INVARIANCE])
def test_reduced_modes_are_bit_identical_over_every_knob(qa_lib, gpu_device, knob, geo, variant, mode):
    from unified_audio_amd import _lib

    G._pin_defaults(qa_lib, knob)
    prob, _ = G._small(geo, variant, gpu_device)
    knob("QA_GEMM_MATH", mode)
    knob("QA_GEMM_PRESPLIT", 1)
    base = prob.run(qa_lib).clone()  # no image attached: the in-loop split under the cost model's launch
    knob("QA_GEMM_MATH", 1)
    assert not torch.equal(prob.run(qa_lib), base), "the mode computed the bits of split-6"
    knob("QA_GEMM_MATH", mode)
    settings = []
    for tile in (-1, 0, 1, 2, 3, 4, 5):
        settings += [{"QA_GEMM_CFG": tile, "QA_GEMM_LINEAR": lin, bk: v} for lin in (0, 1)
                     for bk, v in (("QA_GEMM_BK16", 0), ("QA_GEMM_BK16_MIN_TILES", 0))]
        settings += [{"QA_GEMM_CFG": tile, "QA_GEMM_XCD": x, "QA_GEMM_PANEL": pw} for x in (0, 1) for pw in (0, 1, 2, 3, 8, 1 << 20)]
        settings += [{"QA_GEMM_CFG": tile, "QA_GEMM_PRESPLIT": 0}, {"QA_GEMM_CFG": tile, "QA_GEMM_PRESPLIT": 0, "QA_GEMM_BK16_MIN_TILES": 0}]
    defaults = {n: _lib.get_knob(n) for n in G.GEMM_KNOBS + ("QA_GEMM_PRESPLIT",)}
    wide = 0
    with _attached(qa_lib, prob.wd):
        for s in settings:
            for k, v in {**defaults, **s}.items():
                knob(k, v)
            y, launches = G._profiled(qa_lib, lambda: prob.run(qa_lib))
            cfg = launches.index(1)
            wide += G.TILES[cfg][1] == 128 and s.get("QA_GEMM_PRESPLIT", 1) == 1
            assert torch.equal(y, base), f"math {mode}: {s} (ran {G.TILES[cfg]}) differs from the default launch"
        assert wide > 0, "no launch read the image"
        for k, v in defaults.items():
            knob(k, v)
        B = prob.c["B"]
        if B > 1:  # a batch split in two calls
            cut = (B + 1) // 2
            parts = torch.cat([prob.run(qa_lib, slice(0, cut)), prob.run(qa_lib, slice(cut, B))])
            assert torch.equal(parts, base), f"math {mode}: the batch in two calls differs from one call"


# ---------------------------------------------------------------------------------------------------------------------------------
# (4)

def _with_operands(geo, path, dev, nx, nw):
    """A fresh (geo, path) problem whose x / w are rounded to nx / nw planes, on the host and on the device."""
    c = _linear_epilogue({**G.GEOS[geo], **G.PATHS[path][1]})
    prob = G.Problem(c, dev, zlib.crc32(f"modes-exact/{geo}/{path}".encode()))
    prob.x, prob.w = rounded(prob.x, nx), rounded(prob.w, nw)
    prob.xd.copy_(prob.x.to(dev))
    prob.wd = prob.w.to(dev)
    return prob


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("geo,path", [("ragged", "table_bk16"), ("ragged", "linear_bk16"), ("k9", "cin48"), ("ssl_pos", "table_bk32")])
def test_a_reduced_mode_equals_split6_on_operands_it_represents_exactly(qa_lib, gpu_device, knob, geo, path, mode):
    G._pin_defaults(qa_lib, knob)
    for k, v in G.PATHS[path][0].items():
        knob(k, v)
    # mode 3: both operands bf16.  Mode 2: one operand of two planes against a bf16 one, either way round - with m != 0 in BOTH operands
    # split-6 also issues mm, which split-3 drops, so "l = 0 in both" alone does not make the two equal
    for nx, nw in ((1, 1),) if mode == 3 else ((2, 1), (1, 2)):
        prob = _with_operands(geo, path, gpu_device, nx, nw)
        out = {}
        for math in (1, mode):
            knob("QA_GEMM_MATH", math)
            out[math] = prob.run(qa_lib).clone()
        assert torch.equal(out[mode], out[1]), f"math {mode} differs from split-6 on operands of {nx} / {nw} plane(s)"
    # ... and not on operands that have more planes (the full-precision problem)
    full = plain_problem(geo, path, gpu_device)
    knob("QA_GEMM_MATH", 1)
    y1 = full.run(qa_lib).clone()
    knob("QA_GEMM_MATH", mode)
    assert not torch.equal(full.run(qa_lib), y1)


def test_fp32_and_split6_are_untouched_by_a_reduced_launch_in_between(qa_lib, gpu_device, knob):
    G._pin_defaults(qa_lib, knob)
    prob, _ = G._small("k16", "table_bk32", gpu_device)
    before = {}
    for math in (0, 1):
        knob("QA_GEMM_MATH", math)
        before[math] = prob.run(qa_lib).clone()
    for mode in MODES:
        knob("QA_GEMM_MATH", mode)
        prob.run(qa_lib)
        for math in (0, 1):
            knob("QA_GEMM_MATH", math)
            assert torch.equal(prob.run(qa_lib), before[math]), f"math {math} changed after a math {mode} launch"
    knob("QA_GEMM_MATH", 7)  # any other value: split-6
    assert torch.equal(prob.run(qa_lib), before[1])


# ---------------------------------------------------------------------------------------------------------------------------------
# (5)

def _run(lib, x, w, b):
    return conv1d_cl(lib, x.unsqueeze(0), w.unsqueeze(1), b)[0]


@pytest.mark.parametrize("mode", MODES)
def test_non_finite_inputs_follow_fp64(qa_lib, gpu_device, knob, mode):
    g = torch.Generator().manual_seed(11)
    M, N, K = 300, 136, 96
    x = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) * 0.1
    x[3, 5] = float("inf")
    x[7, 40] = float("-inf")
    x[9, 17] = float("nan")
    x[11, 2], x[11, 70] = float("inf"), float("-inf")  # inf - inf in one row: NaN
    w[20, 33] = float("inf")
    w[21, 90] = float("nan")
    knob("QA_GEMM_MATH", mode)
    y = _run(qa_lib, x.to(gpu_device), w.to(gpu_device), torch.zeros(N, device=gpu_device)).cpu()
    ref = x.double() @ w.double().t()
    assert torch.equal(torch.isfinite(y), torch.isfinite(ref)), f"math {mode}: non-finite pattern differs from fp64"
    assert torch.isnan(y[torch.isnan(ref)]).all(), f"math {mode}: a NaN of fp64 is not NaN"
    inf = torch.isinf(ref)
    if mode == 3:  # one plane: no lower plane to meet an inf with a zero
        assert torch.equal(y[inf], ref[inf].float())
    else:
        assert (torch.isnan(y[inf]) | (y[inf] == ref[inf].float())).all()


class _Case:
    """The fields _oracle_of reads, for operands that are not a G.Problem."""

    def __init__(self, bias, case):
        self.bias, self.c, self.gamma, self.res, self.gate = bias, case, None, None, None


@pytest.mark.parametrize("mode", MODES)
def test_cancellation_inside_a_k_group(qa_lib, gpu_device, knob, mode):
    g = torch.Generator().manual_seed(5)
    M, N, K = 130, 72, 64
    x = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) * 0.1
    w[:, 0] = w[:, 5] = w[:, 2] = w[:, 14] = 32768.0
    w[:, 3] = w[:, 9] = 1.0
    x[0] = 0.0
    x[0, 0], x[0, 3], x[0, 5] = 32768.0, 1.5, -32768.0
    x[1] = 0.0
    x[1, 2], x[1, 9], x[1, 14] = 32768.0, 1.5, -32768.0
    v = 1.0 + 2.0 ** -23 + 2.0 ** -15  # h = 1, m = 2^-15, l = 2^-23: v - v cancels in every plane
    x[2] = 0.0
    x[2, 16], x[2, 17], x[2, 40] = v, -v, 2.0 ** -20
    w[:, 16] = w[:, 17] = w[:, 40] = 1.0
    case = dict(stride=1, pad=(0, 0), pad_mode=0, prologue=0, in_rep=1, act=0, post=0, T_out=M)
    x3, w3, b = x.unsqueeze(0), w.unsqueeze(1), torch.zeros(N)
    ref = _oracle_of(x3, w3, _Case(b, case), PLANES_OF_MODE[mode])
    knob("QA_GEMM_MATH", mode)
    y = conv1d_cl(qa_lib, x3.to(gpu_device), w3.to(gpu_device), b.to(gpu_device)).cpu()
    _check_rounded_parity(f"math{mode} cancellation", y.reshape(-1, N), ref)
    assert torch.all(y[0, 2] == 2.0 ** -20), f"math {mode}: {y[0, 2, :4].tolist()}"


@pytest.mark.parametrize("mode", MODES)
def test_wide_dynamic_range_matches_fp64_of_the_rounded_operands(qa_lib, gpu_device, knob, mode):
    g = torch.Generator().manual_seed(1)
    B, T, C, N = 2, 257, 128, 200
    x = torch.randn(B, T, C, generator=g) * torch.exp2(torch.randint(-40, 41, (B, T, C), generator=g).float())
    w = torch.randn(N, 1, C, generator=g) * torch.exp2(torch.randint(-20, 21, (N, 1, C), generator=g).float())
    b = torch.randn(N, generator=g)
    case = dict(stride=1, pad=(0, 0), pad_mode=0, prologue=0, in_rep=1, act=0, post=0, T_out=T)
    ref = _oracle_of(x, w, _Case(b, case), PLANES_OF_MODE[mode])
    knob("QA_GEMM_MATH", mode)
    y = conv1d_cl(qa_lib, x.to(gpu_device), w.to(gpu_device), b.to(gpu_device)).cpu()
    _check_rounded_parity(f"math{mode} wide range", y.reshape(-1, N), ref)
