"""The reduced conv_gemm arithmetics (QA_GEMM_MATH = 2 split-3, 3 bf16) on the host: the plane split the GPU tests build their oracles
from (tests/gemm_modes_ref.py), the power of those GPU tests, and the Python helper unified_audio_amd.gemm_math.

(a) seeded fp32 data over 2^-40 .. 2^40: h + m + l == x exactly, |x - h| <= 2^-8 |x|, |x - h - m| <= 2^-16 |x|;
(b) power: on the first problem of tests/test_conv_gemm_modes_gpu.py the fp64 result of the bf16-rounded operands is at least 100 parity
    bounds away from the fp64 result of the true operands (tests/util.scaled_err) - a mode-3 kernel that silently ran split-6 would be
    that far from the oracle the GPU test holds it to, and could not pass; the gap of mode 2 (2^-8 of that) is printed;
(c) gemm_math: names and integers, restore on exit and on exception, ValueError for an unknown name before the library is touched.
    The library loads without a device.
"""
import pytest
import torch

from tests import test_conv_gemm_gpu as G
from tests.gemm_modes_ref import UNIT, planes, rounded
from tests.test_conv_gemm_modes_gpu import PLAIN, oracle, plain_problem
from tests.util import conv_ref, scaled_err


def _wide(seed, n=1 << 16):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, generator=g) * torch.exp2(torch.randint(-40, 41, (n,), generator=g).float())


# (a)
@pytest.mark.parametrize("seed", [1, 2])
def test_three_planes_are_exact_and_each_plane_gains_eight_bits(seed):
    x = _wide(seed)
    h, m, l = (p.double() for p in planes(x, 3))
    xd = x.double()
    assert torch.equal(h + m + l, xd)
    assert torch.all((xd - h).abs() <= UNIT[1] * xd.abs())
    assert torch.all((xd - h - m).abs() <= UNIT[2] * xd.abs())
    assert torch.equal(rounded(x, 3), x) and torch.equal(rounded(x, 2).double(), h + m) and torch.equal(rounded(x, 1).double(), h)
    assert not torch.equal(rounded(x, 2), x) and not torch.equal(rounded(x, 1), rounded(x, 2))


def test_non_finite_values_keep_their_meaning():
    x = torch.tensor([float("inf"), float("-inf"), float("nan"), 3.4e38, -3.4e38, 1.0, 0.0])
    h, m, l = planes(x, 3)
    assert torch.equal(h[:2], x[:2]) and torch.isnan(h[2]) and torch.isinf(h[3]) and torch.isinf(h[4])  # 3.4e38 rounds to bf16 inf
    assert torch.all(m[:5] == 0) and torch.all(l[:5] == 0)
    assert h[5] == 1 and m[5] == 0 and h[6] == 0


# (b)
def test_rounded_operands_are_far_from_the_true_ones_on_the_first_gpu_problem():
    geo, path = PLAIN[0]
    prob = plain_problem(geo, path, torch.device("cpu"))
    kw = dict(gamma=prob.gamma, residual=prob.res, gate=prob.gate)
    y_true, scale = conv_ref(prob.x, prob.w, prob.bias, prob.c, torch.float64, **kw)
    for mode, n in ((3, 1), (2, 2)):
        y_n, scale_n, e32 = oracle(prob, n)[:3]
        bound = G.C_PARITY * max(e32, G.E_FLOOR)
        gap = scaled_err(y_n, y_true, scale)
        print(f"mode {mode} {geo}/{path}: rounded-operand oracle is {gap:.3e} from the true operands' result = {gap / bound:.0f} parity bounds ({bound:.3e})")
        if mode == 3:
            assert gap >= 100.0 * bound, f"the oracle is only {gap / bound:.1f} parity bounds from the true operands' result"


# (c)
def test_gemm_math_names_restore_and_errors(qa_lib):
    import unified_audio_amd as qa
    from unified_audio_amd import _lib

    start = _lib.get_knob("QA_GEMM_MATH")
    try:
        for name, value in (("fp32", 0), ("split6", 1), ("split3", 2), ("bf16", 3)):
            for mode in (name, value):
                with qa.gemm_math(mode):
                    assert _lib.get_knob("QA_GEMM_MATH") == value and qa.gemm_math_name() == name
                assert _lib.get_knob("QA_GEMM_MATH") == start
        with qa.gemm_math("split3"):
            with qa.gemm_math("bf16"):
                assert qa.gemm_math_name() == "bf16"
            assert qa.gemm_math_name() == "split3"
        with pytest.raises(RuntimeError, match="boom"):
            with qa.gemm_math("bf16"):
                raise RuntimeError("boom")
        assert _lib.get_knob("QA_GEMM_MATH") == start
        # the plain setter returns the previous value and stays
        assert qa.set_gemm_math("split3") == start and qa.gemm_math_name() == "split3"
        assert qa.set_gemm_math(start) == 2
        for bad in ("fp16", "", "SPLIT3", 4, -1, 2.0, True, None):
            with pytest.raises(ValueError):
                qa.gemm_math(bad)
            with pytest.raises(ValueError):
                qa.set_gemm_math(bad)
            assert _lib.get_knob("QA_GEMM_MATH") == start
        _lib.set_knob("QA_GEMM_MATH", 7)  # a value the library does not name runs split-6
        assert qa.gemm_math_name() == "split6"
    finally:
        _lib.set_knob("QA_GEMM_MATH", start)


def test_an_unknown_name_raises_before_the_library_is_touched(monkeypatch):
    from unified_audio_amd import _lib

    def no_library():
        raise AssertionError("the library was touched")

    monkeypatch.setattr(_lib, "load_library", no_library)
    with pytest.raises(ValueError):
        _lib.gemm_math("fp8")
    with pytest.raises(ValueError):
        _lib.set_gemm_math("fp8")
    _lib.gemm_math("bf16")  # constructing a valid one does not touch it either: the knob is set on entry
