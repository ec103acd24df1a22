"""conv_gemm's two arithmetics (QA_GEMM_MATH): split-6 (the default: each operand split into three bf16 planes, six
v_mfma_f32_32x32x16_bf16 per 16-wide k group, one fp32 accumulator) and the fp32 chain (v_mfma_f32_32x32x2_f32).

tests/test_conv_gemm_gpu.py runs at the library's default, i.e. it checks split-6: fp64 parity of every legal (tile, path,
geometry) and of the headline's own layers, and bit-identity over every tile, BK, LINEAR, XCD and panel setting and over batch
splits.  Here:
(a) the fp32 chain keeps both properties: the parity and invariance tests of that file, run under QA_GEMM_MATH = 0;
(b) split-6 against fp64 and against the fp32 chain on the same problems: both inside the bound of tests/test_conv_gemm_gpu.py
    (C_PARITY * max(e_cpu32, E_FLOOR), tests/util.scaled_err); each check prints its e (pytest -s).  Both passed on MI355X; the
    per-case e range of split-6 has not been recorded yet;
(c) non-finite inputs: inf and NaN in activations or weights leave exactly the outputs non-finite that fp64 leaves non-finite
    (h = inf, m = l = 0: no inf - inf inside the split); fp64's NaNs are NaN; an inf of the fp32 chain may come out NaN under
    split-6 (inf times a zero lower plane of the other operand);
(d) wide dynamic range: products 2^30, 1.5 and -2^30 inside one 8-wide and across one 16-wide k group, an exact cancellation
    of a full 24-bit significand, and operands spread over 2^-40 .. 2^40: within the parity bound, for both arithmetics.
"""
import functools

import pytest
import torch

from tests import test_conv_gemm_gpu as G
from tests.util import conv1d_cl, conv_ref, scaled_err

pytestmark = pytest.mark.gpu


def _rerun_under_fp32_chain(fn):
    """fn of tests/test_conv_gemm_gpu.py with its parametrisation, run with QA_GEMM_MATH = 0."""

    @functools.wraps(fn)
    def test(qa_lib, gpu_device, knob, **kw):
        knob("QA_GEMM_MATH", 0)
        fn(qa_lib, gpu_device, knob, **kw)

    test.pytestmark = []  # functools.wraps shares fn's mark list; the parametrisation is applied afresh below
    for m in getattr(fn, "pytestmark", []):
        if m.name == "parametrize":
            test = pytest.mark.parametrize(*m.args, **m.kwargs)(test)
    return test


# (a)
test_fp32_chain_instantiation_matches_fp64 = _rerun_under_fp32_chain(G.test_conv_gemm_instantiation_matches_fp64)
test_fp32_chain_knobs_are_bit_identical = _rerun_under_fp32_chain(G.test_conv_gemm_knobs_are_bit_identical)


# (b)
@pytest.mark.parametrize("geo", ["ragged", "k9", "k16", "in_rep3", "ssl_pos"])
@pytest.mark.parametrize("path", ["table_bk16", "linear_bk16", "elu", "cin48"])
def test_split6_and_fp32_chain_both_match_fp64(qa_lib, gpu_device, knob, geo, path):
    G._pin_defaults(qa_lib, knob)
    prob, ref = G._small(geo, path, gpu_device)
    for k, v in G.PATHS[path][0].items():
        knob(k, v)
    out = {}
    for math in (0, 1):
        knob("QA_GEMM_MATH", math)
        out[math] = prob.run(qa_lib).clone()
        G._check_parity(f"math{math} {path} {geo}", out[math], ref)


def _run(lib, x, w, b):
    return conv1d_cl(lib, x.unsqueeze(0), w.unsqueeze(1), b)[0]


# (c)
def test_split6_non_finite_inputs_follow_the_fp32_chain(qa_lib, gpu_device, knob):
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
    xd, wd, bd = x.to(gpu_device), w.to(gpu_device), torch.zeros(N, device=gpu_device)
    out = {}
    for math in (0, 1):
        knob("QA_GEMM_MATH", math)
        out[math] = _run(qa_lib, xd, wd, bd).cpu()
    ref = x.double() @ w.double().t()
    for math in (0, 1):
        y = out[math]
        assert torch.equal(torch.isfinite(y), torch.isfinite(ref)), f"math {math}: non-finite pattern differs from fp64"
        assert torch.isnan(y[torch.isnan(ref)]).all(), f"math {math}: a NaN of fp64 is not NaN"
    inf = torch.isinf(ref)
    assert torch.equal(out[0][inf], ref[inf].float()), "fp32 chain: an inf of fp64 is not the same inf"
    # split-6: an inf operand meets the other operand's lower planes, and a plane that is 0 gives inf * 0 = NaN - the inf outputs of
    # the fp32 chain come out as inf or NaN, never finite
    assert (torch.isnan(out[1][inf]) | (out[1][inf] == ref[inf].float())).all()


# (d)
def test_split6_cancellation_inside_a_k_group(qa_lib, gpu_device, knob):
    g = torch.Generator().manual_seed(5)
    M, N, K = 130, 72, 64
    x = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) * 0.1
    # rows 0 / 1: products 2^30, 1.5, -2^30 inside one 8-wide group (k 0, 3, 5) and across the halves of a 16-wide group (k 2, 9, 14)
    w[:, 0] = w[:, 5] = w[:, 2] = w[:, 14] = 32768.0
    w[:, 3] = w[:, 9] = 1.0
    x[0] = 0.0
    x[0, 0], x[0, 3], x[0, 5] = 32768.0, 1.5, -32768.0
    x[1] = 0.0
    x[1, 2], x[1, 9], x[1, 14] = 32768.0, 1.5, -32768.0
    # row 2: a 24-bit significand against its own negation plus a tiny term: exact in every order (2^-20)
    v = 1.0 + 2.0 ** -23 + 2.0 ** -15
    x[2] = 0.0
    x[2, 16], x[2, 17], x[2, 40] = v, -v, 2.0 ** -20
    w[:, 16] = w[:, 17] = w[:, 40] = 1.0
    case = dict(stride=1, pad=(0, 0), pad_mode=0, prologue=0, in_rep=1, act=0, post=0, T_out=M)
    x3, w3, b = x.unsqueeze(0), w.unsqueeze(1), torch.zeros(N)
    y64, scale = conv_ref(x3, w3, b, case)
    y32, _ = conv_ref(x3, w3, b, case, dtype=torch.float32)
    bound = G.C_PARITY * max(scaled_err(y32, y64, scale), G.E_FLOOR)
    for math in (0, 1):
        knob("QA_GEMM_MATH", math)
        y = conv1d_cl(qa_lib, x3.to(gpu_device), w3.to(gpu_device), b.to(gpu_device)).cpu()
        e = scaled_err(y.reshape(-1, N), y64, scale)
        assert e <= bound, f"math {math}: {e:.3e} from fp64, bound {bound:.3e}"
        assert torch.all(y[0, 2] == 2.0 ** -20), f"math {math}: {y[0, 2, :4].tolist()}"


@pytest.mark.parametrize("seed", [1, 2])
def test_split6_wide_dynamic_range_matches_fp64(qa_lib, gpu_device, knob, seed):
    g = torch.Generator().manual_seed(seed)
    B, T, C, N = 2, 257, 128, 200
    x = torch.randn(B, T, C, generator=g) * torch.exp2(torch.randint(-40, 41, (B, T, C), generator=g).float())
    w = torch.randn(N, 1, C, generator=g) * torch.exp2(torch.randint(-20, 21, (N, 1, C), generator=g).float())
    b = torch.randn(N, generator=g)
    case = dict(stride=1, pad=(0, 0), pad_mode=0, prologue=0, in_rep=1, act=0, post=0, T_out=T)
    y64, scale = conv_ref(x, w, b, case)
    y32, _ = conv_ref(x, w, b, case, dtype=torch.float32)
    e32 = scaled_err(y32, y64, scale)
    bound = G.C_PARITY * max(e32, G.E_FLOOR)
    for math in (0, 1):
        knob("QA_GEMM_MATH", math)
        y = conv1d_cl(qa_lib, x.to(gpu_device), w.to(gpu_device), b.to(gpu_device)).cpu()
        e = scaled_err(y.reshape(-1, N), y64, scale)
        print(f"wide range seed {seed} math {math}: e {e:.3e} e_cpu32 {e32:.3e} bound {bound:.3e}")
        assert e <= bound, f"math {math}: {e:.3e} from fp64, bound {bound:.3e}"
