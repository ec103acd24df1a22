"""conv_gemm's split forms on the 16 x 16 x 32 bf16 MFMA: 32-wide k groups, one ds_read_b128 per 16-row fragment, 16 x 16 accumulators,
and the zero-filled upper half of the last group when K = 16 mod 32.  Through qa_conv1d_cl, like tests/test_conv_gemm_gpu.py, on the
smallest shapes that cross every edge: M in {1, 17, 33, 130}, N in {4, 20, 21 (scalar epilogue), 132}, K in {16, 32, 48, 96}, Linear
layers and ksize-3 convolutions of 16 and 32 channels, every forced tile (QA_GEMM_CFG 0 .. 5), both chunk forms (one and two LDS buffers:
QA_GEMM_BK16_MIN_TILES = 0 / QA_GEMM_BK16 = 0), weights split in the loop and read from a pre-split image.

(1) one-hot exactness: x[m, k] = (k == k0) against random fp32 weights gives y[m, n] == w[n, k0] bit for bit - 1 = h, so the products hl,
    hm, hh are the three planes of w and sum to w exactly - for every k0 (one clip per k0); and the same with the roles swapped (one-hot
    weight rows, shifted until every k0 has been a row's).  A wrong lane, slot, swizzle, plane or row / column map fails at its k0.
(2) K = 16 and 48: an inf in x and one in w leave exactly the outputs non-finite that fp64 leaves non-finite - the missing upper half of
    the last group is zero in both operands, whatever lies behind the operands in memory (here: more infs).
(3) fp64 parity of random problems under the bound of tests/test_conv_gemm_gpu.py, C_PARITY * max(e_cpu32, E_FLOOR); largest e per K printed
    (pytest -s).  Measured on MI355X: 6.8e-8 (K = 16), 4.5e-8 (32), 1.3e-7 (48), 1.5e-7 (96); bounds >= 6.0e-7.
(4) K = 48 and 96 at M = 130, N = 132: every tile, chunk form and weight source gives the same bits.
(5) QA_GEMM_MATH = 2 and 3 on the K = 48 shape: the rounded-operand bounds of tests/test_conv_gemm_modes_gpu.py.
"""
import functools

import pytest
import torch

from tests import test_conv_gemm_gpu as G
from tests import test_conv_gemm_modes_gpu as MD
from tests.util import conv1d_cl, scaled_err

pytestmark = pytest.mark.gpu

CHUNK_FORMS = ({"QA_GEMM_BK16_MIN_TILES": 0}, {"QA_GEMM_BK16": 0})  # one LDS buffer of 32 k; two
# (M, N, C_in, ksize): K = ksize * C_in.  ksize 3 runs with stride 3, so that the im2col rows are disjoint frames
SHAPES = [(1, 4, 16, 1), (17, 20, 32, 1), (33, 21, 48, 1), (130, 132, 96, 1), (130, 132, 48, 1), (17, 132, 16, 1), (130, 4, 96, 1),
          (33, 20, 16, 3), (17, 21, 16, 3), (130, 132, 32, 3), (1, 132, 32, 3)]
IDS = [f"{m}x{n}x{k * c}-k{k}" for m, n, c, k in SHAPES]


def _configs(knob, lib):
    """Every (tile, chunk form, weight source) in turn: yields its label with the knobs set."""
    for tile in G.TILES:
        for form in CHUNK_FORMS:
            for presplit in (1, 0):
                G._pin_defaults(lib, knob)
                knob("QA_GEMM_CFG", tile)
                for k, v in form.items():
                    knob(k, v)
                knob("QA_GEMM_PRESPLIT", presplit)
                yield f"cfg{tile} {'one' if 'QA_GEMM_BK16_MIN_TILES' in form else 'two'} buffer(s) {'image' if presplit else 'loop'}"


def _conv(lib, x, w, ksize):
    return conv1d_cl(lib, x, w, None, stride=ksize)


@pytest.mark.parametrize("M,N,Cin,ksize", SHAPES, ids=IDS)
def test_one_hot_operands_are_exact(qa_lib, gpu_device, knob, M, N, Cin, ksize):
    K = ksize * Cin
    g = torch.Generator().manual_seed(1000 * M + N + K)
    # clip k0: every im2col row is the unit vector e_k0 (k = tap * C_in + channel; frames t * ksize + tap with stride = ksize)
    x = torch.zeros(K, M * ksize, Cin)
    for k0 in range(K):
        x[k0, k0 // Cin::ksize, k0 % Cin] = 1.0
    w = torch.randn(N, ksize, Cin, generator=g)
    xr = torch.randn(1, M * ksize, Cin, generator=g)
    want_x = w.reshape(N, K).t()[:, None, :].expand(K, M, N).contiguous()  # y[k0, m, n] = w[n, k0]
    cols = xr.reshape(M, K)
    xd, wd, xrd = x.to(gpu_device), w.to(gpu_device), xr.to(gpu_device)
    shifts = range(0, K, N)
    hot = []
    for s in shifts:  # row n of the weight is e_((n + s) % K)
        wh = torch.zeros(N, K)
        wh[torch.arange(N), (torch.arange(N) + s) % K] = 1.0
        hot.append(wh.reshape(N, ksize, Cin).to(gpu_device))
    for label in _configs(knob, qa_lib):
        with MD._attached(qa_lib, wd):
            y = _conv(qa_lib, xd, wd, ksize).cpu()
        bad = (y != want_x).nonzero()
        assert bad.numel() == 0, f"{label}: one-hot activations, first wrong (k0, m, n) = {bad[0].tolist()} of {bad.shape[0]}"
        for s, wh in zip(shifts, hot):
            with MD._attached(qa_lib, wh):
                y = _conv(qa_lib, xrd, wh, ksize).cpu()[0]
            want = cols[:, (torch.arange(N) + s) % K]
            bad = (y != want).nonzero()
            assert bad.numel() == 0, f"{label}: one-hot weights shifted by {s}, first wrong (m, n) = {bad[0].tolist()} of {bad.shape[0]}"


@pytest.mark.parametrize("K", [16, 48])
@pytest.mark.parametrize("where", ["row0_col0", "behind"])
def test_half_group_is_zero_in_both_operands(qa_lib, gpu_device, knob, K, where):
    M, N = 33, 20
    g = torch.Generator().manual_seed(K)
    x = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g)
    if where == "row0_col0":
        x[0, K - 1] = float("inf")
        w[0, K - 1] = float("-inf")
    else:  # the floats right behind row 0 / weight row 0 - what a 32-wide read of their last group would meet
        x[1, 0] = float("inf")
        w[1, 0] = float("inf")
    ref = x.double() @ w.double().t()
    # the activations lie in rows of K + 16 floats whose tails hold inf, and 16 more infs follow the weight: a group that read past K
    # in one operand only would turn 0 x inf into NaN
    buf = torch.full((M + 1, K + 16), float("inf"))
    buf[:M, :K] = x
    xd = buf.to(gpu_device)[:M, :K].unsqueeze(0)
    wbuf = torch.full((N * K + 16,), float("inf"))
    wbuf[:N * K] = w.reshape(-1)
    wd = wbuf.to(gpu_device)[:N * K].view(N, 1, K)
    for label in _configs(knob, qa_lib):
        with MD._attached(qa_lib, wd):
            y = conv1d_cl(qa_lib, xd, wd, None).cpu()[0]
        assert torch.equal(torch.isfinite(y), torch.isfinite(ref)), \
            f"{label}: finite pattern differs from fp64 at (m, n) = {(torch.isfinite(y) != torch.isfinite(ref)).nonzero()[:4].tolist()}"


@functools.lru_cache(maxsize=None)
def _random_problem(M, N, Cin, ksize, dev):
    c = dict(B=1, T=M * ksize, Cin=Cin, N=N, k=ksize, stride=ksize)
    p = G.Problem(c, dev, 7000 + 1000 * M + N + ksize * Cin)
    return p, p.references()


E_MAX = {}  # K -> largest e of (3) in this session


@pytest.mark.parametrize("M,N,Cin,ksize", SHAPES, ids=IDS)
def test_fp64_parity(qa_lib, gpu_device, knob, M, N, Cin, ksize):
    prob, ref = _random_problem(M, N, Cin, ksize, gpu_device)
    for label in _configs(knob, qa_lib):
        with MD._attached(qa_lib, prob.wd):
            y = prob.run(qa_lib)
        y64, scale, e32 = ref
        e = scaled_err(y.cpu(), y64, scale)
        E_MAX[ksize * Cin] = max(E_MAX.get(ksize * Cin, 0.0), e)
        bound = G.C_PARITY * max(e32, G.E_FLOOR)
        assert e <= bound, f"{label}: {e:.3e} from the fp64 truth, bound {bound:.3e} (fp32 CPU {e32:.3e})"
    print(f"mfma shape parity {M}x{N}x{ksize * Cin}: largest e per K so far " + ", ".join(f"K={k}: {v:.3e}" for k, v in sorted(E_MAX.items())))


@pytest.mark.parametrize("Cin,ksize", [(48, 1), (96, 1), (16, 3), (32, 3)], ids=["K48", "K96", "K48-k3", "K96-k3"])
def test_same_bits_in_every_instance(qa_lib, gpu_device, knob, Cin, ksize):
    prob, _ = _random_problem(130, 132, Cin, ksize, gpu_device)
    first = None
    for label in _configs(knob, qa_lib):
        with MD._attached(qa_lib, prob.wd):
            y = prob.run(qa_lib).clone()
        if first is None:
            first = (label, y)
        assert torch.equal(y, first[1]), f"{label} differs from {first[0]} in {int((y != first[1]).sum())} elements"


@pytest.mark.parametrize("mode", MD.MODES)
def test_reduced_forms_meet_their_bounds(qa_lib, gpu_device, knob, mode):
    prob = MD.plain_problem("ragged", "cin48", gpu_device, B=1, T=130, N=132)  # 130 x 132 x 48, linear epilogue
    ref = MD.oracle(prob, MD.PLANES_OF_MODE[mode])
    for label in _configs(knob, qa_lib):
        knob("QA_GEMM_MATH", mode)
        with MD._attached(qa_lib, prob.wd):
            y = prob.run(qa_lib)
        MD._check_rounded_parity(f"mode {mode} {label}", y, ref)
