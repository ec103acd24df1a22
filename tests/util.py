"""Shared helpers of the test-suite (oracle side on CPU, product side through the C-ABI)."""
from __future__ import annotations

import contextlib
import ctypes as C

import torch
import torch.nn.functional as F

from oracle.hcodec_ref import HCodecSpec as OracleSpec

# small architecture with the same block vocabulary as H-Codec 1.0 (channel ladder 32 -> 64 -> 128, hidden 16 in the
# first residual block like the real model) so that whole-graph parity runs in seconds on CPU
MINI = dict(n_filters=32, ratios=(2, 4), dimension=128, enc_heads=2, enc_layers=1, sem_in=64, sem_ch=64,
            sem_strides=(2, 1), code_dim=128, codebook_size=64, num_quantizers=3, dec_dim=128, dec_inter=256,
            dec_heads=4, dec_layers=1, convnext_layers=2, n_fft=32, hop=8, gn_groups=32)


def mini_oracle_spec() -> OracleSpec:
    return OracleSpec(**MINI)


def rel_err(a: torch.Tensor, b: torch.Tensor) -> float:
    """RMS(a - b) / RMS(b)."""
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt().clamp_min(1e-30))


def conv1d_cl(lib, x, w, bias=None, *, stride=1, pad=(0, 0), pad_mode=0, prologue=0, act=0, gamma=None, residual=None,
              gate=None, post_act=0, T_out=None, in_rep=1, ldx=None, ldy=None, ldr=None, ldg=None, y_offset=None, guard=False):
    """Call qa_conv1d_cl.  x [B,T,C] cuda, w [N,k,C] cuda (library layout).  Returns y [B,T_out,N].

    x, residual and gate may be strided views (see `strided_rows`): their row strides are passed as ldx / ldr / ldg (an explicit
    value must agree with the view).  With `guard` (implied by ldy or y_offset), y is a view with row stride ldy (default N), starting
    y_offset floats into a buffer whose every other element holds a sentinel (`guarded_out`); after the call every element of y must
    have been written and no sentinel may have changed, else AssertionError."""
    from unified_audio_amd import _lib

    B, T, Cin = x.shape
    N, k, _ = w.shape
    if T_out is None:
        T_out = (T * max(in_rep, 1) + pad[0] + pad[1] - k) // stride + 1
    ldx = _row_stride(x, ldx, T)
    ldr = _row_stride(residual, ldr, T_out) if residual is not None else N
    ldg = _row_stride(gate, ldg, T_out) if gate is not None else N
    guard = guard or ldy is not None or y_offset is not None
    if guard:
        buf, y = guarded_out(B * T_out, N, ldy or N, y_offset or 0, x.device)
        y = y.view(B, T_out, N)
    else:
        y = torch.full((B, T_out, N), float("nan"), device=x.device)
    a = _lib.qa_conv_args()
    a.x, a.w, a.y = x.data_ptr(), w.data_ptr(), y.data_ptr()
    a.bias = bias.data_ptr() if bias is not None else None
    a.gamma = gamma.data_ptr() if gamma is not None else None
    a.residual = residual.data_ptr() if residual is not None else None
    a.gate = gate.data_ptr() if gate is not None else None
    a.B, a.T_in, a.C_in, a.T_out, a.N = B, T, Cin, T_out, N
    a.ldx, a.ldy, a.ldr, a.ldg = ldx, y.stride(1), ldr, ldg
    a.ksize, a.stride, a.pad_left, a.pad_right, a.pad_mode = k, stride, pad[0], pad[1], pad_mode
    a.prologue, a.act, a.post_act = prologue, act, post_act
    a.in_rep = in_rep
    _lib.check(lib.qa_conv1d_cl(C.byref(a), torch.cuda.current_stream().cuda_stream))
    if guard:
        check_guarded_out(buf, y.view(B * T_out, N), y_offset or 0)
    return y


def _row_stride(t, ld, rows_per_item):
    """Row stride of a [B, rows, C] operand that the C-ABI reads as rows of `ld` floats (item b at b * rows * ld)."""
    ld = t.stride(1) if ld is None else ld
    assert t.stride(2) == 1 and t.stride(1) == ld and (t.shape[0] == 1 or t.stride(0) == rows_per_item * ld), (t.stride(), ld)
    return ld


def strided_rows(t, ld, offset=0, generator=None):
    """t [B, R, C] -> an equal view whose rows are `ld` floats apart, at column `offset` of each row: the other columns, and one
    row of slack after the last, hold other random numbers, so a kernel that reads outside the view gets a wrong answer
    but stays inside the allocation."""
    B, R, Cc = t.shape
    assert offset + Cc <= ld
    buf = torch.randn((B * R + 1) * ld, generator=generator).to(t.device)
    view = buf[:B * R * ld].view(B, R, ld)[..., offset:offset + Cc]
    view.copy_(t)
    return view


SENTINEL_BITS = 0x7F7ADEAD  # a finite float (~3.3e38) that no output of these tests comes near
GUARD_TAIL_ROWS = 256       # the tallest conv_gemm tile: a store that ignores the row mask lands here


def guarded_out(M, N, ldy, head, device):
    """(buffer, y): y [M, N] with row stride ldy starts `head` floats into the buffer and is NaN; the gap columns (ldy > N), the
    head and GUARD_TAIL_ROWS rows after the last hold SENTINEL_BITS."""
    assert ldy >= N
    buf = torch.empty(head + (M + GUARD_TAIL_ROWS) * ldy, dtype=torch.float32, device=device)
    buf.view(torch.int32).fill_(SENTINEL_BITS)
    y = buf[head:head + M * ldy].view(M, ldy)[:, :N]
    y.fill_(float("nan"))
    return buf, y


def check_guarded_out(buf, y, head):
    """Every element of y [M, N] was written, and nothing else in its buffer (guarded_out)."""
    M, N = y.shape
    ldy = y.stride(0)
    outside = torch.ones(buf.numel(), dtype=torch.bool, device=buf.device)
    outside[head:head + M * ldy].view(M, ldy)[:, :N] = False
    bits = buf.view(torch.int32)
    bad = int((bits[outside] != SENTINEL_BITS).sum())
    assert bad == 0, f"{bad} elements outside the [{M}, {N}] output (ldy {ldy}, offset {head}) were overwritten"
    unwritten = int(torch.isnan(y).sum())
    assert unwritten == 0, f"{unwritten} of the {M * N} output elements were never written"


@contextlib.contextmanager
def with_knob(name, value):
    """Set a library knob (unified_audio_amd._lib.set_knob) for the duration of a with block."""
    from unified_audio_amd import _lib

    old = _lib.set_knob(name, value)
    try:
        yield
    finally:
        _lib.set_knob(name, old)


def conv_ref(x, w, bias, case, dtype=torch.float64, *, gamma=None, residual=None, gate=None, rows=None):
    """Plain CPU restatement of qa_conv1d_cl in `dtype` (float64: the truth; float32: the yardstick), the op sequence of
    tests/test_kernels_gpu._ref_conv plus the epilogue: ELU prologue, repeat_interleave by in_rep, zero or reflect padding
    (the reference's pad1d, short-input rule included), windows . weights + bias, silu(gate) *, act, * gamma, + residual, post_act.

    x [B,T,C], w [N,k,C], gate / residual [B,T_out,N] (CPU, any strides); case: stride, pad (left, right), pad_mode (0 zero,
    1 reflect), prologue, in_rep, act, post (codes of conv1d_cl), T_out.  `rows`: the flat output rows (b * T_out + t) to compute,
    default all.  Returns (y [R, N], scale [R, N]) where scale = |g| |gamma| (sum_k |a_k w_k| + |b|) + |r| is the magnitude the
    rounding error of an fp32 evaluation is proportional to (a = the prologue'd im2col row, g = silu(gate)).  The library evaluates
    ELU(v) < 0 as exp(v) - 1 (csrc/common.h), whose rounding error is relative to exp(v), not to ELU(v): every ELU, prologue
    included, adds exp(v) for v < 0 to the scale of what it produces."""
    from oracle.hcodec_ref import _pad1d_reflect

    B, T, Cin = x.shape
    N, k, _ = w.shape
    stride, (pl, pr) = case.get("stride", 1), case.get("pad", (0, 0))
    rep = max(case.get("in_rep", 1), 1)
    T_out = case["T_out"]
    rows = torch.arange(B * T_out) if rows is None else torch.as_tensor(rows, dtype=torch.long)
    b_of, t_of = rows // T_out, rows % T_out
    win = torch.empty(len(rows), k * Cin, dtype=dtype)
    mag = torch.empty(len(rows), k * Cin, dtype=dtype)  # |a| for the error scale
    for b in b_of.unique().tolist():
        sel = (b_of == b).nonzero()[:, 0]
        xb = x[b].to(dtype).T[None]  # [1, C, T]
        mb = xb.abs()
        if case.get("prologue"):
            mb = F.elu(xb).abs() + _elu_exp(xb)
            xb = F.elu(xb)
        idx = t_of[sel, None] * stride + torch.arange(k)
        for src, dst in ((xb, win), (mb, mag)):
            if rep > 1:
                src = src.repeat_interleave(rep, -1)
            xp = _pad1d_reflect(src, pl, pr) if case.get("pad_mode", 0) == 1 else F.pad(src, (pl, pr))
            dst[sel] = xp[0].T[idx].reshape(len(sel), k * Cin)  # [T_padded, C] -> windows
    wf = w.to(dtype).reshape(N, k * Cin)
    y = win @ wf.T
    scale = mag @ wf.abs().T
    if bias is not None:
        y = y + bias.to(dtype)
        scale = scale + bias.to(dtype).abs()
    if gate is not None:
        g = F.silu(gate.reshape(-1, N)[rows].to(dtype))
        y, scale = g * y, g.abs() * scale
    if case.get("act", 0) == 1:
        scale = scale + _elu_exp(y)
    y = act_ref(y, case.get("act", 0))
    if gamma is not None:
        y, scale = y * gamma.to(dtype), scale * gamma.to(dtype).abs()
    if residual is not None:
        r = residual.reshape(-1, N)[rows].to(dtype)
        y, scale = y + r, scale + r.abs()
    if case.get("post", 0) == 1:
        scale = scale + _elu_exp(y)
    y = act_ref(y, case.get("post", 0))
    return y, scale


def _elu_exp(v):
    return torch.where(v < 0, v.clamp_max(0).exp(), torch.zeros_like(v))


def scaled_err(y, truth, scale):
    """max_{m,n} |y - truth| / (scale + tiny): the elementwise error in units of the operation's own magnitude (conv_ref)."""
    return float(((y.double() - truth.double()).abs() / (scale.double() + 1e-30)).max())


def act_ref(v, code):
    return {0: lambda t: t, 1: F.elu, 2: F.gelu, 3: F.silu}[code](v)


# ------------------------------------------------------------------------------------------------------------------
# Near-tie audit of integer code output (the protocol of tests/test_kernels_gpu.py::test_rvq_search_exact applied to whole
# graphs): the codes of another implementation must EQUAL the oracle's except where the oracle's own decision is a
# near-tie.  `emb` is the ORACLE's RVQ input (so both are judged on identical context); the HIP path's embedding differs
# from it by < STAGE_TOL relative RMS, which moves a squared distance difference by at most ~ 2 |delta| |e1 - e2|, hence
# a tolerance relative to the mean squared norm of the inputs; r02's 4e-4 / 2 % were population bounds far above anything observed.
CODE_TIE_TOL = 5e-5  # 10 x the largest excess the round-3 GPU suite observed (5.1e-6 over 56 audits / 5 004 vectors, no accepted flip)
AUDIT_LOG = []  # (n_vectors, flip fraction, largest accepted relative gap, largest relative excess) per audit: printed by conftest's summary


def audit_codes(emb, cb, got, want, rel_tol=CODE_TIE_TOL, max_flip_frac=0.002):
    """emb [n, D] float32 (oracle RVQ input), cb [Q, K, D], got / want [n, Q] int64.  Returns the fraction of vectors
    whose stream left the oracle's at an (accepted) near-tie.  Raises on any decisive mismatch."""
    import numpy as np

    from oracle import rvq_c

    emb = np.ascontiguousarray(emb, np.float32)
    got = np.ascontiguousarray(got, np.int64)
    want = np.ascontiguousarray(want, np.int64)
    assert got.shape == want.shape, (got.shape, want.shape)
    if got.size == 0:
        return 0.0
    assert got.min() >= 0 and got.max() < cb.shape[1]
    excess, best, gap = rvq_c.check_f64(emb, cb, got)  # follows `got`'s own residual path, in double precision
    tol = rel_tol * float((emb.astype(np.float64) ** 2).sum(1).mean())
    assert excess.max() <= tol, f"a chosen code is not a (near-)minimum of the oracle's distances: excess {excess.max():.3e} > {tol:.3e}"
    assert (got[gap > tol] == best[gap > tol]).all(), "index differs from the double-precision arg-min away from a tie"
    diverged = np.zeros(got.shape[0], bool)
    for q in range(got.shape[1]):
        differs = (got[:, q] != want[:, q]) & ~diverged
        assert (gap[differs, q] <= tol).all(), f"stage {q}: {int((gap[differs, q] > tol).sum())} decisive mismatches vs the oracle"
        diverged |= differs
    frac = float(diverged.mean())
    scale = float((emb.astype(np.float64) ** 2).sum(1).mean())
    first = np.zeros(got.shape[0], bool)
    worst_gap = 0.0
    for q in range(got.shape[1]):  # the gap at the stage where a vector first leaves the oracle's stream
        d = (got[:, q] != want[:, q]) & ~first
        if d.any():
            worst_gap = max(worst_gap, float(gap[d, q].max()))
        first |= d
    AUDIT_LOG.append((int(got.shape[0]), frac, worst_gap / scale, float(excess.max()) / scale))
    assert frac <= max_flip_frac, f"{frac:.4f} of the vectors sit on a near-tie: tolerance too loose or embeddings off"
    return frac


def audit_codes_bnq(emb_bdn, cb, got_bqn, want_bqn, **kw):
    """Same, for the reference's layouts: emb [B, D, N] (oracle tap), codes [B, nq, N]."""
    B, D, N = emb_bdn.shape
    flat = lambda c: c.transpose(1, 2).reshape(B * N, -1).cpu().numpy()  # noqa: E731
    return audit_codes(emb_bdn.transpose(1, 2).reshape(B * N, D).numpy(), cb.numpy() if hasattr(cb, "numpy") else cb,
                       flat(got_bqn), flat(want_bqn), **kw)
