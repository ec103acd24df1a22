"""The recurrence kernels of csrc/lstm.hip alone, through the test hook qa_debug_lstm (one launch_lstm inside a ticket of its own, the
library choosing the kernel as it does inside a codec call), against the recurrence restated in float64 on the CPU from (xw, W_hh)
(tests/lstm_ref.py, pinned against torch.nn.LSTM by tests/test_lstm_ref_cpu.py).  The (unit, gate) row permutation of the kernels'
operands is applied here.

Cases.  T = 2 / 3 / 9: the first hand-off between workgroups, the second, a short run.  The three instances of lstm_team_kernel at the
batch sizes its sequence dealing (b = team + n_teams * q, 32 sequences per launch) branches on: teams without a sequence (B = 1, 5),
a second launch that holds one sequence (33), d = 768's half-filled second row group (4 U = 96 gate rows in two groups of 64: rows
96 .. 127 clamp), d = 1024's second sequence group empty in every team (B = 4) or holding one sequence in team 0 (17); d = 512 / 768 in
both hand-off modes of QA_LSTM_XCD.  lstm_persistent_kernel at d = 1536, whose launcher shares the team launcher's helpers.  T = 1, which
every in-launch form declines, and the per-step kernels with the three knobs off.  Which kernel ran is read off the launch counter of
qa_debug_lstm_stats.  No case injects a fault or shortens the spin limit (tests/test_at_size_gpu.py covers the recovery path).

Parity.  No tolerance is written down: tol = max(2e-6, 4 x rel_err(the same restatement in float32, the float64 truth)) on that same
input - the convention of tests/test_ew_kernels_gpu.py; the kernel's own result never enters it.  h_out and c_state sit between sentinel
guards (tests.util.guarded_out).  Bitwise: two runs agree, and rows 0 .. 2 run alone equal the same rows of the batch (a sequence's
arithmetic does not depend on the batch it rides in).

The in-launch kernels need the whole device resident - 256 CUs, for d = 512 / 768 in eight XCDs of 32: on another device the cases that
expect them skip."""
import ctypes as C
import functools

import pytest
import torch

from tests import lstm_ref as L
from tests.util import check_guarded_out, guarded_out, rel_err

pytestmark = pytest.mark.gpu

HEAD = 64     # floats in front of every guarded output (keeps the 16-byte alignment of the float4 accesses)
B_MAX, T_MAX = 33, 9
PER_LAUNCH = 32  # sequences one in-launch recurrence holds: 4 SG n_teams = 4 x 1 x 8 and 4 x 2 x 4 (team forms), 32 (persistent)
KNOBS = ("QA_LSTM_XCD", "QA_LSTM_TEAM", "QA_LSTM_PERSISTENT")


@functools.lru_cache(maxsize=None)
def _problem(d):
    """Seeded (xw, W_hh) in nn.LSTM's layout at the largest B and T of any case, the float64 truth and the float32 restatement; a case
    takes the leading [B, T] corner (the recurrence runs forward and its sequences are independent)."""
    g = torch.Generator().manual_seed(1000 + d)
    w_hh = (torch.rand(4 * d, d, generator=g, dtype=torch.float64) * 2 - 1) / d ** 0.5  # nn.LSTM's own initialisation
    xw = torch.randn(B_MAX, T_MAX, 4 * d, generator=g, dtype=torch.float64)             # gate pre-activations of order 1
    xw, w_hh = xw.float(), w_hh.float()                                                 # what the kernels are given, exactly
    return xw, w_hh, L.recurrence(xw.double(), w_hh.double()), L.recurrence(xw, w_hh)


def _stats(lib):
    out = (C.c_int64 * 4)()
    assert lib.qa_debug_lstm_stats(0, out) == 0
    return {"launches": out[0], "in_flight": out[1], "diverted": out[2], "degraded": out[3]}


def _whole_device(dev, d):
    p = torch.cuda.get_device_properties(dev)
    if p.multi_processor_count != 256 or "gfx950" not in p.gcnArchName:
        pytest.skip(f"the in-launch recurrence at d = {d} needs 256 CUs in eight XCDs resident at once: "
                    f"{p.gcnArchName} with {p.multi_processor_count} CUs")


def _run(lib, dev, xw, w_hh, expect_launches):
    """One qa_debug_lstm call on xw [B, T, 4d] / w_hh [4d, d] (nn.LSTM's layout) -> (h [B, T, d], c_T [B, d]) on the host."""
    B, T, d4 = xw.shape
    d = d4 // 4
    xw_ug = L.unit_gate_rows(xw.movedim(2, 0)).movedim(0, 2).contiguous().to(dev)
    w_ug = L.unit_gate_rows(w_hh).to(dev)
    hbuf, h = guarded_out(B * T, d, d, HEAD, dev)
    cbuf, c = guarded_out(B, d, d, HEAD, dev)
    before = _stats(lib)
    assert before["degraded"] == 0 and before["in_flight"] == 0, before
    st = lib.qa_debug_lstm(xw_ug.data_ptr(), w_ug.data_ptr(), h.data_ptr(), c.data_ptr(), B, T, d, torch.cuda.current_stream().cuda_stream)
    assert st == 0, lib.qa_last_error()
    torch.cuda.synchronize()
    after = _stats(lib)
    assert after["launches"] - before["launches"] == expect_launches, (before, after)
    assert after["diverted"] == before["diverted"] and after["degraded"] == 0 and after["in_flight"] == 0, (before, after)
    check_guarded_out(hbuf, h, HEAD)
    check_guarded_out(cbuf, c, HEAD)
    assert torch.isfinite(h).all() and torch.isfinite(c).all()
    return h.cpu().reshape(B, T, d).clone(), c.cpu().clone()


def _parity(what, y, ref, yard):
    err, floor = rel_err(y, ref), rel_err(yard, ref)
    tol = max(2e-6, 4.0 * floor)
    print(f"{what}: kernel {err:.3e} float32 restatement {floor:.3e} tol {tol:.3e}")
    assert err <= tol, f"{what}: rel err {err:.3e} > {tol:.3e} (the float32 restatement on the same input: {floor:.3e})"


def _case(lib, dev, d, B, T, in_launch, what):
    xw, w_hh, (h64, c64), (h32, c32) = _problem(d)
    xw, h64, h32, c64, c32 = xw[:B, :T].contiguous(), h64[:B, :T], h32[:B, :T], c64[:B, T - 1], c32[:B, T - 1]
    launches = -(-B // PER_LAUNCH) if in_launch else 0
    h, c = _run(lib, dev, xw, w_hh, launches)
    _parity(f"{what} d {d} B {B} T {T} h", h, h64, h32)
    _parity(f"{what} d {d} B {B} T {T} c_T", c, c64, c32)
    h2, c2 = _run(lib, dev, xw, w_hh, launches)
    assert torch.equal(h, h2) and torch.equal(c, c2), "two runs differ"
    n = min(3, B)
    h3, c3 = _run(lib, dev, xw[:n].contiguous(), w_hh, 1 if in_launch else 0)
    assert torch.equal(h3, h[:n]) and torch.equal(c3, c[:n]), f"rows 0 .. {n - 1} alone differ from the same rows of the batch"


@pytest.mark.parametrize("T", [2, 3, 9])
@pytest.mark.parametrize("mode", [1, 2], ids=["agent", "xcd-local"])
@pytest.mark.parametrize("d,B", [(512, 1), (512, 5), (512, 33), (768, 9), (768, 33)])
def test_team_kernel_one_team_per_xcd(qa_lib, gpu_device, knob, d, B, mode, T):
    _whole_device(gpu_device, d)
    knob("QA_LSTM_XCD", mode)
    _case(qa_lib, gpu_device, d, B, T, True, f"lstm_team_kernel XCD mode {mode}")


@pytest.mark.parametrize("T", [2, 3, 9])
@pytest.mark.parametrize("B", [4, 17, 33])
def test_team_kernel_four_teams_of_64(qa_lib, gpu_device, knob, B, T):
    _whole_device(gpu_device, 1024)
    knob("QA_LSTM_TEAM", 1)
    knob("QA_LSTM_PERSISTENT", -1)
    _case(qa_lib, gpu_device, 1024, B, T, True, "lstm_team_kernel 4 x 64")


def test_persistent_kernel_at_1536(qa_lib, gpu_device, knob):
    _whole_device(gpu_device, 1536)
    knob("QA_LSTM_PERSISTENT", -1)
    _case(qa_lib, gpu_device, 1536, 17, 3, True, "lstm_persistent_kernel")


@pytest.mark.parametrize("d", [512, 768, 1024, 1536])
def test_one_step_is_declined_by_every_in_launch_form(qa_lib, gpu_device, knob, d):
    knob("QA_LSTM_XCD", 1)
    knob("QA_LSTM_TEAM", 1)
    knob("QA_LSTM_PERSISTENT", 1)
    _case(qa_lib, gpu_device, d, 5, 1, False, "T = 1")


@pytest.mark.parametrize("T", [2, 3, 9])  # 9: the replayed step graph (T >= 8)
def test_per_step_kernels_with_the_knobs_off(qa_lib, gpu_device, knob, T):
    for k in KNOBS:
        knob(k, 0)
    _case(qa_lib, gpu_device, 512, 17, T, False, "lstm_step_kernel")
