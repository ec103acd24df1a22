"""The recurrence of csrc/lstm.hip restated on the CPU, from what the kernels are given: the input projection xw = x W_ih^T + b_ih + b_hh
and W_hh.  nn.LSTM's own layout throughout: the 4d axis in gate-major order (blocks i, f, g, o of d), zero initial state.  The dtype of
the arithmetic is the dtype of the arguments: float64 is the truth of tests/test_lstm_kernels_gpu.py, float32 its yardstick
(tests/test_lstm_ref_cpu.py pins the float64 form against torch.nn.LSTM)."""
import torch


def recurrence(xw, w_hh):
    """xw [B, T, 4d], w_hh [4d, d] -> (h [B, T, d], c [B, T, d]), every step's:  gates_t = xw_t + h_{t-1} W_hh^T,  c_t = s(f) c_{t-1} + s(i) tanh(g),
    h_t = s(o) tanh(c_t)."""
    B, T, d4 = xw.shape
    d = d4 // 4
    assert w_hh.shape == (d4, d) and w_hh.dtype == xw.dtype
    h = torch.zeros(B, d, dtype=xw.dtype)
    c = torch.zeros(B, d, dtype=xw.dtype)
    hs = torch.empty(B, T, d, dtype=xw.dtype)
    cs = torch.empty(B, T, d, dtype=xw.dtype)
    for t in range(T):
        i, f, g, o = (xw[:, t] + h @ w_hh.t()).split(d, dim=1)
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
        h = torch.sigmoid(o) * torch.tanh(c)
        hs[:, t], cs[:, t] = h, c
    return hs, cs


def unit_gate_rows(m):
    """The load-time permutation of the kernels' operands: axis 0 of m [4d, ...] from gate-major (row g * d + u) to (unit, gate) order
    (row u * 4 + g)."""
    d = m.shape[0] // 4
    return m.reshape(4, d, *m.shape[1:]).transpose(0, 1).reshape(m.shape).contiguous()
