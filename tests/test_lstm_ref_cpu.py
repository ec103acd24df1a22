"""tests/lstm_ref.py (the float64 truth of tests/test_lstm_kernels_gpu.py) held against torch.nn.LSTM in float64, and its row
permutation against the one the library applies to a checkpoint (hcodec.cpp: dst = u * 4 + g, src = g * d + u)."""
import pytest
import torch

from tests import lstm_ref as L

TOL = 1e-12  # float64 against float64, a different association of the same few operations


@pytest.mark.parametrize("d,B,T", [(8, 1, 1), (8, 3, 9), (128, 5, 4)])
def test_recurrence_matches_nn_lstm(d, B, T):
    torch.manual_seed(d + B + T)
    rnn = torch.nn.LSTM(d, d, 1, batch_first=True).double()
    x = torch.randn(B, T, d, dtype=torch.float64)
    with torch.no_grad():
        want, (h_n, c_n) = rnn(x)
        xw = x @ rnn.weight_ih_l0.t() + rnn.bias_ih_l0 + rnn.bias_hh_l0
        got, c = L.recurrence(xw, rnn.weight_hh_l0.detach())
    assert got.shape == want.shape == (B, T, d)
    assert float((got - want).abs().max()) <= TOL * float(want.abs().max())
    assert c.shape == (B, T, d) and float((c[:, -1] - c_n[0]).abs().max()) <= TOL * float(c_n.abs().max())
    assert float((got[:, -1] - h_n[0]).abs().max()) <= TOL


def test_unit_gate_rows_is_the_load_time_permutation():
    d = 6
    m = torch.arange(4 * d * 3, dtype=torch.float64).view(4 * d, 3)
    p = L.unit_gate_rows(m)
    for u in range(d):
        for g in range(4):
            assert torch.equal(p[u * 4 + g], m[g * d + u])
    v = torch.arange(4 * d, dtype=torch.float64)
    assert torch.equal(L.unit_gate_rows(v), v.view(4, d).t().reshape(-1))
