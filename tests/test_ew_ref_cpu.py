"""The float64 restatements of tests/ew_ref.py (the truth tests/test_ew_kernels_gpu.py holds the kernels of csrc/ew.hip against) pinned
to torch's own operators in float64: F.layer_norm and an RMSNorm with eps inside the sqrt, F.group_norm + F.silu, F.conv1d(groups=C)
with "same" and causal zero padding, R.sconv1d, the fold / trim / envelope of the reference's ISTFT - so a wrong restatement cannot hide
a wrong kernel.  Per-clip lengths: a ragged clip is that clip run alone, for both families."""
import pytest
import torch

from tests import ew_ref as E
from tests.util import rel_err

F64 = torch.float64
PIN = 1e-13  # two float64 evaluations of the same formula: orders of magnitude below anything the fp32 kernels are asked for


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _close(a, b):
    live = ~torch.isnan(b)
    assert torch.equal(torch.isnan(a), ~live), "the two families disagree on what lies behind a clip's end"
    assert rel_err(a[live], b[live]) < PIN


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("C", [4, 260, 2048])
def test_rownorm_ref(mode, C):
    g = _g(1)
    x = torch.randn(5, C, generator=g, dtype=F64) * 0.5 + 100.0
    w, b = torch.randn(C, generator=g, dtype=F64), torch.randn(C, generator=g, dtype=F64)
    for bias in (None, b) if mode else (None,):
        for eps in (1e-6, 1e-5):
            _close(E.rownorm_ref(x, w, bias, eps, mode), E.rownorm_torch(x, w, bias, eps, mode))
    if mode == 0:  # eps inside the sqrt: with a large eps the two placements differ visibly
        y = E.rownorm_ref(x * 1e-3, w, None, 1e-2, 0)
        assert rel_err(y, x * 1e-3 / ((x * 1e-3).pow(2).mean(-1, keepdim=True) + 1e-2).sqrt() * w) < PIN
        assert rel_err(y, x * 1e-3 / ((x * 1e-3).pow(2).mean(-1, keepdim=True).sqrt() + 1e-2) * w) > 1e-2


@pytest.mark.parametrize("ln", [False, True])
@pytest.mark.parametrize("B,T,C,k,lens", [(2, 1, 64, 7, None), (3, 37, 260, 5, None), (3, 37, 8, 5, [37, 5, 1]), (2, 9, 12, 3, [4, 9])])
def test_dwconv_ref(ln, B, T, C, k, lens):
    g = _g(2)
    x = torch.randn(B, T, C, generator=g, dtype=F64)
    w, bias = torch.randn(k, C, generator=g, dtype=F64), torch.randn(C, generator=g, dtype=F64)
    lnw, lnb = (torch.randn(C, generator=g, dtype=F64), torch.randn(C, generator=g, dtype=F64)) if ln else (None, None)
    for pad_left in (-1, k - 1):
        _close(E.dwconv_ref(x, w, bias, lnw, lnb, 1e-6, pad_left, lens), E.dwconv_torch(x, w, bias, lnw, lnb, 1e-6, pad_left, lens))
    # causal: frame t sees nothing behind it
    x2 = x.clone()
    x2[:, T // 2 + 1:] += 1.0
    a, b = E.dwconv_ref(x, w, bias, None, None, 0.0, k - 1), E.dwconv_ref(x2, w, bias, None, None, 0.0, k - 1)
    assert torch.equal(a[:, :T // 2 + 1], b[:, :T // 2 + 1])


@pytest.mark.parametrize("swish", [0, 1])
@pytest.mark.parametrize("B,T,C,G,lens", [(2, 1, 32, 32, None), (3, 66, 64, 32, None), (2, 64, 96, 8, None), (3, 66, 64, 32, [66, 64, 1])])
def test_groupnorm_ref(swish, B, T, C, G, lens):
    g = _g(3)
    x = torch.randn(B, T, C, generator=g, dtype=F64) * 0.5 + 100.0 * torch.tensor([1.0, -1.0]).repeat(C // 2)
    w, bias = torch.randn(C, generator=g, dtype=F64), torch.randn(C, generator=g, dtype=F64)
    a, b = E.groupnorm_ref(x, w, bias, G, 1e-6, swish, lens), E.groupnorm_torch(x, w, bias, G, 1e-6, swish, lens)
    live = ~torch.isnan(b)
    assert torch.equal(torch.isnan(a), ~live)
    # float64 F.group_norm itself carries ~1e-16 * (mean / std)^2 here; 1e-9 is still far below the fp32 kernels' 1e-7
    assert rel_err(a[live], b[live]) < 1e-9


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("T,lens", [(1, None), (3, None), (4, None), (300, None), (9, [9, 3, 1, 7])])
def test_conv_in_ref(bias, T, lens):
    g = _g(4)
    B, k, Cout = (4 if lens else 2), 7, 8
    x = torch.randn(B, T, generator=g, dtype=F64)
    w = torch.randn(k, Cout, generator=g, dtype=F64)
    b = torch.randn(Cout, generator=g, dtype=F64) if bias else None
    for pad_left in (-1, k - 1):
        _close(E.conv_in_ref(x, w, b, pad_left, lens), E.conv_in_torch(x, w, b, pad_left, lens))


@pytest.mark.parametrize("interleaved", [0, 1])
@pytest.mark.parametrize("rot_heads", [0, 1, 5])
def test_rope_ref(interleaved, rot_heads):
    g = _g(5)
    B, N, H, hd, pos0 = 2, 5, 3, 8, 7
    qkv = torch.randn(B, N, 3 * H * hd + 8, generator=g, dtype=F64)
    ang = torch.rand(pos0 + N, hd // 2, generator=g, dtype=F64) * 40.0
    cs = torch.stack((ang.cos(), ang.sin()), -1)
    a, b = E.rope_ref(qkv, cs, H, hd, pos0, interleaved, rot_heads), E.rope_torch(qkv, cs, H, hd, pos0, interleaved, rot_heads)
    assert rel_err(a, b) < PIN
    Hr = H if rot_heads == 0 else min(rot_heads, H)
    d = H * hd
    for lo, hi in ((Hr * hd, d), (d + Hr * hd, 2 * d), (2 * d, qkv.shape[-1])):  # unrotated heads, v and the padding columns
        assert torch.equal(a[..., lo:hi], qkv[..., lo:hi])
    assert not torch.equal(a[..., :Hr * hd], qkv[..., :Hr * hd])
    # a rotation: pair norms are kept, and position 0 with a zero angle is the identity
    ident = E.rope_ref(qkv, torch.tensor([1.0, 0.0], dtype=F64).expand(N, hd // 2, 2), H, hd, 0, interleaved, rot_heads)
    assert torch.equal(ident, qkv)
    assert rel_err(a[..., :d].reshape(B, N, H, hd).norm(dim=-1), qkv[..., :d].reshape(B, N, H, hd).norm(dim=-1)) < PIN


@pytest.mark.parametrize("ld_in,ld_out", [(10, 10), (12, 16)])
def test_istft_spec_and_stft_post_ref(ld_in, ld_out):
    g = _g(6)
    rows, nb = 3, 5
    y = torch.randn(rows, ld_in, generator=g, dtype=F64)
    y[:, :nb] = torch.linspace(2.0, 7.0, rows * nb, dtype=F64).view(rows, nb)  # exp() on both sides of the clip at 100 (log 100 = 4.6)
    y[:, nb:2 * nb] *= 20.0
    S = E.istft_spec_ref(y, nb, ld_out)
    assert rel_err(S, E.istft_spec_torch(y, nb, ld_out)) < PIN
    mag = (S[:, :nb] ** 2 + S[:, nb:2 * nb] ** 2).sqrt()
    assert float(mag.max()) <= 100.0 * (1 + 1e-12) and int((mag > 99.999).sum()) not in (0, rows * nb)
    assert torch.equal(S[:, 2 * nb:], torch.zeros(rows, ld_out - 2 * nb, dtype=F64))
    ri = torch.randn(rows, ld_in, generator=g, dtype=F64)
    ri[0, 0] = ri[0, nb] = 0.0                    # |X| = 0: the clip at 1e-5, angle 0
    ri[1, 1], ri[1, nb + 1] = -2.0, 0.0           # the negative real axis: +pi
    ri[1, 2], ri[1, nb + 2] = -2.0, -0.0          # ... approached from below: -pi
    P = E.stft_post_ref(ri, nb, ld_out)
    assert rel_err(P, E.stft_post_torch(ri, nb, ld_out)) < PIN
    assert float(P[0, 0]) == pytest.approx(torch.log(torch.tensor(1e-5, dtype=F64)).item()) and float(P[0, nb]) == 0.0
    assert float(P[1, nb + 1]) == 1.0 and float(P[1, nb + 2]) == -1.0
    assert torch.equal(P[:, 2 * nb:], torch.zeros(rows, ld_out - 2 * nb, dtype=F64))


@pytest.mark.parametrize("B,T,n_fft,hop,lens", [(2, 1, 16, 4, None), (2, 9, 16, 4, None), (1, 6, 64, 16, None), (2, 9, 16, 4, [9, 1])])
def test_istft_ola_ref(B, T, n_fft, hop, lens):
    g = _g(7)
    win = torch.hann_window(n_fft, dtype=F64)
    frames = torch.randn(B, T, n_fft, generator=g, dtype=F64) * win
    a, b = E.istft_ola_ref(frames, win, hop, lens), E.istft_ola_torch(frames, win, hop, lens)
    assert a.shape == (B, T * hop) and rel_err(a, b) < PIN
    if lens:
        for i, n in enumerate(lens):
            assert torch.equal(a[i, n * hop:], torch.zeros((T - n) * hop, dtype=F64))
            assert torch.equal(a[i, :n * hop], E.istft_ola_ref(frames[i:i + 1, :n], win, hop)[0])
