"""tests/bicodec_kernels_ref.py (the per-kernel float64 truth of tests/test_bicodec_kernels_gpu.py) held, in float64, against what the
project already trusts: the model-level restatements that the reference's own modules were run against (tests/bicodec_tokenize_ref.py:
_se_res2_block, fsq, ref_clip, wav_normalize, the perceiver's GEGLU and final norm; tests/bicodec_forward_ref.py: astp, code_stats) and
torch's operators (F.layer_norm, F.normalize, torch.var).  The kernel-side weight layouts (wt [7][3][in][out], bst, w1t, w2t) are built
from a state dict here, so a transposed tap or channel pair in the restatement fails on the CPU, before any kernel is blamed."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import bicodec_forward_ref as FR
from tests import bicodec_kernels_ref as K
from tests import bicodec_tokenize_ref as T

TOL = 1e-12  # float64 against float64, a different association of the same few operations


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _close(a, b, tol=TOL):
    a, b = a.double(), b.double()
    assert a.shape == b.shape, (a.shape, b.shape)
    err = float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))
    assert err <= tol, err


def _bn_entries(sd, p, n, g):
    sd[p + ".weight"] = torch.randn(n, generator=g, dtype=torch.float64)  # both signs
    sd[p + ".bias"] = torch.randn(n, generator=g, dtype=torch.float64)
    sd[p + ".running_mean"] = torch.randn(n, generator=g, dtype=torch.float64)
    sd[p + ".running_var"] = torch.rand(n, generator=g, dtype=torch.float64) + 0.5


def _block_sd(C, Hd, g, p="blk"):
    sd, W = {}, C // 8
    for q in (".0", ".2"):
        sd[p + q + ".conv.weight"] = torch.randn(C, C, 1, generator=g, dtype=torch.float64) / C ** 0.5
        sd[p + q + ".conv.bias"] = torch.randn(C, generator=g, dtype=torch.float64)
        _bn_entries(sd, p + q + ".bn", C, g)
    for i in range(7):
        sd[f"{p}.1.convs.{i}.weight"] = torch.randn(W, W, 3, generator=g, dtype=torch.float64) / (3 * W) ** 0.5
        sd[f"{p}.1.convs.{i}.bias"] = torch.randn(W, generator=g, dtype=torch.float64)
        _bn_entries(sd, f"{p}.1.bns.{i}", W, g)
    sd[p + ".3.linear1.weight"] = torch.randn(Hd, C, generator=g, dtype=torch.float64) / C ** 0.5
    sd[p + ".3.linear1.bias"] = torch.randn(Hd, generator=g, dtype=torch.float64)
    sd[p + ".3.linear2.weight"] = torch.randn(C, Hd, generator=g, dtype=torch.float64) / Hd ** 0.5
    sd[p + ".3.linear2.bias"] = torch.randn(C, generator=g, dtype=torch.float64)
    return sd


@pytest.mark.parametrize("d", [1, 2, 4])
@pytest.mark.parametrize("C,Hd,Tn", [(32, 8, 13), (64, 3, 5)])
def test_res2_chain_and_se_residual_rebuild_the_se_res2_block(C, Hd, Tn, d):
    g = _gen(10 + C + d)
    sd = _block_sd(C, Hd, g)
    x = torch.randn(2, C, Tn, generator=g, dtype=torch.float64)
    want = T._se_res2_block(sd, "blk", x, d)
    y1 = T._conv_relu_bn(sd, "blk.0", x)
    wt, bst = K.pack_res2(sd, "blk.1")
    assert wt.shape == (7, 3, C // 8, C // 8) and bst.shape == (7, 3, C // 8)
    y2 = K.res2_chain_ref(y1.transpose(1, 2), wt, bst, d)
    assert torch.equal(y2[..., 7 * (C // 8):], y1.transpose(1, 2)[..., 7 * (C // 8):])
    y3 = T._conv_relu_bn(sd, "blk.2", y2.transpose(1, 2))
    gate, out = K.se_residual_ref(x.transpose(1, 2), y3.transpose(1, 2), *K.pack_se(sd, "blk.3"))
    _close(out.transpose(1, 2), want)
    assert gate.shape == (2, C) and float(gate.min()) > 0 and float(gate.max()) < 1
    # the layouts are not symmetric: the same weights with in / out exchanged, or the taps reversed, are another function
    for bad in (wt.transpose(2, 3), wt.flip(1)):
        assert float((K.res2_chain_ref(y1.transpose(1, 2), bad.contiguous(), bst, d) - y2).abs().max()) > 1e-3


@pytest.mark.parametrize("levels", [[4] * 6, [8, 5, 5, 5], [2], [3] * 8])
def test_fsq_ref_is_the_model_level_fsq(levels):
    g = _gen(20 + len(levels))
    D, rows = 37, 200
    w = torch.randn(len(levels), D, generator=g, dtype=torch.float64) / D ** 0.5
    b = 0.1 * torch.randn(len(levels), generator=g, dtype=torch.float64)
    x = torch.randn(1, rows, D, generator=g, dtype=torch.float64)
    sd = {T.SPK + ".quantizer.project_in.weight": w, T.SPK + ".quantizer.project_in.bias": b}
    taps = {}
    want = T.fsq(sd, x, levels, taps)
    bounded, digits, tokens = K.fsq_ref(x[0], w, b, levels)
    _close(bounded, taps["fsq.bounded"][0])
    assert torch.equal(tokens, want[0].long())
    assert torch.equal(K.fsq_digits_of(tokens, levels), digits)
    if levels != [2]:  # L = 2 shifts z by atanh(0.999) = 3.8: unit-variance inputs stay in its upper level
        assert int(digits.min()) == 0 and all(int(digits[:, i].max()) == L - 1 for i, L in enumerate(levels))  # every level is reached


@pytest.mark.parametrize("ref_len", [9, 61, 64])
def test_mel_frames_ref_is_ref_clip_under_stft_padding(ref_len):
    hop = 8
    nf = ref_len // hop + 1
    g = _gen(30)
    for Tn in sorted({1, max(ref_len - 3, 1), ref_len, ref_len + 5}):
        wav = torch.randn(3, Tn, generator=g, dtype=torch.float64)
        want = F.pad(T.ref_clip(wav, ref_len)[None], (hop, hop), mode="reflect")[0][:, :(nf + 1) * hop]
        assert torch.equal(K.mel_frames_ref(wav, ref_len, hop, nf), want)
        lens = [Tn, max(Tn // 2, 1), 1]
        P = K.mel_frames_ref(wav, ref_len, hop, nf, lens)
        for b, n in enumerate(lens):
            assert torch.equal(P[b:b + 1], K.mel_frames_ref(wav[b:b + 1, :n], ref_len, hop, nf))
    # frames t, t + 1 of P viewed as [nf + 1, hop] are torch.stft's centred window t (n_fft = 2 hop)
    wav = torch.randn(1, ref_len + 5, generator=g, dtype=torch.float64)
    P = K.mel_frames_ref(wav, ref_len, hop, nf)[0]
    frames = F.pad(T.ref_clip(wav, ref_len)[None], (hop, hop), mode="reflect")[0, 0].unfold(0, 2 * hop, hop)
    assert frames.shape[0] == nf and torch.equal(P.unfold(0, 2 * hop, hop), frames)


def test_wav_normalize_ref():
    g = _gen(40)
    wav = 0.3 + 0.01 * torch.randn(3, 257, generator=g, dtype=torch.float64)
    _close(K.wav_normalize_ref(wav, 1e-7), T.wav_normalize(wav, 1e-7))
    lens = [257, 100, 1]
    y = K.wav_normalize_ref(wav, 1e-7, lens)
    for b, n in enumerate(lens):
        _close(y[b:b + 1, :n], T.wav_normalize(wav[b:b + 1, :n], 1e-7)) if n > 1 else None
        assert torch.equal(y[b, n:], torch.zeros(257 - n, dtype=torch.float64))
    assert float(y[2, 0]) == 0.0  # one sample: (x - x) / sqrt(0 + eps)


def test_geglu_and_final_norm_are_the_perceivers():
    g = _gen(50)
    Fh, ldo, rows, D = 341, 344, 7, 12
    h = 3.0 * torch.randn(rows, 2 * Fh, generator=g, dtype=torch.float64)
    a, gate = h.chunk(2, dim=-1)  # perceiver(): a, gate = Linear(lat).chunk(2); F.gelu(gate) * a
    out = K.geglu_ref(h, Fh, ldo)
    _close(out[:, :Fh], F.gelu(gate) * a)
    assert torch.equal(out[:, Fh:], torch.zeros(rows, ldo - Fh, dtype=torch.float64))
    lat = torch.randn(3, 5, D, generator=g, dtype=torch.float64)
    gamma = torch.randn(D, generator=g, dtype=torch.float64)
    _close(K.l2norm_scale_ref(lat.reshape(-1, D), gamma, D ** 0.5), (F.normalize(lat, dim=-1) * D ** 0.5 * gamma).reshape(-1, D))
    assert torch.equal(K.l2norm_scale_ref(torch.zeros(2, D), gamma, D ** 0.5), torch.zeros(2, D, dtype=torch.float64))


@pytest.mark.parametrize("Tn", [1, 2, 5, 40])
def test_astp_pool_and_frame_stats_are_the_x_vector_heads(Tn):
    g = _gen(60 + Tn)
    B, C, Hd = 2, 6, 4
    H = FR.HEAD
    sd = {H + ".pool.linear1.weight": torch.randn(Hd, 3 * C, 1, generator=g, dtype=torch.float64),
          H + ".pool.linear1.bias": torch.randn(Hd, generator=g, dtype=torch.float64),
          H + ".pool.linear2.weight": 3.0 * torch.randn(C, Hd, 1, generator=g, dtype=torch.float64),
          H + ".pool.linear2.bias": torch.randn(C, generator=g, dtype=torch.float64)}
    _bn_entries(sd, H + ".bn", 2 * C, g)
    latent = 2.0 + torch.randn(B, Tn, C, generator=g, dtype=torch.float64)
    ctx = K.frame_stats_ref(latent)
    x = latent.transpose(1, 2)
    _close(ctx[:, :C], x.mean(-1))
    if Tn == 1:
        assert torch.isnan(ctx[:, C:]).all() and torch.isnan(torch.var(x, dim=-1)).all()
        return  # the reference's attention is NaN on one frame; nothing to pin the pool to
    _close(ctx[:, C:], torch.sqrt(torch.var(x, dim=-1) + 1e-7))
    x_in = torch.cat((x, ctx[:, :C, None].expand_as(x), ctx[:, C:, None].expand_as(x)), 1)
    logit = F.conv1d(torch.tanh(F.conv1d(x_in, sd[H + ".pool.linear1.weight"], sd[H + ".pool.linear1.bias"])),
                     sd[H + ".pool.linear2.weight"], sd[H + ".pool.linear2.bias"]).transpose(1, 2)
    s, t = K.fold_bn(*(sd[f"{H}.bn.{k}"] for k in ("weight", "bias", "running_mean", "running_var")))
    pool, bn = K.astp_pool_ref(logit, latent, s, t)
    want = FR.astp(sd, latent)
    _close(pool, want)
    _close(bn, T._bn(sd, H + ".bn", want))


def test_astp_pool_ref_clamps_the_variance():
    x = torch.full((1, 5, 3), 2.5, dtype=torch.float64)
    pool, _ = K.astp_pool_ref(torch.randn(1, 5, 3, generator=_gen(61), dtype=torch.float64), x, torch.ones(6), torch.zeros(6))
    _close(pool[:, 3:], torch.full((1, 3), 1e-7 ** 0.5, dtype=torch.float64))


@pytest.mark.parametrize("Kc,n", [(1, 1), (1000, 1023), (1025, 5000)])
def test_code_usage_ref_is_code_stats(Kc, n):
    idx = torch.randint(0, Kc, (n,), generator=_gen(70 + n))
    ppl, active = K.code_usage_ref(idx, Kc)
    p64, a64 = FR.code_stats(idx, Kc)
    exact = FR.perplexity_exact(idx, Kc)
    assert abs(float(ppl) - float(p64)) <= 1e-12 * float(p64) and abs(float(ppl) - exact) <= 1e-12 * exact
    assert float(active) == float(a64)
    # indices outside [0, K) are not counted but stay in n: one_hot over K + 1 classes with the extra column dropped
    bad = torch.cat((idx, torch.full((3,), -1), torch.full((2,), Kc)))
    onehot = F.one_hot(torch.where((bad < 0) | (bad >= Kc), torch.tensor(Kc), bad), Kc + 1)[:, :Kc].double()
    p = onehot.mean(0)
    ppl_b, active_b = K.code_usage_ref(bad, Kc)
    want = math.exp(-math.fsum(float(v) * math.log(float(v) + 1e-10) for v in p))
    assert abs(float(ppl_b) - want) <= 1e-12 * want and float(active_b) == float(a64)


@pytest.mark.parametrize("C", [4, 252])
def test_row_ops_are_torchs(C):
    g = _gen(80 + C)
    x = 100.0 + 0.5 * torch.randn(3, 5, C, generator=g, dtype=torch.float64)
    cond = torch.randn(3, 2 * C + 4, generator=g, dtype=torch.float64)
    scale, shift = cond[:, :C], cond[:, C:2 * C]
    _close(K.adaln_ref(x, scale, shift, 1e-6), F.layer_norm(x, (C,), eps=1e-6) * scale[:, None] + shift[:, None], 1e-9)
    _close(K.add_rowvec_ref(x, scale), x + scale[:, None])
    rows = x.reshape(-1, C).clone()
    rows[3] = 0.0
    y = K.l2norm_rows_ref(rows)
    _close(y, F.normalize(rows, dim=-1))
    assert torch.equal(y[3], torch.zeros(C, dtype=torch.float64))
    ri = torch.randn(6, 2 * 12, generator=g, dtype=torch.float64)
    mag = K.spec_mag_ref(ri, 12, 9, 16)
    _close(mag[:, :9], torch.complex(ri[:, :9], ri[:, 12:21]).abs())
    assert torch.equal(mag[:, 9:], torch.zeros(6, 7, dtype=torch.float64))


def test_pure_moves():
    g = _gen(90)
    V, D, B, Tn = 5, 8, 3, 7
    table = torch.randn(V, D, generator=g)
    tok = torch.randint(0, V, (B, Tn), generator=g)
    tok[0, 1], tok[1, 2] = -3, V + 2
    out = K.gather_rows_ref(tok.reshape(-1), table)
    assert torch.equal(out, F.embedding(tok.clamp(0, V - 1), table).reshape(-1, D))
    assert torch.equal(out[1], table[0]) and torch.equal(out[Tn + 2], table[V - 1])
    lens = [7, 3, 1]
    rag = K.gather_rows_ref(tok.reshape(-1), table, Tn, lens).reshape(B, Tn, D)
    for b, n in enumerate(lens):
        assert torch.equal(rag[b, :n], out.reshape(B, Tn, D)[b, :n]) and torch.equal(rag[b, n:], torch.zeros(Tn - n, D))
    gg = K.gather_global_ref(tok, table)
    for b in range(B):
        for n in range(Tn):
            for c in range(D):
                assert gg[b, c * Tn + n] == table[min(max(int(tok[b, n]), 0), V - 1), c]
    filled = K.tokens_fill_behind_ref(tok, [3, 1, 0])
    assert torch.equal(filled[0, :3], tok[0, :3]) and (filled[0, 3:] == -1).all() and (filled[2] == -1).all()
    x = torch.randn(B, 20, generator=g)
    z = K.zero_behind_ref(x, [3, 1, 0], 4)
    assert torch.equal(z[0, :12], x[0, :12]) and (z[0, 12:] == 0).all() and torch.equal(z[1, :4], x[1, :4]) and (z[2] == 0).all()
    lat, xs, ctx = torch.randn(5, D, generator=g), torch.randn(B, Tn, D, generator=g), torch.randn(B, 5 + Tn, D, generator=g)
    assert torch.equal(K.perceiver_ctx_ref(ctx, lat, xs, Tn), torch.cat((lat.expand(B, -1, -1), xs), 1))
    per = torch.randn(B, 5, D, generator=g)
    assert torch.equal(K.perceiver_ctx_ref(ctx, per, None, Tn), torch.cat((per, ctx[:, 5:]), 1))
