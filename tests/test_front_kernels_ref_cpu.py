"""The float64 restatements of tests/front_kernels_ref.py (the truth tests/test_front_kernels_gpu.py holds the kernels of
csrc/seanet_front.hip, csrc/ssl_kernels.hip and csrc/conformer_kernels.hip against) pinned in float64 to what the project already
trusts: oracle.hcodec_ref.sconv1d / seanet_resblock (causal and not), the layer-0 tap and the gated layer of
oracle.ssl_ref.hidden_states, the convolution module and the stft_logmel framing of tests/conformer_ref.py, torch's own operators for
the rest - so a wrong restatement cannot hide a wrong kernel.  The layout packers are evaluated here as well: each operation is
computed once more FROM THE PACKED weights with plain index arithmetic, so a transposed tap or channel fails on the CPU."""
import dataclasses
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import hcodec_ref as R
from oracle import ssl_ref as S
from tests import conformer_ref as CR
from tests import front_kernels_ref as K
from tests.util import rel_err
from unified_audio_amd import synth

F64 = torch.float64
PIN = 1e-12  # float64 against float64 with another association (the convention of tests/test_bicodec_kernels_ref_cpu.py)


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _rn(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g, dtype=F64) * scale


def seanet_weights(g, C, hid, dtype=F64):
    """Reference-layout weights of conv0 and the first residual block: (w0, b0, w3, b3, wsc, bsc, wpw, bpw)."""
    w = (_rn(g, C, 1, 7, scale=7 ** -0.5), _rn(g, C, scale=0.3), _rn(g, hid, C, 3, scale=(3 * C) ** -0.5), _rn(g, hid, scale=0.3),
         _rn(g, C, C, 1, scale=C ** -0.5), _rn(g, C, scale=0.3), _rn(g, C, hid, 1, scale=hid ** -0.5), _rn(g, C, scale=0.3))
    return tuple(t.to(dtype) for t in w)


def _front_from_packed(wav, w0p, b0, w3p, b3p, wscp, bsc, wpwp, bpw, causal):
    """The fused front from the LIBRARY layouts: conv0 [7][C], k3 [32][3][C] + [32], shortcut [C][C], 1x1 [C][32]."""
    B, L = wav.shape
    l0, l3 = (6, 2) if causal else (3, 1)
    xp = R._pad1d_reflect(wav[:, None], l0, 6 - l0)[:, 0]
    x = b0 + sum(xp[:, j:j + L, None] * w0p[j] for j in range(7))                   # [B, L, C]
    ep = R._pad1d_reflect(F.elu(x).transpose(1, 2), l3, 2 - l3).transpose(1, 2)      # [B, L + 2, C]
    h = b3p + sum(torch.einsum("blc,nc->bln", ep[:, j:j + L], w3p[:, j]) for j in range(3))   # [B, L, 32]
    assert torch.equal(h[..., (w3p.abs().sum((1, 2)) == 0)], torch.zeros_like(h[..., (w3p.abs().sum((1, 2)) == 0)]))
    return F.elu(torch.einsum("blc,nc->bln", x, wscp) + bsc + torch.einsum("blh,nh->bln", F.elu(h), wpwp) + bpw)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("hid", [16, 5])
@pytest.mark.parametrize("L", [8, 9, 129, 300])
def test_seanet_front_ref(L, hid, causal):
    g = _g(10 + L + hid)
    C, B = 32, 2
    w0, b0, w3, b3, wsc, bsc, wpw, bpw = W = seanet_weights(g, C, hid)
    wav = _rn(g, B, L)
    # the oracle: SConv1d conv0, then SEANetResnetBlock over weight-normed convolutions (g = |v|: the fold is the identity), then ELU
    sd = {}
    for name, (w, b) in {"block.1": (w3, b3), "block.3": (wpw, bpw), "shortcut": (wsc, bsc)}.items():
        sd[f"rb.{name}.conv.conv.weight_v"], sd[f"rb.{name}.conv.conv.bias"] = w, b
        sd[f"rb.{name}.conv.conv.weight_g"] = w.flatten(1).norm(dim=1).view(-1, 1, 1)
    x = R.sconv1d(wav[:, None], w0, b0, 1, causal=causal)
    want = F.elu(R.seanet_resblock(sd, "rb", x, causal=causal)).transpose(1, 2)
    assert want.shape == (B, L, C)
    assert rel_err(K.seanet_front_ref(wav, *W, causal), want) < PIN
    assert rel_err(K.seanet_front_torch(wav, *W, causal), want) < PIN
    w3p, b3p = K.pack_k3(w3, b3)
    assert w3p.shape == (32, 3, C) and b3p.shape == (32,) and K.pack_pw(wpw).shape == (C, 32)
    got = _front_from_packed(wav, K.pack_conv0(w0), b0, w3p, b3p, K.pack_shortcut(wsc), bsc, K.pack_pw(wpw), bpw, causal)
    assert rel_err(got, want) < PIN
    if causal and L > 100:  # frame t sees nothing behind it (the left reflections reach samples 1 .. 8 only)
        wav2 = wav.clone()
        wav2[:, L // 2 + 1:] += 1.0
        assert torch.equal(K.seanet_front_ref(wav2, *W, True)[:, :L // 2 + 1], K.seanet_front_ref(wav, *W, True)[:, :L // 2 + 1])


def _ssl_spec(C0, k, stride, **kw):
    return S.SSLSpec(conv_dim=(C0,), conv_kernel=(k,), conv_stride=(stride,), hidden_size=16, num_hidden_layers=0, num_attention_heads=2,
                     intermediate_size=32, num_conv_pos_embeddings=4, num_conv_pos_embedding_groups=2, **kw)


@pytest.mark.parametrize("pad", [0, 160])
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("k,stride,C0,T", [(10, 5, 8, 400), (16, 4, 4, 333), (1, 1, 4, 70), (3, 2, 12, 131)])
def test_ssl_conv0_ref(k, stride, C0, T, bias, pad):
    spec = _ssl_spec(C0, k, stride, conv_bias=bias)
    sd = {n: v.double() for n, v in synth.ssl_state_dict(spec, seed=5).items()}
    g = _g(20 + k)
    wav = 100.0 + 0.5 * _rn(g, 3, T)
    taps = {}
    S.hidden_states(sd, F.pad(wav, (pad, pad)), spec, taps)
    want = taps["ssl.conv0"]  # [B, T1, C0]: conv, GroupNorm(C0 groups), GELU
    T1 = want.shape[1]
    assert T1 == (T + 2 * pad - k) // stride + 1
    pre = "feature_extractor.conv_layers.0."
    w, b, gam, bet = sd[pre + "conv.weight"], sd.get(pre + "conv.bias"), sd[pre + "layer_norm.weight"], sd[pre + "layer_norm.bias"]
    assert (b is not None) == bias
    args = (T1, stride, pad, 1, 1e-5, K.ACT_GELU)
    assert rel_err(K.ssl_conv0_ref(wav, w, b, gam, bet, *args), want) < PIN
    assert rel_err(K.ssl_conv0_torch(wav, w, b, gam, bet, *args), want) < PIN
    wav0 = wav - 100.0
    taps0 = {}
    S.hidden_states(sd, F.pad(wav0, (pad, pad)), spec, taps0)
    assert rel_err(K.ssl_conv0_ref(wav0, w, b, gam, bet, *args), taps0["ssl.conv0"]) < PIN
    # plain conv (+ bias), no activation, fewer frames than the signal holds: the first frames of the full convolution
    full = F.conv1d(F.pad(wav, (pad, pad))[:, None], w, b, stride=stride).transpose(1, 2)
    for fn in (K.ssl_conv0_ref, K.ssl_conv0_torch):
        assert rel_err(fn(wav, w, b, None, None, T1 - 1, stride, pad, 0, 0.0, K.ACT_NONE), full[:, :T1 - 1]) < PIN
    # the packed filter [k][C0]
    wp = K.pack_conv0(w)
    xp = F.pad(wav, (pad, pad))
    v = sum(xp[:, j:j + (T1 - 1) * stride + 1:stride, None] * wp[j] for j in range(k)) + (b if bias else 0.0)
    assert rel_err(v, full) < PIN


def _wavlm_layer(sd, spec, x, gate):
    """HubertEncoderLayer (post-LN) over WavLM's attention with the GIVEN gate [B, H, N] of the relative position bias."""
    B, N, d = x.shape
    H = spec.num_attention_heads
    hd = d // H
    pre = "encoder.layers.0."
    lin = lambda t, n: F.linear(t, sd[pre + n + ".weight"], sd[pre + n + ".bias"])  # noqa: E731
    q, k, v = (lin(x, "attention." + n).view(B, N, H, hd).transpose(1, 2) for n in ("q_proj", "k_proj", "v_proj"))
    rel = torch.arange(N)[None, :] - torch.arange(N)[:, None]
    bias = F.embedding(S.relative_position_bucket(rel, spec.num_buckets, spec.max_bucket_distance),
                       sd[pre + "attention.rel_attn_embed.weight"]).permute(2, 0, 1)
    scores = (q * hd ** -0.5) @ k.transpose(-1, -2) + gate[..., None] * bias[None]
    a = (torch.softmax(scores, -1) @ v).transpose(1, 2).reshape(B, N, d)
    ln = lambda t, n: F.layer_norm(t, (d,), sd[pre + n + ".weight"], sd[pre + n + ".bias"], spec.layer_norm_eps)  # noqa: E731
    h = ln(x + lin(a, "attention.out_proj"), "layer_norm")
    return ln(h + lin(F.gelu(lin(h, "feed_forward.intermediate_dense")), "feed_forward.output_dense"), "final_layer_norm")


@pytest.mark.parametrize("H,hd", [(1, 32), (3, 8), (2, 96)])
def test_ssl_gate_ref(H, hd):
    spec = dataclasses.replace(_ssl_spec(8, 10, 5), hidden_size=H * hd, num_hidden_layers=1, num_attention_heads=H, num_buckets=32,
                               max_bucket_distance=40, num_conv_pos_embedding_groups=1)
    sd = {n: v.double() for n, v in synth.ssl_state_dict(spec, seed=6).items()}
    pre = "encoder.layers.0.attention."
    sd[pre + "gru_rel_pos_linear.weight"] = sd[pre + "gru_rel_pos_linear.weight"] * 10.0  # gates away from sigmoid(0)
    hs = S.hidden_states(sd, _rn(_g(30), 2, 200), spec)
    x = hs[0]  # the input of layer 0 = the rows the gate is computed from
    w8, b8, cst = sd[pre + "gru_rel_pos_linear.weight"], sd[pre + "gru_rel_pos_linear.bias"], sd[pre + "gru_rel_pos_const"].reshape(H)
    gate = K.ssl_gate_ref(x, w8, b8, cst, H)
    assert gate.shape == (2, H, x.shape[1]) and float(gate.std()) > 0.05
    assert rel_err(_wavlm_layer(sd, spec, x, gate), hs[1]) < PIN
    assert rel_err(_wavlm_layer(sd, spec, x, torch.full_like(gate, 1.5)), hs[1]) > 1e-4  # the comparison sees the gate
    assert rel_err(gate, K.ssl_gate_torch(x, w8, b8, cst, H)) < PIN
    # the folded weights [2][hd], [2]
    wab, bab = K.pack_gate(w8, b8)
    assert wab.shape == (2, hd) and bab.shape == (2,)
    z = torch.einsum("bnhe,se->bnhs", x.view(2, -1, H, hd), wab) + bab
    a, b = torch.sigmoid(z[..., 0]), torch.sigmoid(z[..., 1])
    assert rel_err((a * (b * cst - 1.0) + 2.0).permute(0, 2, 1), gate) < PIN


@pytest.mark.parametrize("expo", [0.3, 0.0])
def test_ssl_compress_ref(expo):
    g = _g(40)
    s = _rn(g, 2, 5, 6) * 3.0
    s[0, 0, :4] = torch.tensor([0.0, -0.0, 1e-30, -1e-30], dtype=F64)
    scale = 1.0 / 3.0
    a, b = K.ssl_compress_ref(s, scale, expo, [5, 2]), K.ssl_compress_torch(s, scale, expo, [5, 2])
    assert rel_err(a, b) < PIN
    assert torch.equal(a[1, 2:], torch.zeros(3, 6, dtype=F64)) and torch.equal(a[0, 0, :2].abs(), torch.zeros(2, dtype=F64))
    m = s * float(torch.tensor(scale, dtype=torch.float32))
    if expo > 0:  # audio_tokenizer.py: symbol = (x > 0) * 2 - 1; symbol * |x| ** 0.3
        assert rel_err(K.ssl_compress_ref(s, scale, expo), ((m > 0).double() * 2 - 1) * m.abs() ** expo) < PIN
    else:
        assert torch.equal(K.ssl_compress_ref(s, scale, expo), m)


@pytest.mark.parametrize("k", [31, 15, 7, 1])
def test_glu_dwconv_bn_silu_ref(k):
    """Through the whole layer of tests/conformer_ref.conformer_encoder: its `conv` tap is x + pw2(middle(pw1(LN(x)))) with x = the
    sum of its `ff1` and `attn` taps, so the middle can be swapped for the restatement."""
    d = 12
    params = dict(num_layers=1, dim=d, heads=2, dim_head=8, depthwise_conv_kernel_size=k, ff_mult=2, dropout=0.0, qk_norm=None, pe_attn_head=None)
    sd = {n: (v.double() if v.is_floating_point() else v) for n, v in synth.conformer_state_dict(7, params).items()}
    cp = "layers.0.conv_module."
    sd[cp + "sequential.0.bias"][d:] += torch.linspace(-40.0, 40.0, d, dtype=F64)  # gates that saturate on some channels
    x0 = _rn(_g(50 + k), 2, 70, d)
    taps = {}
    CR.conformer_encoder(sd, params, x0, dtype=F64, taps=taps)
    x = taps["conformer.0.ff1"] + taps["conformer.0.attn"]
    y = F.layer_norm(x, (d,), sd[cp + "layer_norm.weight"], sd[cp + "layer_norm.bias"], 1e-5)
    u = F.linear(y, sd[cp + "sequential.0.weight"][:, :, 0], sd[cp + "sequential.0.bias"])  # [B, T, 2d]
    w, bias = sd[cp + "sequential.2.weight"], sd[cp + "sequential.2.bias"]
    bn = [sd[cp + "sequential.3." + n] for n in ("weight", "bias", "running_mean", "running_var")]
    assert w.shape == (d, 1, k)
    for fn in (K.glu_dwconv_bn_silu_ref, K.glu_dwconv_bn_silu_torch):
        v = fn(u, w, bias, *bn)
        got = F.linear(v, sd[cp + "sequential.5.weight"][:, :, 0], sd[cp + "sequential.5.bias"]) + x
        assert rel_err(got, taps["conformer.0.conv"]) < PIN
        assert rel_err(v, K.glu_dwconv_bn_silu_ref(u, w, bias, *bn)) < PIN
    # the packed operands: 31 centred taps [31][C], BatchNorm as scale / shift (rounded to float32 once: compared at that precision)
    w31 = K.pack_dw31(w)
    assert w31.shape == (31, d) and int((w31 != 0).any(1).sum()) == k
    sc, sh = K.pack_batchnorm(*bn)
    assert sc.dtype == sh.dtype == torch.float32
    xg = F.glu(u, dim=-1)
    xp = F.pad(xg, (0, 0, 15, 15))
    acc = bias + sum(xp[:, j:j + 70] * w31[j] for j in range(31))
    assert rel_err(F.silu(acc * sc.double() + sh.double()), K.glu_dwconv_bn_silu_ref(u, w, bias, *bn)) < 1e-6
    sc64 = bn[0] / torch.sqrt(bn[3] + 1e-5)
    assert rel_err(F.silu(acc * sc64 + (bn[1] - bn[2] * sc64)), K.glu_dwconv_bn_silu_ref(u, w, bias, *bn)) < PIN


@pytest.mark.parametrize("n", [320, 700, 6400])
def test_logmel_frames_ref_is_the_framing_of_stft_logmel(n):
    hop, win = 320, 640
    x = _rn(_g(60), 2, n)
    nf = math.ceil(n / hop)
    P = K.logmel_frames_ref(x, (win - hop) // 2, (nf + 1) * hop)
    assert torch.equal(P, K.logmel_frames_torch(x, (win - hop) // 2, (nf + 1) * hop))
    frames = P.unfold(-1, win, hop)  # rows t and t + 1 of the [nf + 1, hop] image are frame t
    assert frames.shape == (2, nf, win)
    spec = torch.fft.rfft(frames * torch.hann_window(win, dtype=F64), dim=-1)
    mel = torch.log(spec.abs() @ CR.htk_fbanks(win // 2 + 1, 0.0, 8000.0, 80, 16000, F64) + 1e-10)
    assert rel_err(mel, CR.stft_logmel(x, dtype=F64)) < PIN
    for pad, n_out in ((0, n - 7), (0, n), (0, n + 9), (320, n + 320), (320, n + 100), (320, n + 999), (320, 200)):
        assert torch.equal(K.logmel_frames_ref(x, pad, n_out), K.logmel_frames_torch(x, pad, n_out)), (pad, n_out)


def test_log_eps_and_cond_prompt_ref():
    g = _g(70)
    x = torch.rand(3, 50, generator=g, dtype=F64) * 10.0
    x[0, :3] = 0.0
    eps = float(torch.tensor(1e-10, dtype=torch.float32))
    assert rel_err(K.log_eps_ref(x, 1e-10), K.log_eps_torch(x, eps)) < PIN
    assert float(K.log_eps_ref(x, 1e-10)[0, 0]) == pytest.approx(math.log(eps), rel=1e-15)
    sos, cond = _rn(g, 6), _rn(g, 3, 4, 6)
    out = K.cond_prompt_ref(sos, cond)
    assert out.shape == (3, 5, 6) and torch.equal(out[:, 0], sos.expand(3, 6)) and torch.equal(out[:, 1:], cond)
