"""TEST INFRASTRUCTURE ONLY - plain restatements of the kernels of csrc/seanet_front.hip, csrc/ssl_kernels.hip and
csrc/conformer_kernels.hip, taking the weights in the REFERENCE's layouts (Conv1d [out, in, k], BatchNorm statistics, the 8-row
gru_rel_pos_linear) and the activations in the library's (channel-last [B, T, C]).

Three families, all on the CPU:
  *_ref    the reference's formula written out with elementary tensor arithmetic (explicit taps, explicit reflected indices, explicit
           means), float64: the truth of tests/test_front_kernels_gpu.py
  *_torch  the same operation through torch's own operators (F.conv1d, F.pad(mode="reflect"), F.elu, F.group_norm, F.gelu, F.glu,
           F.batch_norm, F.silu, torch.sigmoid, torch.pow, torch.log) in the dtype of its input: in float64 it pins the *_ref functions
           (tests/test_front_kernels_ref_cpu.py), in float32 it is the yardstick the GPU test takes its tolerance from
  pack_*   reference-layout weights -> the library layouts the launchers take (what the loaders of hcodec.cpp / ssl.cpp /
           conformer.cpp do on the host)"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

F64 = torch.float64
ACT_NONE, ACT_GELU = 0, 2  # csrc/common.h


# ------------------------------------------------------------------------------------------------ layout packers
def pack_conv0(w):
    """Conv1d(1 -> C, k) [C, 1, k] -> [k][C] (SEANet conv0 with k = 7, SSL layer 0 with any k)."""
    return w[:, 0, :].t().contiguous()


def pack_k3(w, b, rows=32):
    """Conv1d(C -> hid, 3) [hid, C, 3], [hid] -> [rows][3][C] with the rows >= hid zero, [rows]."""
    hid, C, k = w.shape
    out = torch.zeros(rows, k, C, dtype=w.dtype)
    out[:hid] = w.permute(0, 2, 1)
    bias = torch.zeros(rows, dtype=b.dtype)
    bias[:hid] = b
    return out.contiguous(), bias


def pack_shortcut(w):
    """Conv1d(C -> C, 1) [C, C, 1] -> [C][C] (out, in)."""
    return w[:, :, 0].contiguous()


def pack_pw(w, cols=32):
    """Conv1d(hid -> C, 1) [C, hid, 1] -> [C][cols] with the columns >= hid zero."""
    C, hid, _ = w.shape
    out = torch.zeros(C, cols, dtype=w.dtype)
    out[:, :hid] = w[:, :, 0]
    return out.contiguous()


def pack_dw31(w, taps=31):
    """Depthwise Conv1d [C, 1, k] (k odd <= taps) -> [taps][C], tap j of the kernel at row j + (taps - k) / 2: centred, zeros outside."""
    C, _, k = w.shape
    assert k % 2 == 1 and k <= taps
    out = torch.zeros(taps, C, dtype=w.dtype)
    lo = taps // 2 - k // 2
    out[lo:lo + k] = w[:, 0, :].t()
    return out.contiguous()


def pack_batchnorm(weight, bias, mean, var, eps=1e-5):
    """BatchNorm1d in eval mode as y = x * scale + shift, folded in double and rounded once."""
    sc = weight.double() / torch.sqrt(var.double() + eps)
    return sc.float(), (bias.double() - mean.double() * sc).float()


def pack_gate(w8, b8):
    """gru_rel_pos_linear [8, hd], [8] -> wab [2][hd], bab [2]: the reference sums outputs 0..3 and 4..7 before the sigmoid."""
    return torch.stack((w8[:4].sum(0), w8[4:].sum(0))).contiguous(), torch.stack((b8[:4].sum(), b8[4:].sum()))


# ------------------------------------------------------------------------------------------------ SEANet front
def _reflect_index(n, left, right):
    """Source index of every position of a length-n signal reflect-padded by (left, right); n > max(left, right)."""
    assert n > max(left, right)
    idx = torch.arange(-left, n + right)
    idx = idx.abs()
    return torch.where(idx >= n, 2 * (n - 1) - idx, idx)


def _elu(v):
    return torch.where(v > 0, v, torch.exp(v.clamp(max=0)) - 1.0)


def _sconv_ref(x, w, b, causal):
    """SConv1d at stride 1, channel-last float64: x [B, T, Cin], w [Cout, Cin, k] -> [B, T, Cout]; reflect padding (k - 1, 0) when
    causal, else (ceil((k - 1) / 2), floor((k - 1) / 2))."""
    k = w.shape[-1]
    T = x.shape[1]
    total = k - 1
    left = total if causal else total - total // 2
    xp = x[:, _reflect_index(T, left, total - left)]
    y = b.to(F64).expand(x.shape[0], T, -1).clone()
    for j in range(k):
        y += xp[:, j:j + T] @ w[:, :, j].to(F64).t()
    return y


def seanet_front_ref(wav, w0, b0, w3, b3, wsc, bsc, wpw, bpw, causal):
    """wav [B, L] -> a [B, L, C] = ELU(shortcut(x) + 1x1(ELU(k3(ELU(x))))) with x = conv0(wav); every convolution an SConv1d."""
    x = _sconv_ref(wav.to(F64)[..., None], w0, b0, causal)
    h = _sconv_ref(_elu(x), w3, b3, causal)
    return _elu(_sconv_ref(x, wsc, bsc, causal) + _sconv_ref(_elu(h), wpw, bpw, causal))


def _sconv_torch(x, w, b, causal):
    total = w.shape[-1] - 1
    left = total if causal else total - total // 2
    return F.conv1d(F.pad(x, (left, total - left), mode="reflect") if total else x, w, b)


def seanet_front_torch(wav, w0, b0, w3, b3, wsc, bsc, wpw, bpw, causal):
    x = _sconv_torch(wav[:, None, :], w0, b0, causal)
    h = _sconv_torch(F.elu(x), w3, b3, causal)
    return F.elu(_sconv_torch(x, wsc, bsc, causal) + _sconv_torch(F.elu(h), wpw, bpw, causal)).transpose(1, 2)


# ------------------------------------------------------------------------------------------------ SSL layer 0
def _gelu(v):
    return 0.5 * v * (1.0 + torch.erf(v / math.sqrt(2.0)))


def _ssl_padded(wav, T1, k, stride, pad):
    """Zeros: `pad` in front, and behind as many as frame T1 - 1 needs (at least `pad`: the reference's symmetric padding)."""
    need = (T1 - 1) * stride + k
    return F.pad(wav, (pad, max(pad, need - pad - wav.shape[-1])))


def ssl_conv0_ref(wav, w, bias, gamma, beta, T1, stride, pad, norm_group, eps, act):
    """wav [B, T], w [C0, 1, k] -> [B, T1, C0]: frame t = bias + sum_j w[:, j] xp[t stride + j] over the zero-padded signal; then, with
    norm_group, (v - mean) / sqrt(biased var + eps) * gamma + beta with the statistics per (clip, channel) over the T1 frames; GELU."""
    C0, _, k = w.shape
    xp = _ssl_padded(wav.to(F64), T1, k, stride, pad)
    v = torch.zeros(wav.shape[0], T1, C0, dtype=F64)
    if bias is not None:
        v += bias.to(F64)
    for j in range(k):
        v += xp[:, j:j + (T1 - 1) * stride + 1:stride, None] * w[:, 0, j].to(F64)
    if norm_group:
        d = v - v.mean(1, keepdim=True)
        v = d / (d * d).mean(1, keepdim=True).add(eps).sqrt() * gamma.to(F64) + beta.to(F64)
    return _gelu(v) if act == ACT_GELU else v


def ssl_conv0_torch(wav, w, bias, gamma, beta, T1, stride, pad, norm_group, eps, act):
    C0, _, k = w.shape
    v = F.conv1d(_ssl_padded(wav, T1, k, stride, pad)[:, None], w, bias, stride=stride)[:, :, :T1]
    if norm_group:
        v = F.group_norm(v, C0, gamma, beta, eps)
    return (F.gelu(v) if act == ACT_GELU else v).transpose(1, 2)


# ------------------------------------------------------------------------------------------------ WavLM gate
def ssl_gate_ref(hidden, w8, b8, cst, H):
    """hidden [B, N, H hd] -> gate [B, H, N] = a (b const[h] - 1) + 2, a / b = sigmoid of the sums of outputs 0..3 / 4..7 of
    gru_rel_pos_linear applied to the head's slice of the row."""
    B, N, d = hidden.shape
    x = hidden.to(F64).reshape(B, N, H, d // H)
    proj = (x[..., None, :] * w8.to(F64)).sum(-1) + b8.to(F64)  # [B, N, H, 8]
    a = 1.0 / (1.0 + torch.exp(-proj[..., :4].sum(-1)))
    b = 1.0 / (1.0 + torch.exp(-proj[..., 4:].sum(-1)))
    return (a * (b * cst.to(F64) - 1.0) + 2.0).permute(0, 2, 1)


def ssl_gate_torch(hidden, w8, b8, cst, H):
    """WavLMAttention.forward's own statements (oracle/ssl_ref.py hidden_states.attention)."""
    B, N, d = hidden.shape
    gh = hidden.view(B, N, H, d // H).permute(0, 2, 1, 3)
    proj = F.linear(gh, w8, b8).view(B, H, N, 2, 4).sum(-1)
    ga, gb = torch.sigmoid(proj).chunk(2, dim=-1)
    return (ga * (gb * cst.view(1, H, 1, 1) - 1.0) + 2.0)[..., 0]


# ------------------------------------------------------------------------------------------------ SSL elementwise tail
def ssl_compress_ref(s, scale, expo, lens=None):
    """m = s * scale (scale as the float32 the kernel receives); out = sign |m|^expo with sign = +1 for m > 0 and -1 otherwise, m
    itself for expo <= 0; s [B, N, d] with rows >= lens[b] exactly 0."""
    m = s.to(F64) * float(torch.tensor(scale, dtype=torch.float32))
    out = torch.where(m > 0, 1.0, -1.0) * torch.exp(expo * torch.log(m.abs())) if expo > 0 else m
    return _zero_behind(out, lens)


def ssl_compress_torch(s, scale, expo, lens=None):
    m = s * torch.tensor(scale, dtype=torch.float32).to(s.dtype)
    out = ((m > 0).to(s.dtype) * 2 - 1) * torch.pow(m.abs(), expo) if expo > 0 else m
    return _zero_behind(out, lens)


def _zero_behind(out, lens):
    if lens is not None:
        out = out.clone()
        for b, n in enumerate(lens):
            out[b, n:] = 0.0
    return out


# ------------------------------------------------------------------------------------------------ Conformer convolution module
def glu_dwconv_bn_silu_ref(u, w, bias, bn_w, bn_b, bn_mean, bn_var, eps=1e-5):
    """u [B, T, 2C] -> [B, T, C]: x = u[..., :C] sigmoid(u[..., C:]); y[t] = bias + sum_j w[:, j] x[t + j - (k - 1) / 2] with zeros
    outside the clip (w [C, 1, k], k odd); (y - mean) / sqrt(var + eps) * bn_w + bn_b; y sigmoid(y)."""
    C, _, k = w.shape
    B, T, _ = u.shape
    u = u.to(F64)
    x = u[..., :C] / (1.0 + torch.exp(-u[..., C:]))
    xp = torch.zeros(B, T + k - 1, C, dtype=F64)
    xp[:, k // 2:k // 2 + T] = x
    y = bias.to(F64).expand(B, T, C).clone()
    for j in range(k):
        y += xp[:, j:j + T] * w[:, 0, j].to(F64)
    y = (y - bn_mean.to(F64)) / torch.sqrt(bn_var.to(F64) + eps) * bn_w.to(F64) + bn_b.to(F64)
    return y / (1.0 + torch.exp(-y))


def glu_dwconv_bn_silu_torch(u, w, bias, bn_w, bn_b, bn_mean, bn_var, eps=1e-5):
    """conformer.py's ConvolutionModule between the two pointwise convolutions (tests/conformer_ref.py conformer_encoder)."""
    C, _, k = w.shape
    y = F.glu(u.transpose(1, 2), dim=1)
    y = F.conv1d(y, w, bias, padding=(k - 1) // 2, groups=C)
    y = F.batch_norm(y, bn_mean, bn_var, bn_w, bn_b, False, 0.0, eps)
    return F.silu(y).transpose(1, 2)


# ------------------------------------------------------------------------------------------------ log-mel framing, log, prompt
def logmel_frames_ref(wav, pad, n_out):
    """wav [B, n] -> [B, n_out]: `pad` zeros in front, the signal, zeros behind - cut or extended to n_out samples."""
    B, n = wav.shape
    out = torch.zeros(B, n_out, dtype=wav.dtype)
    m = max(0, min(n, n_out - pad))
    out[:, pad:pad + m] = wav[:, :m]
    return out


def logmel_frames_torch(wav, pad, n_out):
    return F.pad(wav, (pad, max(0, n_out - pad - wav.shape[1])))[:, :n_out]


def log_eps_ref(x, eps):
    return torch.log(x.to(F64) + float(torch.tensor(eps, dtype=torch.float32)))


def log_eps_torch(x, eps):
    return torch.log(x + eps)


def cond_prompt_ref(sos, cond):
    """sos [d], cond [B, T, d] -> [B, T + 1, d]: the start row in front of every item's condition rows."""
    return torch.cat((sos.expand(cond.shape[0], 1, -1), cond), 1)
