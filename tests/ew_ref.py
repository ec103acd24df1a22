"""TEST INFRASTRUCTURE ONLY - plain restatements of the row / elementwise kernels of csrc/ew.hip, in the library's own layouts
(channel-last activations [B, T, C], depthwise / first-conv weights [ksize][C]).

Two families, both on the CPU:
  *_ref    the formula of the kernel's comment written out with elementary tensor arithmetic, float64: the truth of
           tests/test_ew_kernels_gpu.py
  *_torch  the same operation through torch's own operator (F.layer_norm, F.group_norm, F.conv1d, R.sconv1d, F.fold ...) in the
           dtype of its input: in float64 it pins the *_ref functions (tests/test_ew_ref_cpu.py), in float32 it is the yardstick the
           GPU test takes its tolerance from
Per-clip lengths: `lens` (a list of B frame counts, already multiplied by the call's len_mul) makes clip b the clip run alone at
T = lens[b]; what lies behind a clip's end is NaN (exact 0 for the overlap-add, which defines those samples)."""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from oracle import hcodec_ref as R

F64 = torch.float64


def per_clip(fn, x, lens, fill=float("nan")):
    """fn(x[b : b + 1, :len_b]) per clip, stacked into [B, T, ...] with `fill` behind each clip's end."""
    if lens is None:
        return fn(x)
    T = x.shape[1]
    out = None
    for b, n in enumerate(lens):
        n = min(int(n), T)
        yb = fn(x[b:b + 1, :n])
        per_frame = yb.shape[1] // n
        if out is None:
            out = torch.full((x.shape[0], T * per_frame) + tuple(yb.shape[2:]), fill, dtype=yb.dtype)
        out[b, :n * per_frame] = yb[0]
    return out


# ------------------------------------------------------------------------------------------------ row norms
def rownorm_ref(x, w, b, eps, mode):
    """mode 0: x / sqrt(mean(x^2) + eps) * w; mode 1: (x - mean) / sqrt(biased var + eps) * w (+ b).  x [rows, C]."""
    x, w = x.to(F64), w.to(F64)
    if mode == 0:
        return x / (x * x).mean(-1, keepdim=True).add(eps).sqrt() * w
    d = x - x.mean(-1, keepdim=True)
    y = d / (d * d).mean(-1, keepdim=True).add(eps).sqrt() * w
    return y if b is None else y + b.to(F64)


def rownorm_torch(x, w, b, eps, mode):
    if mode == 0:
        return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * w
    return F.layer_norm(x, (x.shape[-1],), w, b, eps)


# ------------------------------------------------------------------------------------------------ depthwise conv (+ LayerNorm)
def _dw_pad(ksize, pad_left):
    return pad_left if pad_left >= 0 else ksize // 2


def dwconv_ref(x, w_kc, bias, lnw, lnb, eps, pad_left=-1, lens=None):
    """y[b, t, c] = bias[c] + sum_j w[j, c] x[b, t + j - pad, c], zero outside the clip; then LayerNorm over c if lnw is given."""
    k = w_kc.shape[0]
    pad = _dw_pad(k, pad_left)

    def one(xb):
        n = xb.shape[1]
        xp = torch.zeros(xb.shape[0], n + k - 1, xb.shape[2], dtype=F64)
        xp[:, pad:pad + n] = xb.to(F64)
        y = bias.to(F64).expand(xb.shape[0], n, -1).clone()
        for j in range(k):
            y += w_kc[j].to(F64) * xp[:, j:j + n]
        return y if lnw is None else rownorm_ref(y, lnw, lnb, eps, 1)

    return per_clip(one, x, lens)


def dwconv_torch(x, w_kc, bias, lnw, lnb, eps, pad_left=-1, lens=None):
    k, C = w_kc.shape
    pad = _dw_pad(k, pad_left)

    def one(xb):
        y = F.conv1d(F.pad(xb.transpose(1, 2), (pad, k - 1 - pad)), w_kc.t().reshape(C, 1, k), bias, groups=C).transpose(1, 2)
        return y if lnw is None else F.layer_norm(y, (C,), lnw, lnb, eps)

    return per_clip(one, x, lens)


# ------------------------------------------------------------------------------------------------ GroupNorm (+ swish)
def groupnorm_ref(x, w, bias, G, eps, swish, lens=None):
    """Statistics per (clip, group) over the clip's frames and the group's C / G channels (biased variance), affine per channel,
    then y * sigmoid(y) if swish."""
    C = x.shape[-1]

    def one(xb):
        v = xb.to(F64).reshape(xb.shape[0], xb.shape[1], G, C // G)
        d = v - v.mean((1, 3), keepdim=True)
        y = (d / (d * d).mean((1, 3), keepdim=True).add(eps).sqrt()).reshape(xb.shape) * w.to(F64) + bias.to(F64)
        return y / (1.0 + torch.exp(-y)) if swish else y

    return per_clip(one, x, lens)


def groupnorm_torch(x, w, bias, G, eps, swish, lens=None):
    def one(xb):
        y = F.group_norm(xb.transpose(1, 2), G, w, bias, eps)
        return (F.silu(y) if swish else y).transpose(1, 2)

    return per_clip(one, x, lens)


# ------------------------------------------------------------------------------------------------ first conv (C_in = 1, reflect)
def _conv_in_pads(ksize, pad_left):
    total = ksize - 1
    left = pad_left if pad_left >= 0 else total - total // 2
    return left, total - left


def conv_in_ref(x, w_kc, bias, pad_left=-1, lens=None):
    """y[b, t, co] = bias[co] + sum_j w[j, co] xp[b, t + j], xp = the reflect padding of SConv1d (short-input rule included).
    x [B, T] -> [B, T, Cout]."""
    k = w_kc.shape[0]
    left, right = _conv_in_pads(k, pad_left)

    def one(xb):
        n = xb.shape[1]
        xp = R._pad1d_reflect(xb.to(F64)[:, None, :], left, right)[:, 0]
        y = torch.zeros(xb.shape[0], n, w_kc.shape[1], dtype=F64)
        if bias is not None:
            y += bias.to(F64)
        for j in range(k):
            y += xp[:, j:j + n, None] * w_kc[j].to(F64)
        return y

    return per_clip(one, x, lens)


def conv_in_torch(x, w_kc, bias, pad_left=-1, lens=None):
    """R.sconv1d (stride 1): non-causal for pad_left < 0, causal for pad_left = ksize - 1."""
    k = w_kc.shape[0]
    assert pad_left < 0 or pad_left == k - 1

    def one(xb):
        return R.sconv1d(xb[:, None, :], w_kc.t().reshape(-1, 1, k), bias, 1, causal=pad_left >= 0).transpose(1, 2)

    return per_clip(one, x, lens)


# ------------------------------------------------------------------------------------------------ RoPE
def _rope_heads(H, rot_heads):
    return min(rot_heads, H) if rot_heads > 0 else H


def rope_ref(qkv, cos_sin, H, hd, pos0=0, interleaved=0, rot_heads=0):
    """qkv [B, N, ld] with (q | k | v) in the first 3 H hd columns; cos_sin [P, hd / 2, 2] = (cos, sin) of position p, pair i.
    Pair i of a head is (i, i + hd / 2) (rotate-half) or (2 i, 2 i + 1) (interleaved): (a, b) -> (a c - b s, b c + a s), for q and
    k of heads < rot_heads (all if 0); everything else is returned as it came."""
    B, N, _ = qkv.shape
    d, half, Hr = H * hd, hd // 2, _rope_heads(H, rot_heads)
    out = qkv.to(F64).clone()
    cs = cos_sin[pos0:pos0 + N].to(F64)
    c, s = cs[None, :, None, :, 0], cs[None, :, None, :, 1]  # [1, N, 1, half]
    for part in range(2):
        v = qkv[..., part * d:(part + 1) * d].to(F64).reshape(B, N, H, hd)[:, :, :Hr]
        a, b = (v[..., 0::2], v[..., 1::2]) if interleaved else (v[..., :half], v[..., half:])
        ra, rb = a * c - b * s, b * c + a * s
        r = torch.stack((ra, rb), -1).reshape(B, N, Hr, hd) if interleaved else torch.cat((ra, rb), -1)
        out[..., part * d:part * d + Hr * hd] = r.reshape(B, N, Hr * hd)
    return out


def rope_torch(qkv, cos_sin, H, hd, pos0=0, interleaved=0, rot_heads=0):
    """The reference's own statements in the dtype of qkv: rotate-half as q * cos + rotate_half(q) * sin over tables cat(f, f)
    (R.attention_block), interleaved as a complex product of (q[2i] + j q[2i+1]) with (cos + j sin) (mimi's apply_rope)."""
    B, N, _ = qkv.shape
    d, Hr = H * hd, _rope_heads(H, rot_heads)
    out = qkv.clone()
    cs = cos_sin[pos0:pos0 + N].to(qkv.dtype)
    for part in range(2):
        v = qkv[..., part * d:part * d + Hr * hd].reshape(B, N, Hr, hd)
        if interleaved:
            rot = torch.view_as_complex(cs.contiguous())[None, :, None, :]
            r = torch.view_as_real(torch.view_as_complex(v.reshape(B, N, Hr, hd // 2, 2).contiguous()) * rot).reshape(B, N, Hr, hd)
        else:
            cos, sin = torch.cat((cs[..., 0], cs[..., 0]), -1)[None, :, None], torch.cat((cs[..., 1], cs[..., 1]), -1)[None, :, None]
            r = v * cos + R._rotate_half(v) * sin
        out[..., part * d:part * d + Hr * hd] = r.reshape(B, N, Hr * hd)
    return out


# ------------------------------------------------------------------------------------------------ ISTFT head / STFT front
def istft_spec_ref(y, nb, ldS):
    """y [rows, >= 2 nb] = (log-magnitude | phase) -> [rows, ldS] = (m cos p | m sin p | 0), m = min(exp(log-magnitude), 100)."""
    y = y.to(F64)
    m, p = torch.exp(y[:, :nb]).clamp(max=100.0), y[:, nb:2 * nb]
    S = torch.zeros(y.shape[0], ldS, dtype=F64)
    S[:, :nb], S[:, nb:2 * nb] = m * torch.cos(p), m * torch.sin(p)
    return S


def istft_spec_torch(y, nb, ldS):
    """vq/heads.py's statement: clip(exp(mag), max=1e2) * (cos p + 1j sin p), in the dtype of y."""
    m, p = torch.clip(torch.exp(y[:, :nb]), max=1e2), y[:, nb:2 * nb]
    spec = m * (torch.cos(p) + 1j * torch.sin(p))
    S = torch.zeros(y.shape[0], ldS, dtype=y.dtype)
    S[:, :nb], S[:, nb:2 * nb] = spec.real, spec.imag
    return S


def stft_post_ref(ri, nb, ldo):
    """ri [rows, >= 2 nb] = (re | im) -> [rows, ldo] = (log(max(|X|, 1e-5)) | atan2(im, re) / pi | 0)."""
    ri = ri.to(F64)
    re, im = ri[:, :nb], ri[:, nb:2 * nb]
    out = torch.zeros(ri.shape[0], ldo, dtype=F64)
    out[:, :nb] = torch.log(torch.sqrt(re * re + im * im).clamp(min=1e-5))
    out[:, nb:2 * nb] = torch.atan2(im, re) / math.pi
    return out


def stft_post_torch(ri, nb, ldo):
    """The encoder front's statement: spec.abs(), spec.angle(), log(clip(mag, min=1e-5)), phase / pi, in the dtype of ri."""
    spec = torch.complex(ri[:, :nb].contiguous(), ri[:, nb:2 * nb].contiguous())
    out = torch.zeros(ri.shape[0], ldo, dtype=ri.dtype)
    out[:, :nb] = torch.log(torch.clip(spec.abs(), min=1e-5))
    out[:, nb:2 * nb] = spec.angle() / torch.pi
    return out


def istft_ola_ref(frames, win, hop, lens=None):
    """frames [B, T, n_fft] (already windowed) -> [B, T hop]: sample n of a clip of Tb frames is
    sum_t frames[t, n + pad - t hop] / sum_t win[n + pad - t hop]^2 over the frames that cover it, pad = (n_fft - hop) / 2;
    the samples behind Tb hop are 0."""
    n_fft = frames.shape[-1]
    pad = (n_fft - hop) // 2
    w2 = win.to(F64) ** 2

    def one(fb):
        Tb = fb.shape[1]
        acc = torch.zeros(fb.shape[0], (Tb - 1) * hop + n_fft, dtype=F64)
        env = torch.zeros((Tb - 1) * hop + n_fft, dtype=F64)
        for t in range(Tb):
            acc[:, t * hop:t * hop + n_fft] += fb[:, t].to(F64)
            env[t * hop:t * hop + n_fft] += w2
        return (acc / env)[:, pad:pad + Tb * hop]

    return per_clip(one, frames, lens, fill=0.0)


def istft_ola_torch(frames, win, hop, lens=None):
    """The fold / trim / envelope of the reference's ISTFT ("same" padding), in the dtype of frames."""
    n_fft = frames.shape[-1]
    pad = (n_fft - hop) // 2

    def one(fb):
        t = fb.shape[1]
        out_size = (t - 1) * hop + n_fft
        y = F.fold(fb.transpose(1, 2), output_size=(1, out_size), kernel_size=(1, n_fft), stride=(1, hop))[:, 0, 0, pad:out_size - pad]
        env = F.fold(win.to(fb.dtype).square().expand(1, t, -1).transpose(1, 2), output_size=(1, out_size), kernel_size=(1, n_fft),
                     stride=(1, hop)).reshape(-1)[pad:out_size - pad]
        return y / env

    return per_clip(one, frames, lens, fill=0.0)
