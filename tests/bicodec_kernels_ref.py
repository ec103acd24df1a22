"""TEST INFRASTRUCTURE ONLY - one plain-PyTorch restatement per kernel of csrc/bicodec_kernels.hip, on plain tensors with the weights
as arguments and laid out as the kernels read them:

    wt  [7][3][W_in][W_out]   the seven width-W dilated k = 3 convolutions of a Res2 chain (step, tap, in, out)
    bst [7][3][W]             per step: convolution bias, BatchNorm scale, BatchNorm shift (eval mode, folded to y = v * s + t)
    w1t [C][Hd], w2t [Hd][C]  the two SE Linears, transposed

Every float operation takes `dtype=`: float64 is the truth of tests/test_bicodec_kernels_gpu.py, the same function in float32 on the CPU
its yardstick.  The pure moves (gathers, the two tails, mel framing, the perceiver context, the widening copy) are index arithmetic and
keep the dtype of what they move.  PINNED: tests/test_bicodec_kernels_ref_cpu.py holds every one of them, in float64, against the
model-level restatements the reference's own modules were run against (tests/bicodec_tokenize_ref.py, tests/bicodec_forward_ref.py) and
against torch's operators.  Nothing in the product path imports this file.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

BN_EPS = 1e-5  # BatchNorm1d's default, as csrc/bicodec.cpp folds it


# ------------------------------------------------------------------------------------------------------------ weight layouts
def fold_bn(weight, bias, mean, var, eps=BN_EPS):
    """BatchNorm1d in eval mode as y = v * s + t."""
    s = weight / torch.sqrt(var + eps)
    return s, bias - mean * s


def pack_res2(sd, p, dtype=torch.float64):
    """The state-dict entries {p}.convs.i.* / {p}.bns.i.* of a Res2Conv1dReluBn -> (wt [7, 3, W, W], bst [7, 3, W])."""
    wt, bst = [], []
    for i in range(7):
        w = sd[f"{p}.convs.{i}.weight"].to(dtype)  # [W_out, W_in, 3]
        s, t = fold_bn(*(sd[f"{p}.bns.{i}.{k}"].to(dtype) for k in ("weight", "bias", "running_mean", "running_var")))
        wt.append(w.permute(2, 1, 0))
        bst.append(torch.stack((sd[f"{p}.convs.{i}.bias"].to(dtype), s, t)))
    return torch.stack(wt).contiguous(), torch.stack(bst).contiguous()


def pack_se(sd, p, dtype=torch.float64):
    """{p}.linear1 / linear2 of an SE_Connect -> (w1t [C, Hd], b1 [Hd], w2t [Hd, C], b2 [C])."""
    return (sd[p + ".linear1.weight"].to(dtype).t().contiguous(), sd[p + ".linear1.bias"].to(dtype),
            sd[p + ".linear2.weight"].to(dtype).t().contiguous(), sd[p + ".linear2.bias"].to(dtype))


# ------------------------------------------------------------------------------------------------------------ pure moves
def gather_rows_ref(tok, table, T=0, lens=None):
    """tok [n] int64, table [V, D] -> [n, D] = table[clamp(tok)]; with lens, row b * T + t is zeros for t >= lens[b]."""
    out = table[tok.clamp(0, table.shape[0] - 1)]
    if lens is not None:
        t = torch.arange(tok.numel()) % T
        b = torch.arange(tok.numel()) // T
        out = torch.where((t < torch.as_tensor(lens)[b])[:, None], out, torch.zeros_like(out))
    return out


def gather_global_ref(tok, table):
    """tok [B, N], table [V, L] -> out[b, c * N + n] = table[clamp(tok[b, n]), c]."""
    zq = table[tok.clamp(0, table.shape[0] - 1)]  # [B, N, L]
    return zq.transpose(1, 2).reshape(tok.shape[0], -1)


def tokens_fill_behind_ref(tok, lens):
    """tok [B, N]: -1 at n >= lens[b]."""
    n = torch.arange(tok.shape[1])[None]
    return torch.where(n < torch.as_tensor(lens)[:, None], tok, torch.full_like(tok, -1))


def zero_behind_ref(x, lens, mul):
    """x [B, T]: 0 at t >= lens[b] * mul."""
    t = torch.arange(x.shape[1])[None]
    return torch.where(t < torch.as_tensor(lens)[:, None] * mul, x, torch.zeros_like(x))


def mel_frames_ref(wav, ref_len, hop, n_frames, lens=None):
    """wav [B, T] -> P [B, (n_frames + 1) * hop]: P[b, i] = clip_b(i - hop), the reference clip (the row's first lens[b] samples, tiled
    and cut to ref_len) under torch.stft's reflect padding of hop samples."""
    B, T = wav.shape
    k = torch.arange((n_frames + 1) * hop) - hop
    k = torch.where(k < 0, -k, torch.where(k >= ref_len, 2 * (ref_len - 1) - k, k))
    return torch.stack([wav[b, k % (T if lens is None else int(lens[b]))] for b in range(B)])


def perceiver_ctx_ref(ctx, lat, x, T):
    """ctx [B, n_lat + T, D] with its latent rows replaced by lat ([n_lat, D]: the learned latents, broadcast; [B, n_lat, D]: per item)
    and, when x [B, T, D] is given, its other rows by x.  x = None leaves them as they are."""
    out = ctx.clone()
    n_lat = lat.shape[-2]
    out[:, :n_lat] = lat
    if x is not None:
        out[:, n_lat:] = x
    return out


# ------------------------------------------------------------------------------------------------------------ row operations
def adaln_ref(x, scale, shift, eps, dtype=torch.float64):
    """x [B, T, C], scale / shift [B, C]: LayerNorm without affine (biased variance), times scale[b] plus shift[b]."""
    x, scale, shift = x.to(dtype), scale.to(dtype), shift.to(dtype)
    mean = x.mean(-1, keepdim=True)
    var = (x - mean).pow(2).mean(-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps) * scale[:, None] + shift[:, None]


def add_rowvec_ref(x, v, dtype=torch.float64):
    """x [B, T, C] + v [B, C]."""
    return x.to(dtype) + v.to(dtype)[:, None]


def l2norm_rows_ref(x, dtype=torch.float64):
    """x / max(||x||_2, 1e-12) per row."""
    x = x.to(dtype)
    return x / x.pow(2).sum(-1, keepdim=True).sqrt().clamp_min(1e-12)


def l2norm_scale_ref(x, gamma, scale, dtype=torch.float64):
    """The perceiver's RMSNorm: x / max(||x||, 1e-12) * scale * gamma."""
    return l2norm_rows_ref(x, dtype) * scale * gamma.to(dtype)


def spec_mag_ref(ri, nbp, nb, ldm, dtype=torch.float64):
    """ri [rows, 2 nbp] = [re | im] -> [rows, ldm]: sqrt(re^2 + im^2) of the first nb bins, zeros behind."""
    ri = ri.to(dtype)
    out = torch.zeros(ri.shape[0], ldm, dtype=dtype)
    out[:, :nb] = torch.sqrt(ri[:, :nb].pow(2) + ri[:, nbp:nbp + nb].pow(2))
    return out


def geglu_ref(h, Fh, ldo, dtype=torch.float64):
    """h [rows, 2 F] = [x | gate] -> [rows, ldo]: gelu_erf(gate) * x in the first F columns, zeros behind."""
    h = h.to(dtype)
    out = torch.zeros(h.shape[0], ldo, dtype=dtype)
    z = h[:, Fh:2 * Fh]
    out[:, :Fh] = 0.5 * z * (1.0 + torch.erf(z * 0.5 ** 0.5)) * h[:, :Fh]
    return out


def wav_normalize_ref(wav, eps, lens=None, dtype=torch.float64):
    """wav [B, T]: (x - mean) / sqrt(var + eps) over each row's first lens[b] samples (population variance), zeros behind."""
    wav = wav.to(dtype)
    out = torch.zeros_like(wav)
    for b in range(wav.shape[0]):
        n = wav.shape[1] if lens is None else int(lens[b])
        r = wav[b, :n]
        mean = r.mean()
        out[b, :n] = (r - mean) / torch.sqrt((r - mean).pow(2).mean() + eps)
    return out


# ------------------------------------------------------------------------------------------------------------ ECAPA pieces
def res2_chain_ref(x, wt, bst, d, dtype=torch.float64):
    """x [B, T, C] (time-major) -> y [B, T, C]: split j < 7 is sp_j = BN(ReLU(conv_j(sp_{j-1} + x_j))) with sp_0 = BN(ReLU(conv_0(x_0))),
    dilation and zero padding d; split 7 is x_7."""
    x, wt, bst = x.to(dtype), wt.to(dtype), bst.to(dtype)
    W = x.shape[-1] // 8
    spx = torch.split(x.transpose(1, 2), W, 1)
    out, sp = [], None
    for i in range(7):
        sp = spx[i] if i == 0 else sp + spx[i]
        sp = F.conv1d(sp, wt[i].permute(2, 1, 0), bst[i, 0], padding=d, dilation=d)  # [3, in, out] -> [out, in, 3]
        sp = F.relu(sp) * bst[i, 1][:, None] + bst[i, 2][:, None]
        out.append(sp)
    out.append(spx[7])
    return torch.cat(out, 1).transpose(1, 2)


def se_gate_ref(y, w1t, b1, w2t, b2, dtype=torch.float64):
    """y [B, T, C] -> gate [B, C] = sigmoid(relu(mean_t(y) w1t + b1) w2t + b2)."""
    y, w1t, b1, w2t, b2 = (t.to(dtype) for t in (y, w1t, b1, w2t, b2))
    return torch.sigmoid(F.relu(y.mean(1) @ w1t + b1) @ w2t + b2)


def se_residual_ref(x, y, w1t, b1, w2t, b2, dtype=torch.float64):
    """(gate [B, C], out [B, T, C] = x + y * gate)."""
    g = se_gate_ref(y, w1t, b1, w2t, b2, dtype)
    return g, x.to(dtype) + y.to(dtype) * g[:, None]


# ------------------------------------------------------------------------------------------------------------ FSQ
def fsq_ref(x, w, bias, levels, dtype=torch.float64):
    """x [rows, D], w [nl, D], bias [nl] -> (bounded [rows, nl] in dtype, digits [rows, nl] int64, tokens [rows] int64): z = x w^T + b,
    bounded = tanh(z + atanh(offset / half_l)) half_l - offset, digit = round_half_even(bounded) + L // 2, token = sum digit * basis
    with basis the running product of the levels in front."""
    z = x.to(dtype) @ w.to(dtype).t() + bias.to(dtype)
    Li = torch.tensor(levels, dtype=torch.int64)
    half_l = (Li.to(dtype) - 1) * (1 + 1e-3) / 2
    offset = torch.where(Li % 2 == 0, 0.5, 0.0).to(dtype)
    bounded = torch.tanh(z + torch.atanh(offset / half_l)) * half_l - offset
    digits = torch.round(bounded).to(torch.int64) + Li // 2
    basis = torch.cumprod(torch.tensor([1] + list(levels[:-1]), dtype=torch.int64), 0)
    return bounded, digits, (digits * basis).sum(-1)


def fsq_digits_of(tokens, levels):
    """tokens [rows] -> the mixed-radix digits [rows, nl], lowest level first."""
    t = tokens.to(torch.int64)
    out = []
    for L in levels:
        out.append(t % L)
        t = t // L
    return torch.stack(out, -1)


# ------------------------------------------------------------------------------------------------------------ x-vector head, statistics
def astp_pool_ref(logit, x, bn_s, bn_t, dtype=torch.float64):
    """logit / x [B, T, C], bn_s / bn_t [2 C] -> (pool [B, 2 C], bn [B, 2 C]): alpha = softmax over T, mean = sum alpha x,
    std = sqrt(max(sum alpha x^2 - mean^2, 1e-7)); pool = cat(mean, std), bn = pool * bn_s + bn_t."""
    logit, x = logit.to(dtype), x.to(dtype)
    alpha = torch.softmax(logit, dim=1)
    mean = (alpha * x).sum(1)
    var = (alpha * x.pow(2)).sum(1) - mean.pow(2)
    pool = torch.cat((mean, torch.sqrt(var.clamp(min=1e-7))), 1)
    return pool, pool * bn_s.to(dtype) + bn_t.to(dtype)


def frame_stats_ref(x, dtype=torch.float64):
    """x [B, T, C] -> [B, 2 C] = cat(mean_t, sqrt(unbiased var_t + 1e-7)); T = 1 gives NaN in the second half, as torch.var does."""
    x = x.to(dtype)
    T = x.shape[1]
    mean = x.sum(1) / T
    var = (x - mean[:, None]).pow(2).sum(1) / (T - 1) if T > 1 else torch.full_like(mean, float("nan"))
    return torch.cat((mean, torch.sqrt(var + 1e-7)), 1)


def code_usage_ref(idx, K, dtype=torch.float64):
    """(perplexity, active) over ALL n indices: p_k = count_k / n with only the indices inside [0, K) counted."""
    idx = idx.reshape(-1)
    counts = torch.bincount(idx[(idx >= 0) & (idx < K)], minlength=K)
    p = counts.to(dtype) / idx.numel()
    return torch.exp(-(p * torch.log(p + 1e-10)).sum()), (counts > 0).sum().to(dtype)
