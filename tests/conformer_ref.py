"""TEST INFRASTRUCTURE ONLY - CPU restatement (float32 = the reference's arithmetic, float64 = the yardstick) of

    Model.stft_logmel                     QuarkAudio-UniSE/model/model.py:53-79
    ConformerEncoder                      model/llm/conformer.py:384-484 (eval mode: dropout off, BatchNorm running statistics)
    the condition path                    model/llm/llm.py:130-132
    CustomLlamaModel.forward / generate   model/llm/llm.py:107-147,291-374

on top of oracle/llm_ref.py's Llama body and tests/lm_score_ref.py's closed-form loss.

[upstream-memory] conformer.py:17 imports RotaryEmbedding and apply_rotary_pos_emb from `x_transformers` (pinned 2.3.1).  The package is
not available offline; `install_x_transformers()` puts a callable restatement, written from memory of that package, into sys.modules
so that the reference's own modules can be constructed and run by the pin test:
    RotaryEmbedding(dim).forward_from_seq_len(n) -> (freqs [1, n, dim] with every frequency repeated on ADJACENT channels, scale 1.0)
    apply_rotary_pos_emb(t, freqs, scale) rotates adjacent pairs (x0, x1) -> (-x1, x0) over the first freqs.shape[-1] channels.
Whether 2.3.1 pairs adjacent channels or halves cannot be verified here; `interleaved=False` restates the other pairing."""
from __future__ import annotations

import math
import sys
import types
from typing import Dict, Optional

import torch
import torch.nn.functional as F

from oracle import llm_ref as L
from tests import lm_score_ref as SR

Tensor = torch.Tensor


# ------------------------------------------------------------------------------- x_transformers restatement [upstream-memory]

class RotaryEmbedding(torch.nn.Module):
    def __init__(self, dim, base=10000):
        super().__init__()
        self.register_buffer("inv_freq", 1.0 / (base ** (torch.arange(0, dim, 2).float() / dim)))

    def forward_from_seq_len(self, seq_len):
        t = torch.arange(seq_len, device=self.inv_freq.device)
        return self.forward(t)

    def forward(self, t):
        if t.ndim == 1:
            t = t[None, :]
        freqs = torch.einsum("b i , j -> b i j", t.type_as(self.inv_freq), self.inv_freq)
        freqs = torch.stack((freqs, freqs), dim=-1).flatten(-2)  # '... d r -> ... (d r)': adjacent repetition
        return freqs, 1.0


def _rotate_adjacent(x):
    x = x.reshape(*x.shape[:-1], x.shape[-1] // 2, 2)
    x1, x2 = x.unbind(dim=-1)
    return torch.stack((-x2, x1), dim=-1).flatten(-2)


def apply_rotary_pos_emb(t, freqs, scale=1):
    rot_dim, seq_len, orig_dtype = freqs.shape[-1], t.shape[-2], t.dtype
    freqs = freqs[:, -seq_len:, :]
    if t.ndim == 4 and freqs.ndim == 3:
        freqs = freqs[:, None]
    t, t_unrotated = t[..., :rot_dim], t[..., rot_dim:]
    t = (t * freqs.cos() * scale) + (_rotate_adjacent(t) * freqs.sin() * scale)
    return torch.cat((t, t_unrotated), dim=-1).type(orig_dtype)


def install_x_transformers():
    """Make `from x_transformers.x_transformers import RotaryEmbedding, apply_rotary_pos_emb` find the restatement above."""
    pkg = types.ModuleType("x_transformers")
    sub = types.ModuleType("x_transformers.x_transformers")
    sub.RotaryEmbedding = RotaryEmbedding
    sub.apply_rotary_pos_emb = apply_rotary_pos_emb
    pkg.x_transformers = sub
    pkg.__path__ = []
    sys.modules["x_transformers"] = pkg
    sys.modules["x_transformers.x_transformers"] = sub


# ------------------------------------------------------------------------------- log-mel front

def htk_fbanks(n_freqs: int, f_min: float, f_max: float, n_mels: int, sample_rate: int, dtype=torch.float32) -> Tensor:
    """torchaudio.functional.melscale_fbanks(mel_scale="htk", norm=None) -> [n_freqs, n_mels], evaluated in `dtype`."""
    all_freqs = torch.linspace(0, sample_rate // 2, n_freqs, dtype=dtype)
    m_min, m_max = 2595.0 * math.log10(1.0 + f_min / 700.0), 2595.0 * math.log10(1.0 + f_max / 700.0)
    m_pts = torch.linspace(m_min, m_max, n_mels + 2, dtype=dtype)
    f_pts = 700.0 * (10.0 ** (m_pts / 2595.0) - 1.0)
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts.unsqueeze(0) - all_freqs.unsqueeze(1)
    down, up = -slopes[:, :-2] / f_diff[:-1], slopes[:, 2:] / f_diff[1:]
    return torch.clamp(torch.minimum(down, up), min=0.0)


def stft_logmel(x: Tensor, hop_length=320, win_length=640, n_fft=640, n_mels=80, dtype=torch.float32) -> Tensor:
    """model.py:53-79 in `dtype` (window, STFT, filter bank and log)."""
    x = x.to(dtype)
    pad_length = math.ceil(x.size(-1) / hop_length) * hop_length - x.size(-1)
    x = F.pad(x, ((win_length - hop_length) // 2, pad_length + (win_length - hop_length) // 2))
    spec = torch.stft(x, n_fft, hop_length, win_length=win_length, window=torch.hann_window(win_length, dtype=dtype), onesided=True,
                      center=False, return_complex=True).transpose(1, 2)
    fb = htk_fbanks(n_fft // 2 + 1, 0.0, 8000.0, n_mels, 16000, dtype)
    return torch.log(spec.abs() @ fb + 1e-10)


# ------------------------------------------------------------------------------- ConformerEncoder

def _rope_apply(t: Tensor, dim_head: int, interleaved: bool, dtype) -> Tensor:
    """t [b, h, n, dim_head]: rotary embedding at positions 0 .. n-1, inv_freq = 10000^(-2i / dim_head)"""
    n = t.shape[-2]
    inv = 1.0 / (10000 ** (torch.arange(0, dim_head, 2).to(dtype) / dim_head))
    fr = torch.arange(n).to(dtype)[:, None] * inv[None, :]
    if interleaved:
        fr = torch.stack((fr, fr), dim=-1).flatten(-2)
        return t * fr.cos() + _rotate_adjacent(t) * fr.sin()
    fr = torch.cat((fr, fr), dim=-1)
    h = dim_head // 2
    return t * fr.cos() + torch.cat((-t[..., h:], t[..., :h]), dim=-1) * fr.sin()


def _ff(sd, p, x):
    d = x.shape[-1]
    y = F.layer_norm(x, (d,), sd[p + ".sequential.0.weight"], sd[p + ".sequential.0.bias"], 1e-5)
    y = F.silu(F.linear(y, sd[p + ".sequential.1.weight"], sd[p + ".sequential.1.bias"]))
    return F.linear(y, sd[p + ".sequential.4.weight"], sd[p + ".sequential.4.bias"])


@torch.no_grad()
def conformer_encoder(sd: Dict[str, Tensor], params: dict, x: Tensor, mask: Optional[Tensor] = None, prefix: str = "",
                      interleaved: bool = True, dtype=torch.float32, taps: Optional[dict] = None) -> Tensor:
    """ConformerEncoder.forward(x, mask) (conformer.py:478-484) in `dtype`; taps (a dict) receives conformer.N.{ff1, attn, conv, out}."""
    sd = {k: v.to(dtype) for k, v in sd.items() if v.is_floating_point()}
    x = x.to(dtype)
    H, hd, k = params["heads"], params["dim_head"], params.get("depthwise_conv_kernel_size", 31)
    pn = params.get("pe_attn_head")
    if params.get("qk_norm") is not None:
        raise ValueError("qk_norm is not restated")
    if (k - 1) % 2 != 0:
        raise ValueError("depthwise_kernel_size must be odd to achieve 'SAME' padding.")
    b, n, d = x.shape
    for i in range(params["num_layers"]):
        p = f"{prefix}layers.{i}"
        x = _ff(sd, p + ".ff1", x) * 0.5 + x
        if taps is not None:
            taps[f"conformer.{i}.ff1"] = x.clone()
        y = F.layer_norm(x, (d,), sd[p + ".attn_norm.weight"], sd[p + ".attn_norm.bias"], 1e-5)
        q, kk, v = (F.linear(y, sd[f"{p}.attn.{nm}.weight"], sd[f"{p}.attn.{nm}.bias"]).view(b, n, H, hd).transpose(1, 2)
                    for nm in ("to_q", "to_k", "to_v"))
        if pn is not None:
            q = torch.cat([_rope_apply(q[:, :pn], hd, interleaved, dtype), q[:, pn:]], dim=1)
            kk = torch.cat([_rope_apply(kk[:, :pn], hd, interleaved, dtype), kk[:, pn:]], dim=1)
        else:
            q, kk = _rope_apply(q, hd, interleaved, dtype), _rope_apply(kk, hd, interleaved, dtype)
        w = torch.matmul(q, kk.transpose(2, 3)) / math.sqrt(hd)
        if mask is not None:
            w = w.masked_fill(~mask[:, None, None, :], float("-inf"))
        o = torch.matmul(F.softmax(w, dim=-1), v).transpose(1, 2).reshape(b, n, H * hd)
        o = F.linear(o, sd[p + ".attn.to_out.0.weight"], sd[p + ".attn.to_out.0.bias"])
        if mask is not None:
            o = o.masked_fill(~mask[..., None], 0.0)
        if taps is not None:
            taps[f"conformer.{i}.attn"] = o.clone()
        x = o + x
        cp = p + ".conv_module"
        y = F.layer_norm(x, (d,), sd[cp + ".layer_norm.weight"], sd[cp + ".layer_norm.bias"], 1e-5).transpose(1, 2)
        y = F.glu(F.conv1d(y, sd[cp + ".sequential.0.weight"], sd[cp + ".sequential.0.bias"]), dim=1)
        y = F.conv1d(y, sd[cp + ".sequential.2.weight"], sd[cp + ".sequential.2.bias"], padding=(k - 1) // 2, groups=d)
        y = F.batch_norm(y, sd[cp + ".sequential.3.running_mean"], sd[cp + ".sequential.3.running_var"], sd[cp + ".sequential.3.weight"],
                         sd[cp + ".sequential.3.bias"], False, 0.0, 1e-5)
        y = F.conv1d(F.silu(y), sd[cp + ".sequential.5.weight"], sd[cp + ".sequential.5.bias"]).transpose(1, 2)
        x = y + x
        if taps is not None:
            taps[f"conformer.{i}.conv"] = x.clone()
        x = _ff(sd, p + ".ff2", x) * 0.5 + x
        x = F.layer_norm(x, (d,), sd[p + ".final_norm.weight"], sd[p + ".final_norm.bias"], 1e-5)
        if taps is not None:
            taps[f"conformer.{i}.out"] = x.clone()
    return x


@torch.no_grad()
def condition(sd, params, cond: Tensor, interleaved=True, dtype=torch.float32, mask=None, taps=None) -> Tensor:
    """cond_output_layer(cond_encoder(cond_input_layer(cond))) (llm.py:130-132)"""
    sdd = {k: v.to(dtype) for k, v in sd.items() if v.is_floating_point() and k.startswith("cond_")}
    x = F.linear(cond.to(dtype), sdd["cond_input_layer.weight"], sdd["cond_input_layer.bias"])
    x = conformer_encoder(sdd, params, x, mask, "cond_encoder.", interleaved, dtype, taps)
    return F.linear(x, sdd["cond_output_layer.weight"], sdd["cond_output_layer.bias"])


# ------------------------------------------------------------------------------- CustomLlamaModel

def _prompt(sd, params, cond, b, interleaved, dtype):
    if cond is None:
        return None
    e = condition(sd, params, cond, interleaved, dtype)
    return torch.cat([sd["mix_sos_embedding.weight"][0].to(dtype).expand(b, 1, -1), e], dim=1)


@torch.no_grad()
def forced_logits(sd, spec: L.LMSpec, params, global_ids, semantic_ids, cond=None, interleaved=True, dtype=torch.float32):
    """llm.py:114-142: teacher-forced logits [B, Lt, V] and targets [B, Lt], Lt = G + T + 1 (the last position is dropped)."""
    inp, tgt = SR.token_ids(global_ids, semantic_ids, spec)
    inp, tgt = inp[:, :-1], tgt[:, :-1]
    lm = {k: v.to(dtype) for k, v in sd.items() if not k.startswith("cond_") and v.is_floating_point()}
    x = lm["codec_embedding.weight"][inp]
    pr = _prompt(sd, params, cond, inp.shape[0], interleaved, dtype)
    if pr is not None:
        x = torch.cat([pr, x], dim=1)
    hs = L.llm_forward(lm, x, L.KVCache(spec.n_layers), spec, dtype)[:, -tgt.shape[1]:]
    return F.linear(hs, lm["output_head.weight"]), tgt


def score(sd, spec, params, global_ids, semantic_ids, cond=None, eps=0.1, interleaved=True, dtype=torch.float32) -> dict:
    """CustomLlamaModel.forward in closed form (tests/lm_score_ref.py's row loss)."""
    z, tgt = forced_logits(sd, spec, params, global_ids, semantic_ids, cond, interleaved, dtype)
    kl = SR.row_kl(z, tgt, eps)
    am = SR.first_argmax(z)
    ok = am == tgt
    return dict(logits=z, targets=tgt, row_kl=kl, argmax=am, loss_seq=kl.mean(-1), correct=ok.sum(-1), loss=float(kl.mean()),
                acc=float(ok.double().mean()))


@torch.no_grad()
def generate(sd, spec: L.LMSpec, params, cond=None, global_length=32, semantic_length=150, batch_size=1, interleaved=True,
             forced: Optional[Tensor] = None, logits_out: Optional[list] = None, dtype=torch.float32):
    """CustomLlamaModel.generate, greedy (llm.py:291-374), batched: (global_ids [B, G], semantic_ids [B, S], tokens [B, G + S] raw ids,
    gaps [B, G + S] top-1 minus top-2 logit in the active slice).  `forced` teacher-forces the fed-back tokens (the audit protocol of
    tests/test_llm_gpu.py); note that the last global token is returned but never fed (llm.py:345)."""
    lm = {k: v.to(dtype) for k, v in sd.items() if not k.startswith("cond_") and v.is_floating_point()}
    b = batch_size if cond is None else cond.shape[0]
    cache = L.KVCache(spec.n_layers)
    pr = _prompt(sd, params, cond, b, interleaved, dtype)
    if pr is not None:
        L.llm_forward(lm, pr, cache, spec, dtype)
    toks, gaps = [], []

    def phase(first_id, steps, lo, hi):
        ids = torch.full((b,), first_id, dtype=torch.long)
        for _ in range(steps):
            hs = L.llm_forward(lm, lm["codec_embedding.weight"][ids][:, None, :], cache, spec, dtype)
            full = F.linear(hs[:, 0], lm["output_head.weight"])
            masked = torch.full_like(full, float("-inf"))
            masked[:, lo:hi] = full[:, lo:hi]
            if logits_out is not None:
                logits_out.append(masked.clone())
            top2 = masked.topk(2, dim=-1).values
            nxt = SR.first_argmax(masked)
            toks.append(nxt)
            gaps.append(top2[:, 0] - top2[:, 1])
            ids = nxt if forced is None else forced[:, len(toks) - 1]

    phase(0, global_length, spec.global_offset, spec.global_offset + spec.global_size)
    phase(1, semantic_length, spec.semantic_offset, spec.semantic_offset + spec.semantic_size)
    tokens = torch.stack(toks, dim=1)
    return (tokens[:, :global_length] - spec.global_offset, tokens[:, global_length:] - spec.semantic_offset, tokens, torch.stack(gaps, dim=1))


# ------------------------------------------------------------------------------- golden cases (tools/gen_golden_lm_cond.py)

# Inputs are regenerated from seeds on both machines (unified_audio_amd/synth.py); tests/golden/lm_cond_*.npz store what the reference's
# OWN classes computed from them.
GOLDEN_CF = dict(num_layers=2, dim=64, heads=2, dim_head=32, depthwise_conv_kernel_size=31, ff_mult=2, dropout=0.1, qk_norm=None,
                 pe_attn_head=None)
GOLDEN_SPEC = SR.SMALL  # the size class of lm_score_small_*
GOLDEN_G, GOLDEN_S, GOLDEN_B, GOLDEN_T = 6, 14, 3, 20
# name -> (pe_attn_head, masked)
CONFORMER_CASES = {"pe_none": (None, False), "pe_1": (1, False), "pe_1_ragged_mask": (1, True)}
# name -> (with condition, label smoothing)
FORWARD_CASES = {"cond_eps01": (True, 0.1), "cond_eps0": (True, 0.0), "nocond_eps01": (False, 0.1), "nocond_eps0": (False, 0.0)}


def golden_conformer_case(name: str):
    """(params, state_dict, x [3, 50, 64], mask or None)"""
    import numpy as np

    from unified_audio_amd import synth

    pe, masked = CONFORMER_CASES[name]
    params = dict(GOLDEN_CF, pe_attn_head=pe)
    x = torch.from_numpy(np.random.default_rng(3).standard_normal((3, 50, 64)).astype("float32"))
    mask = (torch.arange(50)[None, :] < torch.tensor([50, 33, 41])[:, None]) if masked else None
    return params, synth.conformer_state_dict(31, params), x, mask


def golden_logmel_wav() -> Tensor:
    """seeded noise [3, 16123] (not a multiple of the hop) with one all-zero stretch in item 1"""
    from unified_audio_amd import synth

    wav = synth.synth_wav(5, 3, 16123).clone()
    wav[1, 3000:9000] = 0.0
    return wav


def golden_lm_weights():
    from unified_audio_amd import synth

    sd = {k: v for k, v in L.lm_state_dict(71, GOLDEN_SPEC).items() if not k.startswith(("task_embedding", "enroll_sos", "adapter"))}
    sd.update(synth.cond_encoder_state_dict(72, 80, GOLDEN_SPEC.hidden, GOLDEN_CF, 2.0))
    return sd


def golden_lm_inputs():
    """(cond [B, T, 80], global_ids [B, G], semantic_ids [B, S]) of the forward cases; generate uses cond alone"""
    from unified_audio_amd import synth

    gen = torch.Generator().manual_seed(17)
    g = torch.randint(0, GOLDEN_SPEC.global_size, (GOLDEN_B, GOLDEN_G), generator=gen)
    s = torch.randint(0, GOLDEN_SPEC.semantic_size, (GOLDEN_B, GOLDEN_S), generator=gen)
    return synth.synth_logmel(11, GOLDEN_B, GOLDEN_T), g, s


def load_golden(name: str):
    import os

    import numpy as np

    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".npz")
    return {k: torch.from_numpy(v) for k, v in np.load(path).items()}
