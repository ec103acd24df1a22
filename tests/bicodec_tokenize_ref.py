"""TEST INFRASTRUCTURE ONLY - CPU restatement (plain PyTorch, any float dtype: fp64 for the GPU parity tests) of the semantic half of
`BiCodec.tokenize` and of the feature normalisation in front of it:

    Wav2Vec2FeatureExtractor normalisation   audio_tokenizer.py:74-90 (transformers zero_mean_unit_var_norm, nothing padded)
    BiCodec.get_semantic_tokens              model/bicodec/bicodec.py:167-172
    Encoder.forward                          modules/encoder_decoder/feat_encoder.py:29-92   Vocos 1024 -> 384, 2 x (3 x, Vocos), Linear
    FactorizedVectorQuantize.tokenize        modules/vq/factorized_vector_quantize.py:148-152,169-187

PINNED: tests/test_bicodec_tokenize_oracle_cpu.py runs the reference's own modules against this restatement (identical tokens at small
and published widths) and the transformers feature extractor against `wav_normalize`.  Nothing in the product path imports it.
"""
from __future__ import annotations

import math
from typing import Dict

import torch
import torch.nn.functional as F

from oracle.bicodec_ref import _wn, vocos_backbone

SD = Dict[str, torch.Tensor]


def cast(sd: SD, dtype=torch.float64) -> SD:
    return {k: v.to(dtype) if v.is_floating_point() else v for k, v in sd.items()}


def wav_normalize(wav: torch.Tensor, eps: float = 1e-7) -> torch.Tensor:
    """(x - mean) / sqrt(var + eps) per row, population variance."""
    mean = wav.mean(-1, keepdim=True)
    var = (wav - mean).pow(2).mean(-1, keepdim=True)
    return (wav - mean) / torch.sqrt(var + eps)


def encoder(sd: SD, feat: torch.Tensor, vocos_layers: int, taps=None) -> torch.Tensor:
    """Encoder.forward with sample_ratios [1, 1]: feat [B, N, C_in] -> z [B, N, latent] (the reference returns [B, latent, N])."""
    x = vocos_backbone(sd, "encoder.encoder", feat.transpose(1, 2), vocos_layers)                 # [B, N, C]
    if taps is not None:
        taps["enc.backbone"] = x
    for i in range(2):
        x = 3.0 * x.transpose(1, 2)  # SamplingBlock with both scales 1: conv_res + skip1_res + skip2_res = 3 x (samper.py:78-95)
        x = vocos_backbone(sd, f"encoder.downsample.{i}.1", x, 2)
    if taps is not None:
        taps["enc.down"] = x
    z = F.linear(x, sd["encoder.project.weight"], sd["encoder.project.bias"])
    if taps is not None:
        taps["enc.out"] = z
    return z


def normalized_codebook(sd: SD) -> torch.Tensor:
    return F.normalize(sd["quantizer.codebook.weight"])


def quantize(sd: SD, z: torch.Tensor, taps=None) -> torch.Tensor:
    """FactorizedVectorQuantize.tokenize: z [B, N, latent] -> indices [B, N] int64 (first index wins a tie)."""
    B, N, _ = z.shape
    ze = F.conv1d(z.transpose(1, 2), _wn(sd, "quantizer.in_project"), sd["quantizer.in_project.bias"])  # [B, D, N]
    e = F.normalize(ze.transpose(1, 2).reshape(B * N, -1))
    if taps is not None:
        taps["vq.latent"] = e
    cb = normalized_codebook(sd)
    dist = e.pow(2).sum(1, keepdim=True) - 2 * e @ cb.t() + cb.pow(2).sum(1, keepdim=True).t()
    return (-dist).max(1)[1].reshape(B, N)


@torch.no_grad()
def get_semantic_tokens(sd: SD, feat: torch.Tensor, vocos_layers: int, taps=None) -> torch.Tensor:
    return quantize(sd, encoder(sd, feat, vocos_layers, taps), taps)


# ---------------------------------------------------------------- global tokens (bicodec.py:174-178, audio_tokenizer.py:54-72)

SPK = "speaker_encoder"


def ref_clip(wav: torch.Tensor, ref_len: int) -> torch.Tensor:
    """BiCodecTokenizer.get_ref_clip: tile a short row, then truncate to ref_len."""
    if ref_len > wav.shape[-1]:
        wav = torch.tile(wav, (1, ref_len // wav.shape[-1] + 1))
    return wav[:, :ref_len]


def _hz_to_mel(f):  # slaney scale (torchaudio.functional._hz_to_mel, mel_scale="slaney")
    f_sp, min_log_hz, min_log_mel, logstep = 200.0 / 3, 1000.0, 15.0, math.log(6.4) / 27.0
    return min_log_mel + math.log(f / min_log_hz) / logstep if f >= min_log_hz else f / f_sp


def _mel_to_hz(m: torch.Tensor) -> torch.Tensor:
    f_sp, min_log_hz, min_log_mel, logstep = 200.0 / 3, 1000.0, 15.0, math.log(6.4) / 27.0
    return torch.where(m >= min_log_mel, min_log_hz * torch.exp(logstep * (m - min_log_mel)), f_sp * m)


def mel_filterbank(n_fft: int, n_mels: int, sample_rate: int, f_min: float, f_max, dtype=torch.float64) -> torch.Tensor:
    """torchaudio.functional.melscale_fbanks(norm="slaney", mel_scale="slaney"): triangles in Hz between mel-spaced edges,
    area-normalised.  [n_fft // 2 + 1, n_mels]."""
    f_max = float(sample_rate // 2) if f_max is None else float(f_max)
    all_freqs = torch.linspace(0, sample_rate // 2, n_fft // 2 + 1, dtype=dtype)
    m_pts = torch.linspace(_hz_to_mel(float(f_min)), _hz_to_mel(f_max), n_mels + 2, dtype=dtype)
    f_pts = _mel_to_hz(m_pts)
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts.unsqueeze(0) - all_freqs.unsqueeze(1)
    down = -slopes[:, :-2] / f_diff[:-1]
    up = slopes[:, 2:] / f_diff[1:]
    fb = torch.clamp(torch.minimum(down, up), min=0)
    return fb * (2.0 / (f_pts[2:n_mels + 2] - f_pts[:n_mels])).unsqueeze(0)


def mel_spectrogram(wav: torch.Tensor, mel: dict) -> torch.Tensor:
    """torchaudio MelSpectrogram(power=1, center=True, reflect pad, periodic Hann of win_length centred in n_fft, no log):
    wav [B, T] -> [B, frames, n_mels] (the reference's [B, n_mels, frames] transposed, as SpeakerEncoder.tokenize takes it)."""
    window = torch.hann_window(mel["win_length"], periodic=True, dtype=wav.dtype)
    spec = torch.stft(wav, mel["n_fft"], mel["hop_length"], mel["win_length"], window, center=True, pad_mode="reflect",
                      return_complex=True).abs()
    fb = mel_filterbank(mel["n_fft"], mel["num_mels"], mel["sample_rate"], mel["mel_fmin"], mel.get("mel_fmax"), wav.dtype)
    return spec.transpose(1, 2) @ fb


def _bn(sd: SD, p: str, x: torch.Tensor) -> torch.Tensor:  # BatchNorm1d in eval mode
    return F.batch_norm(x, sd[p + ".running_mean"], sd[p + ".running_var"], sd[p + ".weight"], sd[p + ".bias"], False, 0.0, 1e-5)


def _conv_relu_bn(sd: SD, p: str, x: torch.Tensor, pad: int = 0) -> torch.Tensor:  # Conv1dReluBn: BN(ReLU(conv))
    return _bn(sd, p + ".bn", F.relu(F.conv1d(x, sd[p + ".conv.weight"], sd[p + ".conv.bias"], padding=pad)))


def _se_res2_block(sd: SD, p: str, x: torch.Tensor, dilation: int, scale: int = 8) -> torch.Tensor:
    """SE_Res2Block: x + SE(Conv1dReluBn(Res2Conv1dReluBn(Conv1dReluBn(x))))."""
    y = _conv_relu_bn(sd, p + ".0", x)
    spx = torch.split(y, y.shape[1] // scale, 1)
    out, sp = [], spx[0]
    for i in range(scale - 1):  # a sequential chain: each conv takes the previous output plus the next split
        if i >= 1:
            sp = sp + spx[i]
        sp = F.conv1d(sp, sd[f"{p}.1.convs.{i}.weight"], sd[f"{p}.1.convs.{i}.bias"], padding=dilation, dilation=dilation)
        sp = _bn(sd, f"{p}.1.bns.{i}", F.relu(sp))
        out.append(sp)
    out.append(spx[scale - 1])
    y = _conv_relu_bn(sd, p + ".2", torch.cat(out, 1))
    g = F.relu(F.linear(y.mean(2), sd[p + ".3.linear1.weight"], sd[p + ".3.linear1.bias"]))
    g = torch.sigmoid(F.linear(g, sd[p + ".3.linear2.weight"], sd[p + ".3.linear2.bias"]))
    return x + y * g.unsqueeze(2)


def ecapa_latent(sd: SD, mel: torch.Tensor, taps=None) -> torch.Tensor:
    """ECAPA_TDNN.forward(mel, return_latent=True)[1]: mel [B, T, n_mels] -> latent [B, T, 1536] (the reference's [B, 1536, T])."""
    p = SPK + ".speaker_encoder"
    out1 = _conv_relu_bn(sd, p + ".layer1", mel.transpose(1, 2), pad=2)
    out2 = _se_res2_block(sd, p + ".layer2.se_res2block", out1, 2)
    out3 = _se_res2_block(sd, p + ".layer3.se_res2block", out2, 3)
    out4 = _se_res2_block(sd, p + ".layer4.se_res2block", out3, 4)
    latent = F.relu(F.conv1d(torch.cat([out2, out3, out4], 1), sd[p + ".conv.weight"], sd[p + ".conv.bias"]))
    if taps is not None:
        for i, o in enumerate((out1, out2, out3, out4)):
            taps[f"ecapa.layer{i + 1}"] = o.transpose(1, 2)
        taps["ecapa.latent"] = latent.transpose(1, 2)
    return latent.transpose(1, 2)


def perceiver(sd: SD, x: torch.Tensor, depth: int = 2, heads: int = 8, dim_head: int = 64) -> torch.Tensor:
    """PerceiverResampler.forward: x [B, T, dim_context] -> [B, num_latents, dim]."""
    p = SPK + ".perceiver_sampler"
    x = F.linear(x, sd[p + ".proj_context.weight"], sd[p + ".proj_context.bias"])
    B = x.shape[0]
    lat = sd[p + ".latents"].unsqueeze(0).expand(B, -1, -1)
    split = lambda t: t.reshape(B, t.shape[1], heads, dim_head).transpose(1, 2)  # noqa: E731
    for i in range(depth):
        q = f"{p}.layers.{i}"
        ctx = torch.cat((lat, x), dim=-2)  # cross_attn_include_queries
        k, v = F.linear(ctx, sd[q + ".0.to_kv.weight"]).chunk(2, dim=-1)
        sim = split(F.linear(lat, sd[q + ".0.to_q.weight"])) @ split(k).transpose(-1, -2) * dim_head ** -0.5
        o = (sim.softmax(-1) @ split(v)).transpose(1, 2).reshape(B, lat.shape[1], heads * dim_head)
        lat = F.linear(o, sd[q + ".0.to_out.weight"]) + lat
        a, gate = F.linear(lat, sd[q + ".1.0.weight"], sd[q + ".1.0.bias"]).chunk(2, dim=-1)
        lat = F.linear(F.gelu(gate) * a, sd[q + ".1.2.weight"], sd[q + ".1.2.bias"]) + lat
    return F.normalize(lat, dim=-1) * lat.shape[-1] ** 0.5 * sd[p + ".norm.gamma"]


def fsq(sd: SD, x: torch.Tensor, levels, taps=None) -> torch.Tensor:
    """ResidualFSQ with one quantizer (scale 1): project_in -> bound -> round half to even -> index. x [B, n, dim] -> int32 [B, n]."""
    z = F.linear(x, sd[SPK + ".quantizer.project_in.weight"], sd[SPK + ".quantizer.project_in.bias"])
    L = torch.tensor(levels, dtype=z.dtype)
    half_l = (L - 1) * (1 + 1e-3) / 2
    offset = torch.where(torch.tensor(levels) % 2 == 0, 0.5, 0.0).to(z.dtype)
    bounded = torch.tanh(z + torch.atanh(offset / half_l)) * half_l - offset
    if taps is not None:
        taps["fsq.bounded"] = bounded
    basis = torch.cumprod(torch.tensor([1] + list(levels[:-1]), dtype=torch.int64), 0)
    digits = torch.round(bounded).to(torch.int64) + torch.tensor(levels, dtype=torch.int64) // 2
    return (digits * basis).sum(-1).to(torch.int32)


@torch.no_grad()
def get_global_tokens(sd: SD, ref_wav: torch.Tensor, mel: dict, levels, depth=2, heads=8, dim_head=64, taps=None) -> torch.Tensor:
    """BiCodec.get_global_tokens: ref_wav [B, T] -> int32 [B, token_num] (the reference's [B, 1, token_num])."""
    m = mel_spectrogram(ref_wav, mel)
    if taps is not None:
        taps["mel"] = m
    lat = perceiver(sd, ecapa_latent(sd, m, taps), depth, heads, dim_head)
    if taps is not None:
        taps["perceiver.out"] = lat
    return fsq(sd, lat, levels, taps)
