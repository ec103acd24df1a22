"""TEST INFRASTRUCTURE ONLY - CPU restatement (plain PyTorch, any float dtype: fp64 for the GPU parity tests) of what `BiCodec.forward`
(QuarkAudio-UniSE/model/bicodec/bicodec.py:113-149, eval mode) adds to tokenize and detokenize:

    x-vector head        speaker/ecapa_tdnn.py:204-206, speaker/pooling_layers.py:119-144 (ASTP, global_context_att=True)
    postnet              encoder_decoder/feat_decoder.py:79-96 without condition, on the prenet output BEFORE the d-vector add
    code statistics      vq/factorized_vector_quantize.py:98-103 (perplexity, active_num), eval vq_loss = NaN (:121-131)

The rest comes from tests/bicodec_tokenize_ref.py (semantic / global tokens, mel, ECAPA latent) and oracle/bicodec_ref.py (z_q, d-vector,
prenet).  PINNED: tests/test_bicodec_forward_oracle_cpu.py runs the reference's own modules against it.  Nothing in the product path
imports it.
"""
from __future__ import annotations

import math
from typing import Dict

import torch
import torch.nn.functional as F

from oracle import bicodec_ref as BR
from tests import bicodec_tokenize_ref as T

SD = Dict[str, torch.Tensor]
HEAD = "speaker_encoder.speaker_encoder"


def astp(sd: SD, latent: torch.Tensor) -> torch.Tensor:
    """ASTP with global_context_att=True (ECAPA_TDNN_GLOB_c512): latent [B, T, 1536] -> [B, 3072] = cat(mean, std) of the
    attention-weighted frames; the attention sees each frame next to the plain mean and (unbiased) std of all frames."""
    x = latent.transpose(1, 2)
    context_mean = torch.mean(x, dim=-1, keepdim=True).expand_as(x)
    context_std = torch.sqrt(torch.var(x, dim=-1, keepdim=True) + 1e-7).expand_as(x)
    x_in = torch.cat((x, context_mean, context_std), dim=1)
    alpha = torch.tanh(F.conv1d(x_in, sd[HEAD + ".pool.linear1.weight"], sd[HEAD + ".pool.linear1.bias"]))
    alpha = torch.softmax(F.conv1d(alpha, sd[HEAD + ".pool.linear2.weight"], sd[HEAD + ".pool.linear2.bias"]), dim=2)
    mean = torch.sum(alpha * x, dim=2)
    var = torch.sum(alpha * (x ** 2), dim=2) - mean ** 2
    std = torch.sqrt(var.clamp(min=1e-7))
    return torch.cat([mean, std], dim=1)


def x_vector(sd: SD, latent: torch.Tensor, taps=None) -> torch.Tensor:
    """ECAPA_TDNN.forward's output from its latent: Linear(BatchNorm1d(ASTP(latent)))."""
    pool = astp(sd, latent)
    if taps is not None:
        taps["ecapa.pool"] = pool
    return F.linear(T._bn(sd, HEAD + ".bn", pool), sd[HEAD + ".linear.weight"], sd[HEAD + ".linear.bias"])


def postnet(sd: SD, x: torch.Tensor, vocos_layers: int, use_tanh_at_final: bool = False) -> torch.Tensor:
    """Decoder.forward without condition, sample_ratios [1, 1]: x [B, latent, N] -> [B, out_channels, N]."""
    y = F.linear(x.transpose(1, 2), sd["postnet.linear_pre.weight"], sd["postnet.linear_pre.bias"])       # [B, N, C]
    for i in range(2):
        y = 3.0 * y.transpose(1, 2)  # SamplingBlock with both scales 1 (samper.py:78-95)
        y = BR.vocos_backbone(sd, f"postnet.downsample.{i}.1", y, 2)
    y = BR.vocos_backbone(sd, "postnet.vocos_backbone", y.transpose(1, 2), vocos_layers)
    y = F.linear(y, sd["postnet.linear.weight"], sd["postnet.linear.bias"]).transpose(1, 2)
    return torch.tanh(y) if use_tanh_at_final else y


def d_vector(sd: SD, global_tokens: torch.Tensor, spec) -> torch.Tensor:
    """SpeakerEncoder.detokenize (oracle.bicodec_ref.global_detokenize) with the FSQ codes in the weights' dtype: [B, latent]."""
    B = global_tokens.shape[0]
    codes = BR.fsq_codes(global_tokens.reshape(B, -1).long(), spec.fsq_levels).to(sd["speaker_encoder.project.weight"].dtype)
    zq = F.linear(codes, sd["speaker_encoder.quantizer.project_out.weight"], sd["speaker_encoder.quantizer.project_out.bias"])
    return F.linear(zq.transpose(1, 2).reshape(B, -1), sd["speaker_encoder.project.weight"], sd["speaker_encoder.project.bias"])


def prenet_out(sd: SD, semantic_tokens: torch.Tensor, global_tokens: torch.Tensor, spec) -> torch.Tensor:
    """The prenet output of detokenize's tokens, before the d-vector add: [B, latent, N]."""
    z_q = BR.semantic_detokenize(sd, semantic_tokens)
    d = d_vector(sd, global_tokens, spec)
    return BR.prenet(sd, z_q, d, spec)


def pred_feat(sd: SD, semantic_tokens: torch.Tensor, global_tokens: torch.Tensor, spec, vocos_layers: int, dtype=torch.float64,
              use_tanh_at_final: bool = False) -> torch.Tensor:
    """postnet(prenet(z_q(tokens), d(tokens))) in `dtype`."""
    sdd = T.cast(sd, dtype)
    with torch.no_grad():
        return postnet(sdd, prenet_out(sdd, semantic_tokens, global_tokens, spec), vocos_layers, use_tanh_at_final)


def code_stats(indices: torch.Tensor, codebook_size: int, dtype=torch.float64):
    """(perplexity, active_num) of all the indices of a batch, as FactorizedVectorQuantize.forward computes them."""
    onehot = F.one_hot(indices.reshape(-1), codebook_size).to(dtype)
    avg_probs = torch.mean(onehot, dim=0)
    perplexity = torch.exp(-torch.sum(avg_probs * torch.log(avg_probs + 1e-10)))
    return perplexity, (onehot.sum(0) > 0).sum().to(dtype)


def perplexity_exact(indices: torch.Tensor, codebook_size: int) -> float:
    """exp(entropy) of the code histogram in Python floats (math.fsum), for the bound of the fp32 / fp64 variants."""
    counts = torch.bincount(indices.reshape(-1), minlength=codebook_size).tolist()
    n = sum(counts)
    return math.exp(-math.fsum((c / n) * math.log(c / n + 1e-10) for c in counts if c))
