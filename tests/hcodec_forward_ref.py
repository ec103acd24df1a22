"""CPU restatement of H-Codec's Codec.forward in eval mode, on top of the oracle's encode / decode restatements.

    semantic_decoder  <-> semantic_module.Decoder            QuarkAudio-HCodec/HCodec-1.0/vq/semantic_module.py:205-300
    forward10         <-> Codec.forward (1.0)                QuarkAudio-HCodec/HCodec-1.0/vq/codec.py:138-162
    forward15         <-> Codec.forward (1.5, eval)          QuarkAudio-HCodec/HCodec-1.5/vq/codec_adaptive.py:100-148
    forward20         <-> Codec.forward (2.0)                QuarkAudio-HCodec/HCodec-2.0/vq/codec.py:54-72

The forwards compute in float32 like the reference (the oracle's LSTM is fp32 only); `pred_feat` takes a `dtype`: float64 is the
yardstick the GPU tests bound the HIP path's semantic decoder against, applied to that path's own codes.  `commit_loss` is 0 in eval
(see unified_audio_amd.Codec.forward)."""
from __future__ import annotations

from typing import Dict

import torch
import torch.nn.functional as F

from oracle import hcodec_ref as R


def _cast(sd: Dict[str, torch.Tensor], dtype) -> Dict[str, torch.Tensor]:
    return {k: v.to(dtype) if v.is_floating_point() else v for k, v in sd.items()}


def semantic_decoder(sd: Dict[str, torch.Tensor], z: torch.Tensor, sd_spec, dtype=torch.float32) -> torch.Tensor:
    """Decoder.forward (semantic_module.py:294-299): z [B, code_dim, N] -> [B, output_channels, N * prod(strides)]."""
    p = "semantic_decoder"
    w = lambda k: sd[f"{p}.{k}"].to(dtype)  # noqa: E731
    x = F.conv1d(z.to(dtype), w("conv1.conv.weight"), padding=1)
    for i, s in enumerate(sd_spec.strides):
        bp = f"conv_blocks.{i}"
        if s == 1:
            x = F.conv1d(x, w(f"{bp}.conv.conv.weight"), w(f"{bp}.conv.conv.bias"), padding=1)
        else:  # ConvTranspose1d(k = 2 s, padding (s + 1) // 2, output_padding s % 2), semantic_module.py:86-104
            x = F.conv_transpose1d(x, w(f"{bp}.conv.deconv.weight"), w(f"{bp}.conv.deconv.bias"), stride=s, padding=(s + 1) // 2,
                                   output_padding=s % 2)
        for u in range(2):  # ResidualUnit: x + conv2(ELU(conv1(ELU(x))))
            y = F.conv1d(F.elu(x), w(f"{bp}.res_units.{u}.conv1.conv.weight"), padding=1)
            x = x + F.conv1d(F.elu(y), w(f"{bp}.res_units.{u}.conv2.weight"))
    return F.conv1d(x, w("conv2.conv.weight"), padding=1)


def semantic_embedding(sd, semantic_codes: torch.Tensor, num_quantizers: int) -> torch.Tensor:
    """Sum of the semantic code vectors, [B, nq, N] int64 -> [B, code_dim, N] (get_output_from_indices)."""
    return R.rvq_lookup(semantic_codes.transpose(1, 2), R.rvq_codebooks(sd, "semantic_quantizer", num_quantizers)).transpose(1, 2)


def pred_feat(sd, semantic_codes, num_quantizers: int, sd_spec, dtype=torch.float32, codebook_size: int = 0) -> torch.Tensor:
    """semantic_decoder(sum of the semantic code vectors).  codebook_size > 0: H-Codec 1.5 length-injected codes [B, nq, G], de-aggregated
    back to the N25 frames first (codec_adaptive.py:134-139)."""
    if codebook_size:
        from oracle import hcodec15_ref as R15

        plain, tl = R15.extract_lengths(semantic_codes, codebook_size)
        semantic_codes = R15.deaggregate_indices(plain, tl.clamp_min(0))
    sd = _cast({k: v for k, v in sd.items() if k.startswith(("semantic_decoder.", "semantic_quantizer."))}, dtype)
    return semantic_decoder(sd, semantic_embedding(sd, semantic_codes, num_quantizers), sd_spec, dtype)


def forward10(sd, wav, feat, spec, sd_spec):
    """(recon [B, T], pred_feat, commit_loss, (acoustic_codes, semantic_codes))."""
    ac, sc = R.encode(sd, wav.unsqueeze(1) if wav.dim() == 2 else wav, feat, spec)
    recon = R.decode(sd, ac, sc, spec)
    return recon, pred_feat(sd, sc, spec.num_quantizers, sd_spec), torch.zeros(()), (ac, sc)


def forward20(sd, wav, feat, spec, sd_spec):
    from oracle import hcodec20_ref as R20

    ac, sc = R20.encode(sd, wav, feat, spec)
    recon = R20.decode(sd, ac, sc, spec)
    return recon, pred_feat(sd, sc, spec.num_quantizers, sd_spec), torch.zeros(()), (ac, sc)


def forward15(sd, wav, feat, spec, sd_spec):
    """({'recon', 'pred_feat', 'commit_loss', 'token_lengths'}, (length-injected acoustic, semantic codes [B, nq, G]))."""
    from oracle import hcodec15_ref as R15

    enc = R15.encode(sd, wav, feat, spec)
    ac, sc = enc["acoustic_codes"], enc["semantic_codes"]
    recon = R15.decode(sd, ac, sc, spec)
    tl = R15.extract_lengths(sc, spec.codebook_size)[1]
    pred = pred_feat(sd, sc, spec.num_quantizers, sd_spec, codebook_size=spec.codebook_size)
    return {"recon": recon, "pred_feat": pred, "commit_loss": torch.zeros(()), "token_lengths": tl}, (ac, sc)
