"""Inputs and CPU-oracle answers shared by tests/test_bicodec_ragged_cpu.py and tests/test_bicodec_ragged_gpu.py:
the specs, the seeds, the lengths, and - computed once per process, never modified - the fp64 oracle on every clip ALONE.

Detokenize and the semantic encoder: the small specs of tests/test_bicodec_tokenize_gpu.py (rates (4, 5, 2), kernels (8, 11, 4)) and the
odd geometry of tests/test_bicodec_gpu.py (rates (3, 2), kernels (7, 4): asymmetric phase pads); token / frame lengths (37, 20, 7, 1) in
T = 37 - a clip that fills the call, one that ends inside a row tile, one exactly a k7 wide, one shorter than every half-kernel and
every dilated pad.

The tokenizer: the small LayerNorm / stable-LN (XLSR-style) spec of tests/test_ssl_ragged_gpu.py with what BiCodecTokenizer requires of
its front-end - hidden states 11 / 14 / 16 (so 16 layers), no padding, no compression.  Sample lengths (320 * 36 + 57, 320 * 20,
320 * 7 + 123, 400): by the extractor's floor rule (one frame per 320 samples once 400 are there) these are 35 / 19 / 7 / 1 frames, not
the 36 / 20 / 7 / 1 the round numbers suggest.  REF_LEN = 4800: the 400-sample clip tiles 12 times, the 2363-sample clip 2.03 times,
the two long clips are truncated."""
from __future__ import annotations

import dataclasses
import functools

import torch
import torch.nn.functional as F

from oracle import bicodec_ref as BR
from oracle import gen_golden_bicodec as G
from oracle import ssl_ref as SR
from tests import bicodec_tokenize_ref as T
from unified_audio_amd import synth

STAGE_TOL = 5e-5   # tests/test_bicodec_gpu.py, tests/test_bicodec_tokenize_gpu.py
FLIP_CAP = 0.002   # tests/util.audit_codes' cap as those files assert it
TOKEN_LENGTHS = (37, 20, 7, 1)
SAMPLE_LENGTHS = (320 * 36 + 57, 320 * 20, 320 * 7 + 123, 400)
FRAMES = (35, 19, 7, 1)
REF_LEN = 4800
ENC_SMALL = dict(input_channels=64, vocos_dim=32, vocos_inter=64, vocos_layers=2, latent_dim=64, codebook_size=128, codebook_dim=8)
DSPECS = {
    "small": BR.BiCodecSpec(**G.SMALL),
    "odd": BR.BiCodecSpec(**dict(G.SMALL, rates=(3, 2), kernel_sizes=(7, 4), gen_channels=128)),
}
# seeds for which the oracle in fp32 already agrees with the oracle in fp64 on every token (tests/test_bicodec_ragged_cpu.py asserts it)
SEED_DETOK = {"small": 211, "odd": 212}
SEED_SEM = 221
SEED_TOK = 231
SEED_PUBLISHED = 241
PUBLISHED_LENGTHS = (50, 23)
XLSR_SMALL = SR.SSLSpec(conv_dim=(64,) * 7, num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=2, hidden_size=128,
                        num_hidden_layers=16, num_attention_heads=2, intermediate_size=256, conv_bias=True, feat_extract_norm="layer",
                        do_stable_layer_norm=True, select=(11, 14, 16), pad=0, compress_exponent=0.0)


def detokenize64(sd64, sem, glob, spec, taps=None):
    """oracle.bicodec_ref.detokenize in float64.  The oracle's own entry point is float32 in one place (fsq_codes ends in .float());
    its stages are dtype-agnostic, so this composes them as detokenize does, with global_detokenize's three lines restated around a
    cast of the FSQ codes - (digit - L // 2) / (L // 2), exact in either format."""
    z_q = BR.semantic_detokenize(sd64, sem)
    codes = BR.fsq_codes(glob.transpose(1, 2)[..., 0], spec.fsq_levels).double()
    zq = F.linear(codes, sd64["speaker_encoder.quantizer.project_out.weight"], sd64["speaker_encoder.quantizer.project_out.bias"])
    d = F.linear(zq.transpose(1, 2).reshape(zq.shape[0], -1), sd64["speaker_encoder.project.weight"], sd64["speaker_encoder.project.bias"])
    x = BR.prenet(sd64, z_q, d, spec, taps) + d.unsqueeze(-1)
    if taps is not None:
        taps["z_q"], taps["d_vector"], taps["prenet.out"] = z_q, d, x
    return BR.wave_generator(sd64, x, spec, taps)


def fields(spec):
    return {f: getattr(spec, f) for f in spec.__dataclass_fields__}


def cl(t):  # oracle [B, C, T] -> library [B, T, C]
    return t.transpose(1, 2).contiguous()


@torch.no_grad()
@functools.lru_cache(maxsize=None)
def detok_case(name):
    """weights, tokens [4, 37] (every entry a valid token: a rectangular call can run them too) and the oracle on each clip alone."""
    spec = DSPECS[name]
    seed = SEED_DETOK[name]
    sd = synth.bicodec_state_dict(seed, spec)
    sem, glob = synth.bicodec_tokens(seed + 100, len(TOKEN_LENGTHS), max(TOKEN_LENGTHS), spec)
    sd64 = T.cast(sd)
    alone = []
    for b, n in enumerate(TOKEN_LENGTHS):
        taps = {}
        wav = detokenize64(sd64, sem[b:b + 1, :n], glob[b:b + 1], spec, taps)
        alone.append(dict(wav=wav[0, 0], taps=oracle_detok_taps(sd64, spec, taps)))
    return dict(spec=spec, sd=sd, sem=sem, glob=glob, alone=alone)


def oracle_detok_taps(sd, spec, taps):
    """the oracle's intermediates in the library's layout ([T, C] per clip) and activation state (a block's output is stored already
    activated by its consumer's Snake, tests/test_bicodec_gpu.py)"""
    out = {"z_q": cl(taps["z_q"])[0], "prenet.down": taps["prenet.down"][0], "prenet.backbone": taps["prenet.backbone"][0],
           "prenet.out": cl(taps["prenet.out"])[0]}
    n = len(spec.rates)
    for i in range(n):
        alpha = sd[f"decoder.model.{i + 2}.block.0.alpha"] if i + 1 < n else sd[f"decoder.model.{n + 1}.alpha"]
        out[f"gen.block{i}"] = cl(BR.snake(taps[f"gen.block{i}"], alpha))[0]
    return out


def encoder_sd(espec_kw, seed):
    """tokenizer + detokenizer weights of a small model (tests/test_bicodec_tokenize_gpu._full_sd, without its import of the library)"""
    import unified_audio_amd as qa

    espec = qa.BiCodecEncoderSpec(**espec_kw)
    dspec = qa.BiCodecSpec(**G.SMALL)
    sd = synth.bicodec_state_dict(seed, dspec)
    sd.update(synth.bicodec_encoder_state_dict(seed + 1, espec))
    sd.update(synth.bicodec_speaker_state_dict(seed + 2, espec))
    return espec, dspec, sd


@functools.lru_cache(maxsize=None)
def semantic_case():
    """feat [4, 37, 64] and, per clip alone, the oracle's tokens and its normalised latents (the audit's context)"""
    espec, dspec, sd = encoder_sd(ENC_SMALL, SEED_SEM)
    feat = synth.synth_feat(SEED_SEM + 5, len(TOKEN_LENGTHS), max(TOKEN_LENGTHS), espec.input_channels).transpose(1, 2).contiguous()
    sd64 = T.cast(sd)
    alone = []
    for b, n in enumerate(TOKEN_LENGTHS):
        taps = {}
        tok = T.get_semantic_tokens(sd64, feat[b:b + 1, :n].double(), espec.vocos_layers, taps)
        alone.append(dict(tokens=tok[0], latent=taps["vq.latent"]))
    return dict(espec=espec, dspec=dspec, sd=sd, feat=feat, alone=alone)


@functools.lru_cache(maxsize=None)
def tokenizer_case():
    """wav [4, 11577] with other (finite) samples behind every clip's end; per clip alone the oracle's global tokens (and their bounded
    FSQ values, the audit's context) of get_ref_clip(clip)"""
    # the speaker encoder's widths are the detokenizer's (token_num 4 of 32-wide latents), so that the round trip runs
    espec, dspec, sd = encoder_sd(dict(ENC_SMALL, input_channels=XLSR_SMALL.hidden_size, spk_latent_dim=G.SMALL["spk_latent_dim"],
                                       token_num=G.SMALL["token_num"]), SEED_TOK)
    ssl_sd = SR.synth_state_dict(SEED_TOK + 5, XLSR_SMALL, "wav2vec2")
    wav = synth.synth_wav(SEED_TOK + 6, len(SAMPLE_LENGTHS), max(SAMPLE_LENGTHS)) * torch.tensor([[1.0], [0.3], [2.0], [0.7]]) + 0.05
    sd64 = T.cast(sd)
    alone = []
    for b, n in enumerate(SAMPLE_LENGTHS):
        taps = {}
        clip = T.ref_clip(wav[b:b + 1, :n], REF_LEN)
        glob = T.get_global_tokens(sd64, clip.double(), espec.mel_params, espec.fsq_levels, taps=taps)
        alone.append(dict(glob=glob[0], bounded=taps["fsq.bounded"]))
    return dict(espec=espec, dspec=dspec, sd=sd, ssl_sd=ssl_sd, wav=wav, alone=alone)


@functools.lru_cache(maxsize=None)
def published_case():
    """the published widths with 2-layer backbones (tests/test_bicodec_gpu.py::test_published_widths_short_backbone), B = 2: weights,
    tokens and features; per clip alone the oracle's semantic tokens and latents (the detokenize oracle at these widths is run by the
    GPU test itself)"""
    import unified_audio_amd as qa

    spec = BR.BiCodecSpec(vocos_layers=2)
    espec = dataclasses.replace(qa.SPEC_BICODEC_ENCODER, vocos_layers=2)
    sd = synth.bicodec_state_dict(SEED_PUBLISHED, spec)
    sd.update(synth.bicodec_encoder_state_dict(SEED_PUBLISHED + 1, espec))
    sd.update(synth.bicodec_speaker_state_dict(SEED_PUBLISHED + 2, espec))
    B, Tm = len(PUBLISHED_LENGTHS), max(PUBLISHED_LENGTHS)
    sem, glob = synth.bicodec_tokens(SEED_PUBLISHED + 3, B, Tm, spec)
    feat = synth.synth_feat(SEED_PUBLISHED + 4, B, Tm, espec.input_channels).transpose(1, 2).contiguous()
    sd64 = cast_used(sd, ("encoder.", "quantizer."))
    alone = []
    for b, n in enumerate(PUBLISHED_LENGTHS):
        taps = {}
        tok = T.get_semantic_tokens(sd64, feat[b:b + 1, :n].double(), espec.vocos_layers, taps)
        alone.append(dict(tokens=tok[0], latent=taps["vq.latent"]))
    return dict(spec=spec, espec=espec, sd=sd, sem=sem, glob=glob, feat=feat, alone=alone)


def cast_used(sd, prefixes, dtype=torch.float64):
    return {k: v.to(dtype) for k, v in sd.items() if k.startswith(prefixes)}


def frames_rule(n):
    """XLSR-53's frame count for n samples without padding: kernels 10, 3, 3, 3, 3, 2, 2 at strides 5, 2, 2, 2, 2, 2, 2 (floor)"""
    for k, s in zip((10, 3, 3, 3, 3, 2, 2), (5, 2, 2, 2, 2, 2, 2)):
        n = (n - k) // s + 1
    return n


def xlsr_qa_spec():
    import unified_audio_amd as qa

    return qa.SSLSpec(**{f.name: getattr(XLSR_SMALL, f.name) for f in dataclasses.fields(XLSR_SMALL)})
