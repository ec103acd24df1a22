"""Inputs and CPU-oracle answers shared by tests/test_hcodec20_ragged_cpu.py and tests/test_hcodec20_ragged_gpu.py (DESIGN.md
section 33): the specs, the seeds, the lengths and - computed once per process, never modified - oracle/hcodec20_ref.py on every clip
ALONE at its own length.

Small spec: the `small20` dimensions of tests/test_hcodec_ragged_gpu.py (width 256, 4 heads of 64, 5 codebooks of 64, one block and one
layer per stack).  FRAMES = [35, 17, 9, 1] code frames in N = 35, longest first, so GEMM tiles straddle clips.  In STFT / decoder frames
(4 per code frame): 140 cross the 128-query attention tile; 68 cross a 64-row boundary and leave a 4-key tail in the third 32-key tile;
36 leave a 4-key tail in the second; one code frame is 4 frames under the k9 / stride-4 output convolution.

Full width: SPEC_20 with two ConvNeXt blocks per stack (tests/test_hcodec_gpu.py::test_hcodec20_full_width_parity), FRAMES = [8, 3, 1]."""
from __future__ import annotations

import dataclasses
import functools

import torch

from oracle import hcodec20_ref as R20
from oracle import synth

HOP = 3840    # samples per code frame: hop 960 * frame_stride 4
FPC = 4       # STFT / decoder / SSL frames per code frame
JUNK = 10 ** 9  # behind a clip's end the code tensors may hold anything
FRAMES = [35, 17, 9, 1]
N = 35
SMALL = R20.HCodec20Spec(enc_dim=256, enc_inter=512, enc_convnext_layers=1, enc_transformer_layers=1, dimension=128, sem_in=64, sem_ch=128,
                         codebook_size=64, num_quantizers=5, dec_dim=256, dec_inter=512, dec_convnext_layers=1, dec_transformer_layers=1)
WIDE = dataclasses.replace(R20.SPEC_20, enc_convnext_layers=2, dec_convnext_layers=2)
WIDE_FRAMES = [8, 3, 1]
WIDE_N = 8


def product_spec(o, causal=False):
    import unified_audio_amd as qa

    return qa.HCodecSpec(version=20, enc_dim=o.enc_dim, enc_inter=o.enc_inter, enc_convnext_layers=o.enc_convnext_layers,
                         enc_layers=o.enc_transformer_layers, frame_stride=o.stride, tr_inter_cap=o.tr_inter_cap, dimension=o.dimension,
                         code_dim=o.dimension, sem_in=o.sem_in, sem_ch=o.sem_ch, sem_strides=o.sem_strides, codebook_size=o.codebook_size,
                         num_quantizers=o.num_quantizers, dec_dim=o.dec_dim, dec_inter=o.dec_inter, dec_heads=o.dec_dim // 64,
                         dec_layers=o.dec_transformer_layers, convnext_layers=o.dec_convnext_layers, n_fft=o.n_fft, hop=o.hop,
                         gn_groups=o.gn_groups, causal=causal)


def _alone(sd, ospec, wav, feat, frames):
    out = []
    with torch.no_grad():
        for b, f in enumerate(frames):
            taps = {}
            ac, sc = R20.encode(sd, wav[b:b + 1, :HOP * f], feat[b:b + 1, :, :FPC * f], ospec, taps)
            out.append(dict(ac=ac, sc=sc, emb=taps["enc.emb"], sem=taps["enc.sem"], wav=R20.decode(sd, ac, sc, ospec)))
    return out


@functools.lru_cache(maxsize=None)
def small_case():
    """The issue's set-up: weights of seed 5, wav of seed 7, features of seed 9, and the oracle on every clip alone."""
    sd = synth.hcodec20_state_dict(5, SMALL)
    wav, feat = synth.synth_wav_fullband(7, 4, HOP * N), synth.synth_feat(9, 4, FPC * N, 64)
    return dict(spec=SMALL, sd=sd, wav=wav, feat=feat, alone=_alone(sd, SMALL, wav, feat, FRAMES))


@functools.lru_cache(maxsize=None)
def wide_case():
    sd = synth.hcodec20_state_dict(61, WIDE)
    wav, feat = synth.synth_wav_fullband(62, 3, HOP * WIDE_N), synth.synth_feat(63, 3, FPC * WIDE_N, WIDE.sem_in)
    return dict(spec=WIDE, sd=sd, wav=wav, feat=feat, alone=_alone(sd, WIDE, wav, feat, WIDE_FRAMES))
