"""Per-clip lengths for H-Codec 2.0, the parts that need no GPU: qa_resample_ragged is declared, exported and
bound; the frame arithmetic of the 2.0 tokenizer; and, on the CPU oracle, why zero padding is not the per-clip answer."""
import ctypes as C
import math
import os
import re

import pytest
import torch

from oracle import hcodec20_ref as R20
from oracle import resample_ref as RR
from tests import hcodec20_ragged_cases as K
from tests.util import rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CTYPE = {"const float*": C.c_void_p, "float*": C.c_void_p, "void*": C.c_void_p, "int64_t": C.c_int64, "int32_t": C.c_int32}


def test_resample_ragged_is_declared_exported_and_bound(qa_lib):
    from unified_audio_amd import _lib

    header = open(os.path.join(ROOT, "include", "quarkaudio.h")).read()
    m = re.search(r"\bint\s+qa_resample_ragged\s*\(([^;]*?)\)\s*;", header, re.S)
    assert m, "qa_resample_ragged is not declared in quarkaudio.h"
    args = [(" ".join(a.split()[:-1]), a.split()[-1]) for a in m.group(1).split(",")]
    assert hasattr(qa_lib, "qa_resample_ragged")
    res, bound = _lib.SYMBOLS["qa_resample_ragged"]
    assert res is C.c_int and len(bound) == len(args) == 8, (bound, args)
    for (ctype, arg), got in zip(args, bound):
        if arg == "lengths":  # host memory: a typed pointer, so that ctypes refuses a tensor's data_ptr() there
            assert ctype == "const int64_t*" and got is C.POINTER(C.c_int64)
        else:
            assert got is _CTYPE[ctype], (arg, ctype, got)
    assert [a for _, a in args] == ["wav", "B", "T", "lengths", "orig_freq", "new_freq", "out", "stream"]
    assert qa_lib.qa_version() == 103


def test_null_arguments_are_refused_without_a_device(qa_lib):
    ln = (C.c_int64 * 1)(1)
    assert qa_lib.qa_resample_ragged(None, 1, 4, ln, 48000, 16000, None, None) == -1
    assert b"qa_resample_ragged" in qa_lib.qa_last_error()
    assert qa_lib.qa_resample_ragged(C.c_void_p(64), 1, 4, None, 48000, 16000, C.c_void_p(64), None) == -1
    assert b"qa_resample_ragged" in qa_lib.qa_last_error()


def test_frame_arithmetic_of_the_2_0_tokenizer():
    """f code frames -> 3840 f samples at 48 kHz -> 1280 f samples at 16 kHz -> 4 f SSL frames (HuBERT's rule behind the (160, 160)
    padding of the tokenizers: (n + 320 - 400) // 320 + 1)."""
    from unified_audio_amd.hcodec import SPEC_20, HCodecTokenizer, code_frames

    class Tok:
        sampling_rate = 48000
        resampled_lengths = HCodecTokenizer.resampled_lengths

    assert SPEC_20.enc_hop == K.HOP == 3840 and SPEC_20.dec_upsample == K.FPC == int(math.prod(SPEC_20.sem_strides))
    assert code_frames([3840 * 5 + 7, 3840 + 1, 3840, 1], 3840) == [6, 2, 1, 1]
    for f in (1, 2, 9, 17, 35, 375):
        (n16,) = Tok().resampled_lengths([3840 * f])
        assert n16 == 1280 * f == RR.resample(torch.zeros(1, 3840 * f), 48000, 16000).shape[-1]
        assert (n16 + 320 - 400) // 320 + 1 == 4 * f
    assert Tok().resampled_lengths([3847, 41, 1]) == [1283, 14, 1]
    t = Tok()
    t.sampling_rate = 44100
    assert t.resampled_lengths([4410, 3847, 1]) == [math.ceil(16000 * n / 44100) for n in (4410, 3847, 1)]


def _resample_by_window(wav, orig_freq, new_freq):
    """oracle.resample_ref.resample with its convolution evaluated window by window: the same kernel, padding and cut, and every output
    one fixed-order sum over its own window, so that an output does not depend on how many windows the call holds.  (F.conv1d picks its
    blocking by the signal's length; on the host measured here that moved the prefix below by one unit in the last place, 6e-8.)"""
    kernel, width, orig, new = RR.sinc_resample_kernel(orig_freq, new_freq)
    x = torch.nn.functional.pad(wav, (width, width + orig)).unfold(-1, kernel.shape[-1], orig)  # [n, windows, taps]
    y = torch.stack([(x * kernel[i, 0]).sum(-1) for i in range(new)], dim=-1).reshape(wav.shape[0], -1)
    return y[:, :math.ceil(new * wav.shape[-1] / orig)]


def test_a_zero_filled_row_rings_behind_the_clip():
    """The oracle's resampler: a 3847-sample clip alone gives 1283 outputs; the same clip zero-filled to 11 520 samples gives the same
    1283 bit for bit, and filter ringing behind them - so a per-clip resample has to WRITE its zeros."""
    g = torch.Generator().manual_seed(3847)
    clip = torch.randn(1, 3847, generator=g)
    zero_filled = torch.nn.functional.pad(clip, (0, 11520 - 3847))
    alone, filled = _resample_by_window(clip, 48000, 16000), _resample_by_window(zero_filled, 48000, 16000)
    assert alone.shape[-1] == 1283 and filled.shape[-1] == 3840
    assert torch.equal(filled[:, :1283], alone)
    ring = float(filled[:, 1283:1293].abs().max())
    print(f"ringing in the ten outputs behind the clip: {ring:.3e}")
    assert ring > 1e-3
    # the helper is the oracle: the bound of tests/test_boundary_gpu.py::test_resample_matches_the_torchaudio_restatement
    for got, x in ((alone, clip), (filled, zero_filled)):
        want = RR.resample(x, 48000, 16000)
        assert got.shape == want.shape and float((got - want).abs().max()) < 2e-6 * float(want.abs().max()) + 1e-6


def test_zero_padding_is_not_the_clip_alone():
    """The shorter clips of the issue's batch, zero-padded to N = 35 code frames through the oracle, against the same clip alone: at
    least one acoustic code changes, the decode of the clip's own codes (dropped codes behind them) differs by more than 0.1 relative
    RMS where the project's bound is 1e-4, and the semantic codes do not move."""
    c = K.small_case()
    sd, o = c["sd"], c["spec"]
    with torch.no_grad():
        for b, f in list(enumerate(K.FRAMES))[1:]:
            alone = c["alone"][b]
            wav = torch.zeros(1, K.HOP * K.N)
            feat = torch.zeros(1, 64, K.FPC * K.N)
            wav[:, :K.HOP * f], feat[:, :, :K.FPC * f] = c["wav"][b, :K.HOP * f], c["feat"][b, :, :K.FPC * f]
            taps = {}
            ac, sc = R20.encode(sd, wav, feat, o, taps)
            changed = float((ac[:, :, :f] != alone["ac"]).float().mean())
            emb = rel_err(taps["enc.emb"][:, :, :f], alone["emb"])
            pad = torch.full((1, o.num_quantizers, K.N), -1, dtype=torch.int64)
            ac_p, sc_p = pad.clone(), pad.clone()
            ac_p[:, :, :f], sc_p[:, :, :f] = alone["ac"], alone["sc"]
            err = rel_err(R20.decode(sd, ac_p, sc_p, o)[:, :K.HOP * f], alone["wav"])
            print(f"clip of {f} code frames zero-padded to {K.N}: acoustic codes changed {changed:.2f}, enc.emb rel. {emb:.2f}, "
                  f"decode rel. RMS {err:.2f}")
            assert changed > 0 and emb > 1e-4
            assert err > 0.1
            assert torch.equal(sc[:, :, :f], alone["sc"])
