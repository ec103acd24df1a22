"""CPU side of the condition path with per-row lengths.

  1  the per-row oracle (tests/lm_cond_ragged_ref.py) at full lengths IS the batched restatement
  2  lengths are not the mask: the reference's ConformerEncoder.forward(x, mask) hides padded keys but its convolution module never sees
     the mask, so a masked batch differs from each clip alone on every short row - by far more than any arithmetic error - whether or not
     the padded input frames are zeroed first; and a log-mel row cut out of a batch differs from the log-mel of the short clip alone
  3  the host plan of the condition form (csrc/lm_score_rows.h, ScoreRowsShape::cond_form) as a stand-alone program under the host
     sanitizers (tools/lm_cond_rows_selftest.cpp)"""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import conformer_ref as R
from tests import lm_cond_ragged_ref as RR
from unified_audio_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL_CF = dict(num_layers=2, dim=64, heads=2, dim_head=32, depthwise_conv_kernel_size=31, ff_mult=2, dropout=0.1, qk_norm=None,
                pe_attn_head=1)
LENGTHS = [130, 1, 15, 16, 64, 65]


def _err(y, y64):
    y64 = y64.double()
    return float((y.double() - y64).abs().max() / y64.pow(2).mean().sqrt())


def _setup():
    sd = synth.conformer_state_dict(33, SMALL_CF)
    x = torch.from_numpy(np.random.default_rng(8).standard_normal((6, 130, 64)).astype("float32"))
    return sd, x


def test_oracle_at_full_lengths_is_the_batched_restatement():
    sd, x = _setup()
    x = x[:3, :40]
    t_rows, t_batch = {}, {}
    rows = RR.conformer_encoder(sd, SMALL_CF, x, [40] * 3, dtype=torch.float64, taps=t_rows)
    batch = R.conformer_encoder(sd, SMALL_CF, x, dtype=torch.float64, taps=t_batch)
    assert _err(rows, batch) <= 1e-12
    for name in t_batch:
        assert _err(t_rows[name], t_batch[name]) <= 1e-12, name
    wav = synth.synth_wav(5, 3, 1083)
    assert torch.equal(RR.stft_logmel(wav, [1083] * 3, dtype=torch.float64), R.stft_logmel(wav, dtype=torch.float64))
    csd = synth.cond_encoder_state_dict(52, 80, 128, SMALL_CF)
    mel = synth.synth_logmel(9, 2, 30)
    assert _err(RR.condition(csd, SMALL_CF, mel, [30, 30], dtype=torch.float64), R.condition(csd, SMALL_CF, mel, dtype=torch.float64)) <= 1e-12


@pytest.mark.parametrize("zero_padding", [False, True])
def test_the_mask_is_not_lengths(zero_padding):
    """Every short row of the masked batch is at least 1e-2 (max |d| / rms) away from the clip alone; float32 arithmetic is 1e-6."""
    sd, x = _setup()
    mask = torch.arange(130)[None, :] < torch.tensor(LENGTHS)[:, None]
    xin = x.clone()
    if zero_padding:
        xin[~mask] = 0.0
    masked = R.conformer_encoder(sd, SMALL_CF, xin, mask, dtype=torch.float64)
    alone = RR.conformer_encoder(sd, SMALL_CF, x, LENGTHS, dtype=torch.float64)
    alone32 = RR.conformer_encoder(sd, SMALL_CF, x, LENGTHS)
    for b, n in enumerate(LENGTHS):
        e, e32 = _err(masked[b, :n], alone[b, :n]), _err(alone32[b, :n], alone[b, :n])
        print(f"row {b} length {n}: masked batch vs clip alone {e:.3e}; float32 restatement {e32:.3e}")
        assert e32 <= 1e-5
        if n < 130:
            assert e >= 1e-2, f"row {b}: the mask reproduced the clip alone ({e:.3e})"
        else:
            assert e <= 1e-12


@pytest.mark.parametrize("n", [1, 320, 321, 480])
def test_a_logmel_row_of_a_batch_is_not_the_short_clip(n):
    """R.stft_logmel of the [1, 1083] clip, cut to the frames the n-sample clip owns, against that clip alone: above 0.1 in log-mel."""
    wav = synth.synth_wav(5, 1, 1083)
    full = R.stft_logmel(wav, dtype=torch.float64)[0]
    alone = R.stft_logmel(wav[:, :n], dtype=torch.float64)[0]
    F = RR.frames(n)
    assert alone.shape[0] == F
    d = float((full[:F] - alone).abs().max())
    print(f"n = {n}: {F} frames, max |batch row - clip alone| = {d:.3f}")
    assert d > 0.1


def test_cond_rows_selftest_is_clean_under_the_host_sanitizers(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler: tools/lm_cond_rows_selftest.cpp cannot be built")
    exe = str(tmp_path / "lm_cond_rows_selftest")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-I",
           os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "unified_audio_amd", "csrc"),
           os.path.join(ROOT, "tools", "lm_cond_rows_selftest.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "lm_cond_rows_selftest: ok" in r.stdout
