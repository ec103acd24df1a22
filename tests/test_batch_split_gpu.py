"""QA_BATCH_SPLIT: a one-stream phase of an H-Codec call as two half-batch lanes on two streams (csrc/hcodec.cpp)
against the one-lane call (knob 0).  Every op of a split region is per clip - conv_gemm's bits do not depend on M or the tile, attention
is per (clip, head) - and a lane is a row range of the same buffers, so both code tensors and the waveform must agree BIT FOR BIT.

Every case sets every bit of the knob (bits a build does not define select nothing, so the cases stand for regions added later) and
QA_BATCH_SPLIT_MIN_ROWS = 0, and calls three times - split, one lane, split - so that what an earlier call left in the workspace cannot
hide a lane reading memory the other lane still writes.  The library checks that the lanes' workspace ranges are disjoint in every one
of these calls.  Around each case the LSTM diagnostics must show no diverted launch and no degraded device, and nothing on stderr may
report the per-step re-run: the recurrences run behind the join and have the device to themselves.

Models: tests/util.MINI (width 128, 2 heads, 1 - 2 layers; the smallest the library builds), n25 of 12 - 20 code frames; taps off."""
import ctypes as C
import dataclasses

import pytest
import torch

from oracle import synth
from tests.util import MINI

pytestmark = pytest.mark.gpu

ALL = 7  # bit 1 bottleneck, bit 2 decode_tail, bit 4 encode_front


def _lstm_stats(qa_lib):
    from unified_audio_amd import _lib

    out = (C.c_int64 * 4)()
    _lib.check(qa_lib.qa_debug_lstm_stats(0, out))
    return {"launches": out[0], "in_flight": out[1], "diverted": out[2], "degraded": out[3]}


def _split_regions(qa_lib):
    fn = qa_lib.qa_debug_batch_split_regions
    fn.restype, fn.argtypes = C.c_longlong, []
    return int(fn())


def _mini15(device, **kw):
    import unified_audio_amd as qa

    spec = dataclasses.replace(qa.HCodecSpec(**MINI), adaptive=True, agg_layers=2, bt_layers=2, agg_heads=2, bt_heads=2, agg_ff=128, bt_ff=128,
                               max_tokens_per_group=8, **kw)
    return qa.Codec(None, None, None, spec=spec, device=device).load_state_dict(synth.hcodec10_state_dict(7, spec)), spec


def _inputs15(spec, B, n25, device):
    return (synth.synth_wav(8, B, n25 * spec.enc_hop).to(device).unsqueeze(1), synth.synth_feat(10, B, 2 * n25, spec.sem_in).to(device))


def _abab(qa_lib, knob, capfd, call, names, want_split):
    """call() with the knob at ALL, 0, ALL: the outputs of the first run, after asserting that the three agree bit for bit, that the split
    runs took two lanes exactly when want_split, and that no recurrence was diverted, degraded or re-run"""
    knob("QA_BATCH_SPLIT_MIN_ROWS", 0)
    before = _lstm_stats(qa_lib)
    runs, lanes = [], []
    for v in (ALL, 0, ALL):
        knob("QA_BATCH_SPLIT", v)
        r0 = _split_regions(qa_lib)
        out = call()
        torch.cuda.synchronize()
        runs.append([t.clone() for t in out])
        lanes.append(_split_regions(qa_lib) - r0)
    for other, word in ((runs[1], "one lane"), (runs[2], "the second split call")):
        for name, u, v in zip(names, runs[0], other):
            assert u.shape == v.shape and torch.equal(u, v), f"{name}: the split call differs from {word} in {int((u != v).sum())} of {u.numel()} values"
    print("regions that ran as two lanes (split, one lane, split):", lanes)
    assert lanes[1] == 0 and lanes[0] == lanes[2] and (lanes[0] > 0) == want_split, lanes
    after = _lstm_stats(qa_lib)
    assert after["diverted"] == before["diverted"] and after["degraded"] == 0, (before, after)
    assert "re-running" not in capfd.readouterr().err
    return runs[0]


def _codec15_roundtrip(codec, wav, feat):
    codes = codec.encode(wav, feat, threshold=0.9)
    ac, sc = codes["acoustic_codes"], codes["semantic_codes"]
    return ac, sc, codec.decode(ac, sc)


@pytest.mark.parametrize("B, n25", [(3, 13), (2, 16), (1, 20)], ids=["B3-odd-split", "B2", "B1-no-split"])
def test_hcodec15_encode_decode(qa_lib, gpu_device, knob, capfd, B, n25):
    """B = 3: lanes of 2 and 1 clips, 26 and 13 rows - no multiple of any tile; B = 1: one lane, and the call still succeeds."""
    codec, spec = _mini15(gpu_device)
    wav, feat = _inputs15(spec, B, n25, gpu_device)
    ac, sc, w = _abab(qa_lib, knob, capfd, lambda: _codec15_roundtrip(codec, wav, feat), ("acoustic_codes", "semantic_codes", "wav"), B >= 2)
    assert ac.shape[:2] == (B, spec.num_quantizers) and w.shape == (B, n25 * spec.enc_hop) and bool(torch.isfinite(w).all())


@pytest.mark.parametrize("frames", [[16, 11, 3], [5, 9, 16]], ids=["shortest-alone-in-lane-1", "longest-alone-in-lane-1"])
def test_hcodec15_ragged(qa_lib, gpu_device, knob, capfd, frames):
    """encode_ragged / decode_ragged, B = 3: lane 1 holds clip 2 alone with its own slice of the lengths and of the key mask."""
    codec, spec = _mini15(gpu_device)
    n25 = max(frames)
    wav, feat = _inputs15(spec, 3, n25, gpu_device)

    def call():
        codes = codec.encode_ragged(wav, feat, frames, threshold=0.9)
        ac, sc = codes["acoustic_codes"], codes["semantic_codes"]
        return ac, sc, codec.decode_ragged(ac, sc)

    ac, sc, w = _abab(qa_lib, knob, capfd, call, ("acoustic_codes", "semantic_codes", "wav"), True)
    assert codec.adaptive_frames(sc) == frames
    length = torch.div(sc[:, 0], spec.codebook_size, rounding_mode="floor") + 1  # 0: an entry behind the clip's groups
    behind = (length == 0)[:, None, :].expand_as(sc)
    assert bool(behind.any()) and bool((sc[behind] == -1).all()) and bool((ac[behind] == -1).all())
    spf = spec.enc_hop
    for b, f in enumerate(frames):
        assert bool((w[b, spf * f:] == 0).all()) and bool(torch.isfinite(w[b]).all())


def test_hcodec15_causal(qa_lib, gpu_device, knob, capfd):
    """the causal variant of the 1.5 spec: causal convolutions, causal aggregators and a causal bottleneck with a short context"""
    codec, spec = _mini15(gpu_device, causal=True, agg_causal=True, agg_context=5, bt_causal=True, bt_context=7)
    wav, feat = _inputs15(spec, 3, 14, gpu_device)
    _abab(qa_lib, knob, capfd, lambda: _codec15_roundtrip(codec, wav, feat), ("acoustic_codes", "semantic_codes", "wav"), True)


def _codes(seed, B, q, n, K, device):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, K, (B, q, n), generator=g).to(device), torch.randint(0, K, (B, q, n), generator=g).to(device)


@pytest.mark.parametrize("lengths", [None, [12, 7, 2]], ids=["rectangular", "ragged"])
def test_hcodec10_decode(qa_lib, gpu_device, knob, capfd, lengths):
    """decode_tail of H-Codec 1.0 (sub-pixel upsampler), B = 3.  This build splits no region of it: the case pins the one-lane path."""
    import unified_audio_amd as qa

    spec = qa.HCodecSpec(**MINI)
    codec = qa.Codec(None, None, None, spec=spec, device=gpu_device).load_state_dict(synth.hcodec10_state_dict(5, spec))
    ac, sc = _codes(3, 3, spec.num_quantizers, 12, spec.codebook_size, gpu_device)
    (w,) = _abab(qa_lib, knob, capfd, lambda: (codec.decode(ac, sc, lengths=lengths),), ("wav",), False)
    assert bool(torch.isfinite(w).all())


def test_hcodec20_decode(qa_lib, gpu_device, knob, capfd):
    """decode_tail of H-Codec 2.0, B = 3: the in_rep embed convolution, and the persistent recurrence (the d = 1536 path) forced on at the
    test width.  This build splits no region of it: the case pins the one-lane path."""
    import unified_audio_amd as qa
    from oracle import hcodec20_ref as R20

    o = R20.HCodec20Spec(enc_dim=256, enc_inter=512, enc_convnext_layers=1, enc_transformer_layers=1, dimension=128, sem_in=64, sem_ch=128,
                         codebook_size=64, num_quantizers=5, dec_dim=256, dec_inter=512, dec_convnext_layers=1, dec_transformer_layers=1)
    p = qa.HCodecSpec(version=20, enc_dim=o.enc_dim, enc_inter=o.enc_inter, enc_convnext_layers=o.enc_convnext_layers,
                      enc_layers=o.enc_transformer_layers, frame_stride=o.stride, tr_inter_cap=o.tr_inter_cap, dimension=o.dimension,
                      code_dim=o.dimension, sem_in=o.sem_in, sem_ch=o.sem_ch, sem_strides=o.sem_strides, codebook_size=o.codebook_size,
                      num_quantizers=o.num_quantizers, dec_dim=o.dec_dim, dec_inter=o.dec_inter, dec_heads=o.dec_dim // 64,
                      dec_layers=o.dec_transformer_layers, convnext_layers=o.dec_convnext_layers, n_fft=o.n_fft, hop=o.hop, gn_groups=o.gn_groups)
    codec = qa.Codec(None, None, None, spec=p, device=gpu_device).load_state_dict(synth.hcodec20_state_dict(5, o))
    knob("QA_LSTM_PERSISTENT", 1)
    ac, sc = _codes(4, 3, o.num_quantizers, 12, o.codebook_size, gpu_device)
    (w,) = _abab(qa_lib, knob, capfd, lambda: (codec.decode(ac, sc),), ("wav",), False)
    assert bool(torch.isfinite(w).all())


def test_taps_on_takes_one_lane(qa_lib, gpu_device, knob):
    """With taps on a region falls back to one lane (the golden tests keep seeing the parent's path): the same codes and waveform."""
    codec, spec = _mini15(gpu_device)
    wav, feat = _inputs15(spec, 3, 13, gpu_device)
    knob("QA_BATCH_SPLIT_MIN_ROWS", 0)
    knob("QA_BATCH_SPLIT", ALL)
    r0 = _split_regions(qa_lib)
    want = [t.clone() for t in _codec15_roundtrip(codec, wav, feat)]
    r1 = _split_regions(qa_lib)
    codec.enable_taps()
    got = [t.clone() for t in _codec15_roundtrip(codec, wav, feat)]
    torch.cuda.synchronize()
    assert r1 > r0 and _split_regions(qa_lib) == r1
    assert codec.tap("dec.bottleneck").numel() == 3 * 13 * 2 * spec.code_dim
    for name, u, v in zip(("acoustic_codes", "semantic_codes", "wav"), want, got):
        assert u.shape == v.shape and torch.equal(u, v), name
