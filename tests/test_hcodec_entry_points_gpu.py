"""The argument checks of the H-Codec entry points (csrc/hcodec.cpp: qa_hcodec_encode / _encode_ragged / _encode_adaptive / _forward /
_forward_adaptive and the decode family): a waveform that is no whole number of code frames, a handle of the other family, a feature
count that does not fit the code frames - each refused with its status before anything is written, in a message that names the entry
point the caller called and the offending values - and `lengths = [n] * B` is the call without lengths, bit for bit.

Models: tests/util.MINI (hop 16) as H-Codec 1.0, and the same at width 128 as an H-Codec 1.5 (the spec of test_agg_last_rows_gpu: the
encoder LSTM needs a multiple of 128), both with the semantic decoder attached so that forward gets as far as its own checks."""
import ctypes as C
import dataclasses

import pytest
import torch

from tests.util import MINI, with_knob
from unified_audio_amd import synth

pytestmark = pytest.mark.gpu

HOP = 16  # samples per code frame of MINI: 2 * prod(ratios); 2 feature frames per code frame
B, N = 2, 9
INVALID = -1  # QA_ERR_INVALID
SENTINEL = -(7 ** 20)  # no code


@pytest.fixture(scope="module")
def codecs(qa_lib, gpu_device):
    import unified_audio_amd as qa
    from unified_audio_amd.hcodec import SemanticDecoderSpec

    out = {}
    for name, spec in (("1.0", qa.HCodecSpec(**MINI)),
                       ("1.5", dataclasses.replace(qa.HCodecSpec(**MINI), adaptive=True, agg_layers=2, bt_layers=1, agg_heads=2, bt_heads=2,
                                                   agg_ff=128, bt_ff=128, max_tokens_per_group=32))):
        sd = synth.hcodec10_state_dict(7, spec)
        sd.update(synth.hcodec_semantic_decoder_state_dict(107, SemanticDecoderSpec.from_codec_spec(spec)))
        out[name] = qa.Codec(None, None, None, spec=spec, device=gpu_device).load_state_dict(sd)
        assert out[name].has_semantic_decoder
    return out


def _inputs(device, samples, seed=11):
    wav = synth.synth_wav(seed, B, samples).to(device).unsqueeze(1)
    feat = synth.synth_feat(seed + 1, B, 2 * N, MINI["sem_in"]).to(device)
    return wav, feat


class _Raw:
    """One codec's entry points through ctypes, on contiguous device tensors; every call returns (status, qa_last_error())."""

    def __init__(self, codec, wav, feat):
        from unified_audio_amd.hcodec import _stream_ptr

        self.lib, self.h, self.dev, self.stream = codec._lib, codec._handle, codec.device, _stream_ptr(codec.device)
        self.wav, self.feat = wav.contiguous(), feat.contiguous()
        q = codec.spec.num_quantizers
        self.T = self.wav.shape[-1]
        self.ac = torch.full((B, q, N), SENTINEL, dtype=torch.int64, device=self.dev)
        self.sc = self.ac.clone()
        self.recon = torch.full((B, N * HOP), float("inf"), device=self.dev)
        self.pred = torch.full((B, MINI["sem_in"], 2 * N), float("inf"), device=self.dev)
        self.tl = torch.full((B, N), SENTINEL, dtype=torch.int64, device=self.dev)
        self.g = C.c_int64(SENTINEL)

    def _ret(self, st):
        return st, self.lib.qa_last_error().decode("utf-8", "replace")

    def _feat(self, n_feat=None):
        sb, sch, st = self.feat.stride()
        return self.feat.data_ptr(), sb, sch, st, self.feat.shape[2] if n_feat is None else n_feat

    def encode(self):
        return self._ret(self.lib.qa_hcodec_encode(self.h, self.wav.data_ptr(), B, self.T, *self._feat(), self.ac.data_ptr(), self.sc.data_ptr(),
                                                   self.stream))

    def encode_ragged(self, frames, n_feat=None):
        return self._ret(self.lib.qa_hcodec_encode_ragged(self.h, self.wav.data_ptr(), B, self.T, (C.c_int64 * B)(*frames), *self._feat(n_feat),
                                                          self.ac.data_ptr(), self.sc.data_ptr(), self.stream))

    def encode_adaptive(self):
        return self._ret(self.lib.qa_hcodec_encode_adaptive(self.h, self.wav.data_ptr(), B, self.T, *self._feat(), self.ac.data_ptr(),
                                                            self.sc.data_ptr(), C.byref(self.g), 0.0, self.stream))

    def decode(self):
        codes = torch.zeros_like(self.ac)
        return self._ret(self.lib.qa_hcodec_decode(self.h, codes.data_ptr(), codes.data_ptr(), B, N, self.recon.data_ptr(), self.stream))

    def decode_adaptive(self):
        codes = torch.zeros_like(self.ac)
        return self._ret(self.lib.qa_hcodec_decode_adaptive(self.h, codes.data_ptr(), codes.data_ptr(), B, N, N, self.recon.data_ptr(),
                                                            self.stream))

    def forward(self):
        return self._ret(self.lib.qa_hcodec_forward(self.h, self.wav.data_ptr(), B, self.T, *self._feat(), self.recon.data_ptr(),
                                                    self.pred.data_ptr(), self.stream))

    def forward_adaptive(self):
        return self._ret(self.lib.qa_hcodec_forward_adaptive(self.h, self.wav.data_ptr(), B, self.T, *self._feat(), self.recon.data_ptr(),
                                                             self.pred.data_ptr(), self.tl.data_ptr(), C.byref(self.g), self.stream))

    def untouched(self):
        torch.cuda.synchronize()
        return (bool((self.ac == SENTINEL).all()) and bool((self.sc == SENTINEL).all()) and bool(torch.isinf(self.recon).all())
                and bool(torch.isinf(self.pred).all()) and bool((self.tl == SENTINEL).all()) and self.g.value == SENTINEL)


def test_a_waveform_that_is_no_whole_number_of_code_frames(codecs, gpu_device):
    """1. T = 3 * hop + 1 through the Python calls: QA_ERR_INVALID, the message says `multiple of 16`.  Through ctypes the five entry
    points name themselves, and no output - codes, waveform, features, group lengths, the group count - is written."""
    import unified_audio_amd as qa

    wav, feat = _inputs(gpu_device, 3 * HOP + 1)
    c10, c15 = codecs["1.0"], codecs["1.5"]
    calls = {"1.0 encode": lambda: c10.encode(wav, feat), "1.0 encode(lengths)": lambda: c10.encode(wav, feat, lengths=[3, 2]),
             "1.0 forward": lambda: c10(wav, feat), "1.5 encode": lambda: c15.encode(wav, feat), "1.5 forward": lambda: c15(wav, feat)}
    for name, call in calls.items():
        with pytest.raises(qa.QuarkAudioError) as e:
            call()
        print(name, "->", e.value)
        assert e.value.status == INVALID and f"multiple of {HOP}" in str(e.value), (name, str(e.value))
    r10, r15 = _Raw(c10, wav, feat), _Raw(c15, wav, feat)
    for fn, call in (("qa_hcodec_encode", r10.encode), ("qa_hcodec_encode_ragged", lambda: r10.encode_ragged([3, 2])),
                     ("qa_hcodec_forward", r10.forward), ("qa_hcodec_encode_adaptive", r15.encode_adaptive),
                     ("qa_hcodec_forward_adaptive", r15.forward_adaptive)):
        st, msg = call()
        assert st == INVALID and msg.startswith(fn + ":") and f"multiple of {HOP}" in msg and f"{3 * HOP + 1}" in msg, (fn, st, msg)
    assert r10.untouched() and r15.untouched()


def test_a_handle_of_the_other_family(codecs, gpu_device):
    """2. The rectangular entry points on the 1.5 handle and the adaptive ones on the 1.0 handle, all other arguments valid:
    QA_ERR_INVALID, the message names the entry point and the family, nothing is written."""
    wav, feat = _inputs(gpu_device, N * HOP)
    r10, r15 = _Raw(codecs["1.0"], wav, feat), _Raw(codecs["1.5"], wav, feat)
    for fn, call, words in (("qa_hcodec_encode", r15.encode, ("is an H-Codec 1.5 model", "qa_hcodec_encode_adaptive")),
                            ("qa_hcodec_decode", r15.decode, ("is an H-Codec 1.5 model", "qa_hcodec_decode_adaptive")),
                            ("qa_hcodec_forward", r15.forward, ("is an H-Codec 1.5 model", "qa_hcodec_forward_adaptive")),
                            ("qa_hcodec_encode_adaptive", r10.encode_adaptive, ("is not an H-Codec 1.5 model",)),
                            ("qa_hcodec_decode_adaptive", r10.decode_adaptive, ("is not an H-Codec 1.5 model",)),
                            ("qa_hcodec_forward_adaptive", r10.forward_adaptive, ("is not an H-Codec 1.5 model",))):
        st, msg = call()
        assert st == INVALID and msg.startswith(fn + ":") and all(w in msg for w in words), (fn, st, msg)
    assert r10.untouched() and r15.untouched()


@pytest.mark.parametrize("fused", [1, 0], ids=["fused-stage0", "unfused-stage0"])
def test_equal_lengths_are_the_call_without_lengths(codecs, gpu_device, fused):
    """3. lengths = [9, 9]: encode and decode give the bits of the calls without lengths.  At 144 samples the rectangular encode takes
    the fused stage 0 (32 filters, L >= 8), which a truly ragged call never does; QA_SEANET_FUSED = 0 is the other rectangular graph."""
    codec = codecs["1.0"]
    wav, feat = _inputs(gpu_device, N * HOP, seed=21 + fused)
    with with_knob("QA_SEANET_FUSED", fused):
        ac, sc = codec.encode(wav, feat)
        ac2, sc2 = codec.encode(wav, feat, lengths=[N] * B)
        w = codec.decode(ac, sc)
        w2 = codec.decode(ac, sc, lengths=[N] * B)
    assert ac.shape == (B, MINI["num_quantizers"], N) and w.shape == (B, N * HOP)
    assert torch.equal(ac, ac2) and torch.equal(sc, sc2) and torch.equal(w, w2)
    assert bool((ac2 >= 0).all()) and bool((sc2 >= 0).all()) and bool(torch.isfinite(w2).all())


def test_a_feature_count_that_does_not_fit_the_code_frames(codecs, gpu_device):
    """4. qa_hcodec_encode_ragged with n_feat != N * 2: QA_ERR_INVALID, the message names both counts, nothing is written."""
    wav, feat = _inputs(gpu_device, N * HOP)
    r = _Raw(codecs["1.0"], wav, feat)
    for frames in ([N, N - 1], [N, N]):
        st, msg = r.encode_ragged(frames, n_feat=2 * N - 2)
        assert st == INVALID and msg.startswith("qa_hcodec_encode_ragged:") and f"{2 * N - 2} frames" in msg and f"need {2 * N}" in msg, (st, msg)
    assert r.untouched()
