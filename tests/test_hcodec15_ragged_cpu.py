"""Per-clip lengths of the H-Codec 1.5 entry points, the parts that need no GPU: why a per-clip call exists at all
(two facts about the reference's batch semantics, on the CPU oracle), the wire format's length-0 entry, the three C-ABI symbols, and the
argument checks made on the host."""
import ctypes as C
import dataclasses
import os
import re

import pytest
import torch

from oracle import hcodec15_ref as R15
from oracle import hcodec_ref as R
from oracle import synth
from tests.util import rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOP = 640
TOL = 1e-4  # the project's waveform / embedding tolerance: what "the same answer" means everywhere else in the suite


@pytest.fixture(scope="module")
def small15():
    """SPEC_15 with one aggregator and one bottleneck layer at threshold 0.7, and the inputs of DESIGN.md section 28."""
    spec = dataclasses.replace(R.SPEC_15, agg_layers=1, bt_layers=1, threshold=0.7)
    return spec, synth.hcodec10_state_dict(1234, spec), synth.synth_wav(7, 4, HOP * 70), synth.synth_feat(9, 4, 140, 1024)


def test_a_rectangular_batch_of_equal_clips_is_not_the_clips_alone(small15):
    """Four clips of 33 frames in one rectangular encode: a row with fewer groups than the batch maximum carries padded query tokens that
    the reference attends over unmasked, so its aggregated embedding differs from the clip alone by more than the tolerance."""
    spec, sd, wav, feat = small15
    f = 33
    w, ft = wav[:, None, :HOP * f], feat[:, :, :2 * f]
    taps = {}
    batch = R15.encode(sd, w, ft, spec, taps)
    nseg = (R15.extract_lengths(batch["semantic_codes"], spec.codebook_size)[1] > 0).sum(dim=1).tolist()
    assert min(nseg) < max(nseg), nseg
    worst = 0.0
    for b in range(4):
        t1 = {}
        R15.encode(sd, w[b:b + 1], ft[b:b + 1], spec, t1)
        assert t1["enc.emb_agg"].shape[2] == nseg[b]
        e = rel_err(taps["enc.emb_agg"][b:b + 1, :, :nseg[b]], t1["enc.emb_agg"])
        print(f"clip {b}: {nseg[b]} of {max(nseg)} groups, enc.emb_agg batch vs alone {e:.2e}")
        if nseg[b] == max(nseg):
            assert e < TOL, (b, e)  # no padded query: the row is the clip alone
        worst = max(worst, e)
    assert worst > TOL, worst


def test_a_padded_rectangular_decode_is_not_the_clips_alone(small15):
    """The clip-alone codes of clips of 70 / 33 / 17 / 1 frames, padded with length-0 entries, through one rectangular decode: the
    shorter clips' waveforms differ from the clip alone by far more than the tolerance (their padding frames are keys and neighbours)."""
    spec, sd, wav, feat = small15
    frames = [70, 33, 17, 1]
    alone = [R15.encode(sd, wav[b:b + 1, None, :HOP * f], feat[b:b + 1, :, :2 * f], spec) for b, f in enumerate(frames)]
    G = max(a["semantic_codes"].shape[2] for a in alone)
    q = spec.num_quantizers
    ac, sc = torch.full((4, q, G), -1, dtype=torch.int64), torch.full((4, q, G), -1, dtype=torch.int64)
    for b, a in enumerate(alone):
        g = a["semantic_codes"].shape[2]
        ac[b, :, :g], sc[b, :, :g] = a["acoustic_codes"][0], a["semantic_codes"][0]
    w = R15.decode(sd, ac, sc, spec)
    assert w.shape == (4, 2 * spec.hop * 70)
    for b, (f, a) in enumerate(zip(frames, alone)):
        w1 = R15.decode(sd, a["acoustic_codes"], a["semantic_codes"], spec)
        e = rel_err(w[b, :w1.shape[1]], w1[0])
        print(f"clip {b}: {f} frames, padded rectangular decode vs alone {e:.2e}")
        assert (e > TOL) == (f < 70), (b, f, e)


def test_minus_one_is_a_length_zero_entry():
    """floor(-1 / K) + 1 = 0: the dropped code is a legal padded group of the 1.5 wire format, and contributes no frame."""
    K = 16384
    codes = torch.tensor([[[5 + 2 * K, -1, 7, -1]]])
    plain, lengths = R15.extract_lengths(codes, K)
    assert lengths.tolist() == [[3, 0, 1, 0]] and plain[0, 0].tolist() == [5, K - 1, 7, K - 1]
    assert R15.deaggregate_indices(plain, lengths).shape == (1, 1, 4)


_CTYPE = {"qa_hcodec*": C.c_void_p, "const float*": C.c_void_p, "float*": C.c_void_p, "void*": C.c_void_p, "int64_t": C.c_int64,
          "float": C.c_float}
_HOST = {"frames", "frames_out", "n_groups"}  # host memory: typed pointers, so that ctypes refuses a tensor's data_ptr() there


@pytest.mark.parametrize("name", ["qa_hcodec_encode_adaptive_ragged", "qa_hcodec_adaptive_clip_frames", "qa_hcodec_decode_adaptive_ragged"])
def test_entry_points_are_declared_exported_and_bound(qa_lib, name):
    from unified_audio_amd import _lib

    header = open(os.path.join(ROOT, "include", "quarkaudio.h")).read()
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", header, re.S)
    assert m, f"{name} is not declared in quarkaudio.h"
    args = [(" ".join(a.split()[:-1]), a.split()[-1]) for a in m.group(1).split(",")]
    assert hasattr(qa_lib, name)
    res, bound = _lib.SYMBOLS[name]
    assert res is C.c_int and len(bound) == len(args), (len(bound), args)
    for (ctype, arg), got in zip(args, bound):
        if arg in _HOST:
            assert ctype in ("const int64_t*", "int64_t*") and got is C.POINTER(C.c_int64), (arg, ctype, got)
        else:
            assert got is _CTYPE.get(ctype, C.c_void_p), (name, arg, ctype, got)
    assert args[-1][1] == "stream" and re.search(r"#define QA_VERSION 103\b", header)


def test_null_arguments_are_refused_without_a_device(qa_lib):
    fr = (C.c_int64 * 1)(1)
    g = C.c_int64(0)
    assert qa_lib.qa_hcodec_encode_adaptive_ragged(None, None, 1, 640, fr, None, 0, 0, 0, 2, None, None, C.byref(g), 0.0, None) == -1
    assert b"qa_hcodec_encode_adaptive_ragged" in qa_lib.qa_last_error()
    assert qa_lib.qa_hcodec_adaptive_clip_frames(None, None, 1, 1, fr, None) == -1
    assert b"qa_hcodec_adaptive_clip_frames" in qa_lib.qa_last_error()
    assert qa_lib.qa_hcodec_decode_adaptive_ragged(None, None, None, 1, 1, 1, fr, None, None) == -1
    assert b"qa_hcodec_decode_adaptive_ragged" in qa_lib.qa_last_error()


def test_the_python_methods_check_their_arguments_without_a_device(qa_lib):
    """Codec.encode_ragged / decode_ragged / adaptive_frames refuse what they cannot pass on before they touch the handle (status -1);
    well-formed arguments reach the missing weights (status -3); a 1.0 model has no adaptive_frames (status -4)."""
    import unified_audio_amd as qa

    spec = dataclasses.replace(qa.HCodecSpec(), adaptive=True)
    codec = qa.Codec(None, None, None, spec=spec, device="cuda:0")
    q = spec.num_quantizers
    x, f, c = torch.zeros(2, 1, 640), torch.zeros(2, spec.sem_in, 2), torch.zeros(2, q, 1, dtype=torch.int64)
    bad = [lambda: codec.encode_ragged(x, f, [1]),                      # wrong count
           lambda: codec.encode_ragged(x, f, [1.5, 1]),                 # not an integer
           lambda: codec.encode_ragged(x[:, 0], f, [1, 1]),             # no channel dimension
           lambda: codec.encode_ragged(x, f[:, :3], [1, 1]),            # wrong feature width
           lambda: codec.encode_ragged(x, f, [1, 1], threshold=1.5),
           lambda: codec.decode_ragged(c, c[:, :, :0]),                 # shapes differ
           lambda: codec.decode_ragged(c[:, :q - 1], c[:, :q - 1]),     # wrong quantizer count
           lambda: codec.decode_ragged(c, c, lengths=[1, 1]),           # the lengths ride in the codes
           lambda: codec.adaptive_frames(c[0])]
    for i, call in enumerate(bad):
        with pytest.raises(qa.QuarkAudioError) as e:
            call()
        assert e.value.status == -1, (i, str(e.value))
    for call in (lambda: codec.encode_ragged(x, f, [1, 1]), lambda: codec.decode_ragged(c, c), lambda: codec.adaptive_frames(c)):
        with pytest.raises(qa.QuarkAudioError) as e:
            call()
        assert e.value.status == -3
    with pytest.raises(qa.QuarkAudioError) as e:
        qa.Codec(None, None, None, spec=qa.HCodecSpec(), device="cuda:0").adaptive_frames(c)
    assert e.value.status == -4
