"""The handle-owned device array of a call's per-row lengths (DeviceInts, csrc/host_util.h) across a growth: one
BiCodec tokenizer handle called with per-clip lengths at B = 3, then B = 260 (past the 256 rows of the first allocation and of one upload
launch), then B = 3 again - and, on a fresh handle, tokenize with BOTH length vectors at B = 260 as the first per-clip call, so that the
two vectors of one call are uploaded across the growth.

Every row of every call equals, bit for bit, the same clip run alone through the rectangular B = 1 call (the assertion of
tests/test_bicodec_ragged_gpu.py, at its tolerance of zero).  The rows of a batch cycle through four clips at four lengths, so the clips
run alone are four calls, made once on a handle of their own.  The small tokenizer of tests/bicodec_ragged_cases.py; feature frames
(8, 5, 3, 1) in N = 8, samples (800, 640, 523, 400) in T = 800, reference clip 4800 samples."""
import functools

import pytest
import torch

from tests import bicodec_ragged_cases as K
from unified_audio_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FRAMES = (8, 5, 3, 1)
SAMPLES = (800, 640, 523, 400)
SEED = 251
BIG = 260


def _model():
    import unified_audio_amd as qa

    espec, dspec, sd = K.encoder_sd(K.ENC_SMALL, SEED)
    return qa.BiCodec(dspec, device=DEV, encoder_spec=espec).load_state_dict(sd)


@functools.lru_cache(maxsize=None)
def _alone():
    """the four clips and what the rectangular B = 1 calls return for each of them alone; built once, never modified"""
    m = _model()
    feat = synth.synth_feat(SEED + 5, 4, max(FRAMES), K.ENC_SMALL["input_channels"]).transpose(1, 2).contiguous().to(DEV)
    wav = (synth.synth_wav(SEED + 6, 4, max(SAMPLES)) * torch.tensor([[1.0], [0.3], [2.0], [0.7]]) + 0.05).to(DEV)
    sem = torch.full((4, max(FRAMES)), -1, dtype=torch.int64, device=DEV)
    glob = []
    for i, (n, t) in enumerate(zip(FRAMES, SAMPLES)):
        sem[i, :n] = m.get_semantic_tokens({"feat": feat[i:i + 1, :n].contiguous()})[0]
        glob.append(m.get_global_tokens({"ref_wav": wav[i:i + 1, :t].contiguous()}, K.REF_LEN)[0])
    torch.cuda.synchronize()
    return dict(feat=feat, wav=wav, sem=sem, glob=torch.stack(glob))


def _batch(B):
    """B rows cycling through the four clips: inputs, lengths and the expected rows"""
    a = _alone()
    idx = torch.arange(B, device=DEV) % 4
    lens = lambda v: [v[b % 4] for b in range(B)]  # noqa: E731
    return dict(feat=a["feat"][idx].contiguous(), wav=a["wav"][idx].contiguous(), frames=lens(FRAMES), samples=lens(SAMPLES),
                sem=a["sem"][idx], glob=a["glob"][idx])


def test_semantic_rows_across_a_growth_of_the_length_array(qa_lib, gpu_device):
    m = _model()
    for B in (3, BIG, 3):
        c = _batch(B)
        assert any(n < max(FRAMES) for n in c["frames"])
        got = m.get_semantic_tokens({"feat": c["feat"]}, lengths=c["frames"])
        assert got.shape == (B, max(FRAMES)) and torch.equal(got, c["sem"]), B


def test_both_vectors_of_the_first_tokenize_call_cross_the_growth(qa_lib, gpu_device):
    m = _model()
    for B in (BIG, 3):
        c = _batch(B)
        sem, glob = m.tokenize({"feat": c["feat"], "ref_wav": c["wav"]}, K.REF_LEN, lengths=c["samples"], frame_lengths=c["frames"])
        assert torch.equal(sem, c["sem"]), B
        assert glob.shape == c["glob"].shape and torch.equal(glob, c["glob"]), B
