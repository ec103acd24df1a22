"""UniSE driver on the HIP components with enrollments of different lengths: the segments of all utterances go through ONE ragged
LLM_SFT.generate, and every utterance's tokens equal the ones it gets alone (the reference's one-file-per-step mode).  The prompts stay
below 1024 cache positions, where a row of a ragged call equals the sequence alone bit for bit (tests/test_lm_ragged_gpu.py)."""
import pytest
import torch

from tests.test_unise_driver_gpu import _components

pytestmark = pytest.mark.gpu


def test_mixed_enrollments_equal_one_utterance_at_a_time(qa_lib, gpu_device):
    from unified_audio_amd import unise as U

    fx, lm = _components(gpu_device)
    calls = []
    real = lm.generate

    def spy(*a, **kw):
        calls.append(kw.get("enroll_lengths"))
        return real(*a, **kw)

    lm.generate = spy
    g = torch.Generator().manual_seed(2)
    srcs = [(torch.randn(1, n, generator=g) * 0.1).to(gpu_device) for n in (70000, 170001, 80000, 90000)]  # 1 + 3 + 1 + 2 segments
    enrs = [(torch.randn(1, n, generator=g) * 0.1).to(gpu_device) for n in (32000, 48000, 32000, 80000)]
    for drv in (U.UniSE(lm, fx), U.UniSE(lm, fx, max_segments=3)):
        calls.clear()
        batched = drv.enhance_tokens("tse", srcs, enrs)
        assert all(c is not None and len(set(c)) > 1 for c in calls[:1]) and len(calls) == (1 if drv.max_segments > 7 else 3)
        assert [b[0].shape for b in batched] == [(1, 32), (3, 32), (1, 32), (2, 32)]
        for i, src in enumerate(srcs):
            calls.clear()
            one = drv.enhance_tokens("tse", [src], [enrs[i]])[0]
            assert calls == [None]
            assert torch.equal(one[0], batched[i][0]) and torch.equal(one[1], batched[i][1]), i
