"""Host logic of the UniSE driver for enrollments of different lengths: ONE ragged LLM_SFT.generate over the segments of all
utterances (enroll_lengths = every segment's own feature-frame count), the front-end once per distinct length, results in the caller's
order, and equal lengths through the call without the keyword.  Stand-in models; no GPU."""
import torch

from unified_audio_amd import unise as U

HOP = 320  # the stand-in front-end's frame rate: samples // 320 frames


def _fakes():
    log = {"ssl": [], "lm": []}

    class FakeSSL:
        def __call__(self, wavs):
            log["ssl"].append(tuple(wavs.shape))
            n = wavs.shape[1] // HOP
            return wavs[:, :n * HOP:HOP].unsqueeze(-1).repeat(1, 1, 4)  # [B, n, 4]: frame t carries sample 320 t

    class FakeLM:
        def generate(self, task_name, enroll_mel, enroll_feats, mix_mel, mix_feats, do_sample, **kw):
            B = mix_feats.shape[0]
            log["lm"].append(dict(task=task_name, B=B, kw=dict(kw), enroll=enroll_feats.clone(), Ne=enroll_mel.size(1)))
            # a token stream that depends on the segment AND on the valid part of its enrollment
            lens = kw.get("enroll_lengths", [enroll_feats.shape[1]] * B)
            tag = torch.stack([mix_feats[b, 0, 0] * 1000 + enroll_feats[b, :lens[b], 0].sum() for b in range(B)])
            return tag.view(B, 1).repeat(1, 32).round().long(), tag.view(B, 1).repeat(1, mix_mel.size(1)).round().long()

    return log, FakeLM(), FakeSSL()


def _utterances():
    g = torch.Generator().manual_seed(5)
    srcs = [torch.randn(1, n, generator=g) for n in (90000, 170000, 80000, 100000)]  # 2 + 3 + 1 + 2 segments
    enrs = [torch.full((1, n), float(i + 1)) for i, n in enumerate((32000, 48000, 32000, 80000))]
    return srcs, enrs


def test_mixed_enrollment_lengths_make_one_ragged_generate_call():
    log, lm, ssl = _fakes()
    drv = U.UniSE(lm, ssl)
    srcs, enrs = _utterances()
    out = drv.enhance_tokens("tse", srcs, enrs)
    assert len(log["lm"]) == 1, f"{len(log['lm'])} generate calls: the LM pass is still grouped by enrollment length"
    call = log["lm"][0]
    frames = {32000: 100, 48000: 150, 80000: 250}
    per_segment = [100] * 2 + [150] * 3 + [100] * 1 + [250] * 2
    assert call["B"] == 8 and list(call["kw"]["enroll_lengths"]) == per_segment
    # the features are padded to the longest enrollment and tiled over each utterance's segments, in the caller's order
    e = call["enroll"]
    assert e.shape == (8, 250, 4)
    for row, (utt, n) in enumerate(zip([0, 0, 1, 1, 1, 2, 3, 3], per_segment)):
        assert (e[row, :n] == float(utt + 1)).all() and (e[row, n:] == 0).all(), row
    assert call["Ne"] == U.mel_frames(80000)
    # the front-end: once per DISTINCT enrollment length (never on a zero-padded waveform), then once on the segments
    assert sorted(log["ssl"][:-1]) == [(1, 48000), (1, 80000), (2, 32000)] and log["ssl"][-1] == (8, 80000)
    assert all(frames[s[1]] == s[1] // HOP for s in log["ssl"][:-1])
    # results in the caller's order, equal to one utterance at a time
    assert [o[0].shape[0] for o in out] == [2, 3, 1, 2]
    for i, (src, enr) in enumerate(zip(srcs, enrs)):
        one = drv.enhance_tokens("tse", [src], [enr])[0]
        assert torch.equal(one[0], out[i][0]) and torch.equal(one[1], out[i][1]), i
        assert "enroll_lengths" not in log["lm"][-1]["kw"]


def test_equal_enrollment_lengths_take_the_call_without_the_keyword():
    log, lm, ssl = _fakes()
    drv = U.UniSE(lm, ssl)
    srcs, _ = _utterances()
    enrs = [torch.full((1, 48000), float(i + 1)) for i in range(4)]
    drv.enhance_tokens("tse", srcs, enrs)
    assert len(log["lm"]) == 1 and log["lm"][0]["kw"] == {} and log["lm"][0]["enroll"].shape == (8, 150, 4)
    assert log["ssl"] == [(4, 48000), (8, 80000)]


def test_micro_batches_carry_their_own_lengths_and_trim_to_their_longest():
    """max_segments = 3 over 2 + 3 + 1 + 2 segments: [u0 u0 u1] [u1 u1 u2] [u3 u3] - each micro-batch one generate call, ragged only
    where its lengths differ, its features trimmed to its own longest enrollment; tokens as with one big batch."""
    log, lm, ssl = _fakes()
    srcs, enrs = _utterances()
    ref = U.UniSE(lm, ssl).enhance_tokens("tse", srcs, enrs)
    log["lm"].clear()
    out = U.UniSE(lm, ssl, max_segments=3).enhance_tokens("tse", srcs, enrs)
    calls = log["lm"]
    assert [c["B"] for c in calls] == [3, 3, 2]
    assert [c["kw"].get("enroll_lengths") for c in calls] == [[100, 100, 150], [150, 150, 100], None]
    assert [c["enroll"].shape[1] for c in calls] == [150, 150, 250]
    for (g0, s0), (g1, s1) in zip(ref, out):
        assert torch.equal(g0, g1) and torch.equal(s0, s1)
