"""Host logic of UniSE(tail="trim"): an utterance gives its full 5 s segments plus one last segment at its own length, and every stage of
a micro-batch - front-end, LM, detokenizer - is handed the rows' own sample / frame / token counts.  tail="wrap" makes the calls it
always made.  Stand-in models that record their arguments, in the style of tests/test_unise_ragged_cpu.py; no GPU."""
import pytest
import torch

from unified_audio_amd import unise as U

HOP = 320  # the stand-in front-end's frame rate: samples // 320 frames


def _fakes(lengths=True):
    log = {"ssl": [], "lm": [], "detok": []}

    class FakeSSL:
        def frames(self, n):
            return n // HOP

        def __call__(self, wavs, lengths=None):
            log["ssl"].append(dict(shape=tuple(wavs.shape), lengths=None if lengths is None else list(lengths), wavs=wavs.clone()))
            n = wavs.shape[1] // HOP
            return wavs[:, :n * HOP:HOP].unsqueeze(-1).repeat(1, 1, 4)  # [B, n, 4]: frame t carries sample 320 t

    class PlainSSL:
        def __call__(self, wavs):
            return FakeSSL()(wavs)

    class FakeLM:
        def generate(self, task_name, enroll_mel, enroll_feats, mix_mel, mix_feats, do_sample, enroll_lengths=None, mix_lengths=None,
                     semantic_lengths=None):
            B, S = mix_feats.shape[0], mix_mel.size(1)
            log["lm"].append(dict(task=task_name, B=B, S=S, mix=tuple(mix_feats.shape), enroll_lengths=enroll_lengths, mix_lengths=mix_lengths,
                                  semantic_lengths=semantic_lengths))
            ns = semantic_lengths if semantic_lengths is not None else [S] * B
            sids = torch.full((B, S), -1, dtype=torch.long)
            for b in range(B):  # token t of a row: its index, so that the detokenizer below can be checked sample by sample
                sids[b, :ns[b]] = torch.arange(ns[b])
            return torch.zeros(B, 32, dtype=torch.long), sids

    class PlainLM:
        def generate(self, task_name, enroll_mel, enroll_feats, mix_mel, mix_feats, do_sample):
            return FakeLM().generate(task_name, enroll_mel, enroll_feats, mix_mel, mix_feats, do_sample)

    def detokenize(global_tokens, semantic_tokens, lengths=None):
        log["detok"].append(dict(shape=tuple(semantic_tokens.shape), lengths=None if lengths is None else list(lengths)))
        return semantic_tokens.float().repeat_interleave(HOP, dim=1).unsqueeze(1)  # sample i of a row carries its token index i // 320

    def plain_detokenize(global_tokens, semantic_tokens):
        return detokenize(global_tokens, semantic_tokens)

    return log, (FakeLM() if lengths else PlainLM()), (FakeSSL() if lengths else PlainSSL()), (detokenize if lengths else plain_detokenize)


# 0.4 s (the min_tail wrap), 2 s, 5 s (no tail at all), 7.3 s (one full segment and a tail of 36800 samples)
LENGTHS = (6400, 32000, 80000, 116800)


def _utterances():
    g = torch.Generator().manual_seed(5)
    return [torch.randn(1, n, generator=g) for n in LENGTHS]


def test_trim_hands_every_stage_the_rows_own_lengths():
    log, lm, ssl, detok = _fakes()
    drv = U.UniSE(lm, ssl, detokenize=detok, tail="trim")
    srcs = _utterances()
    out = drv.enhance("se", srcs)
    samples = [16000, 32000, 80000, 80000, 36800]  # 1 + 1 + 1 + 2 segments
    assert [U.trim_samples(n) for n in LENGTHS] == [[16000], [32000], [80000], [80000, 36800]]
    # front-end: one call over the five segments with their sample counts
    assert len(log["ssl"]) == 1 and log["ssl"][0]["shape"] == (5, 80000) and log["ssl"][0]["lengths"] == samples
    wavs = log["ssl"][0]["wavs"]
    # the 0.4 s utterance wraps around up to min_tail; every row is zero behind its samples; 'se' divides by the WHOLE utterance's peak
    peak = [float(s.abs().max()) for s in srcs]
    assert torch.equal(wavs[0, :16000], torch.cat([srcs[0][0]] * 3)[:16000] / peak[0])
    assert torch.equal(wavs[4, :36800], srcs[3][0, 80000:] / peak[3]) and torch.equal(wavs[3], srcs[3][0, :80000] / peak[3])
    assert all(bool((wavs[i, n:] == 0).all()) for i, n in enumerate(samples))
    # LM: one call, frames and tokens per row
    assert len(log["lm"]) == 1
    call = log["lm"][0]
    assert call["B"] == 5 and call["S"] == 250 and call["mix"] == (5, 250, 4) and call["enroll_lengths"] is None
    assert call["mix_lengths"] == [50, 100, 250, 250, 115] and call["semantic_lengths"] == [50, 100, 250, 250, 115]
    # detokenizer: the same token counts
    assert log["detok"] == [dict(shape=(5, 250), lengths=[50, 100, 250, 250, 115])]
    # every utterance comes back at exactly its own length, its rows joined: sample i of a row carries token i // 320
    assert [tuple(o.shape) for o in out] == [(n,) for n in LENGTHS]
    assert torch.equal(out[3], torch.cat([torch.arange(80000) // HOP, torch.arange(36800) // HOP]).float())
    assert torch.equal(out[0], (torch.arange(6400) // HOP).float())
    toks = drv.enhance_tokens("se", srcs)
    assert [tuple(t[1].shape) for t in toks] == [(1, 250), (1, 250), (1, 250), (2, 250)]
    assert bool((toks[0][1][0, 50:] == -1).all()) and bool((toks[3][1][1, 115:] == -1).all()) and int(toks[3][1][1, 114]) == 114


def test_trim_micro_batches_run_at_their_own_longest_row():
    """max_segments = 2 over 1 + 1 + 1 + 2 segments: [0.4 s, 2 s] [5 s, 5 s] [2.3 s] - the first and the last micro-batch are cut to
    their longest row, the middle one has no tail and makes the calls without lengths; the results do not depend on the split."""
    log, lm, ssl, detok = _fakes()
    srcs = _utterances()
    ref = U.UniSE(lm, ssl, detokenize=detok, tail="trim").enhance("se", srcs)
    for k in log:
        log[k].clear()
    out = U.UniSE(lm, ssl, detokenize=detok, tail="trim", max_segments=2).enhance("se", srcs)
    assert [(c["shape"], c["lengths"]) for c in log["ssl"]] == [((2, 32000), [16000, 32000]), ((2, 80000), None), ((1, 36800), [36800])]
    assert [(c["S"], c["mix"], c["mix_lengths"], c["semantic_lengths"]) for c in log["lm"]] == [
        (100, (2, 100, 4), [50, 100], [50, 100]), (250, (2, 250, 4), None, None), (115, (1, 115, 4), [115], [115])]
    assert log["detok"] == [dict(shape=(2, 100), lengths=[50, 100]), dict(shape=(2, 250), lengths=None), dict(shape=(1, 115), lengths=[115])]
    assert all(torch.equal(a, b) for a, b in zip(ref, out))


def test_trim_with_enrollments_keeps_their_lengths_too():
    log, lm, ssl, detok = _fakes()
    drv = U.UniSE(lm, ssl, detokenize=detok, tail="trim")
    srcs = _utterances()[1::2]  # 2 s and 7.3 s: 1 + 2 segments
    enrs = [torch.ones(1, 32000), torch.ones(1, 48000)]
    out = drv.enhance("tse", srcs, enrs)
    call = log["lm"][-1]
    assert call["enroll_lengths"] == [100, 150, 150] and call["mix_lengths"] == [100, 250, 115] and call["semantic_lengths"] == [100, 250, 115]
    assert torch.equal(log["ssl"][-1]["wavs"][2, :36800], srcs[1][0, 80000:]), "'tse' does not normalise"
    assert [tuple(o.shape) for o in out] == [(32000,), (116800,)]


def test_trim_is_refused_at_construction_when_a_stage_cannot_take_lengths():
    _, lm, ssl, detok = _fakes()
    _, plain_lm, plain_ssl, plain_detok = _fakes(lengths=False)
    with pytest.raises(TypeError, match=r"dnn\.generate"):
        U.UniSE(plain_lm, ssl, detokenize=detok, tail="trim")
    with pytest.raises(TypeError, match=r"semantic_model\(wavs, lengths=\)"):
        U.UniSE(lm, plain_ssl, detokenize=detok, tail="trim")
    with pytest.raises(TypeError, match=r"detokenize\(global_tokens, semantic_tokens, lengths=\)"):
        U.UniSE(lm, ssl, detokenize=plain_detok, tail="trim")
    with pytest.raises(ValueError, match="tail must be"):
        U.UniSE(lm, ssl, detokenize=detok, tail="cut")
    U.UniSE(plain_lm, plain_ssl, detokenize=plain_detok)  # the default asks for none of it
    U.UniSE(lm, ssl, tail="trim")  # tokens only: no detokenizer to ask


def test_wrap_makes_the_calls_it_always_made():
    log, lm, ssl, detok = _fakes()
    srcs = _utterances()
    default = U.UniSE(lm, ssl, detokenize=detok).enhance("se", srcs)
    calls = {k: [{n: v for n, v in c.items() if n != "wavs"} for c in log[k]] for k in log}
    wavs = log["ssl"][0]["wavs"]
    for k in log:
        log[k].clear()
    wrap = U.UniSE(lm, ssl, detokenize=detok, tail="wrap").enhance("se", srcs)
    assert {k: [{n: v for n, v in c.items() if n != "wavs"} for c in log[k]] for k in log} == calls
    assert torch.equal(log["ssl"][0]["wavs"], wavs) and all(torch.equal(a, b) for a, b in zip(default, wrap))
    # five wrap-padded 5 s segments through calls without any length
    assert calls["ssl"] == [dict(shape=(5, 80000), lengths=None)] and calls["detok"] == [dict(shape=(5, 250), lengths=None)]
    assert [(c["S"], c["mix_lengths"], c["semantic_lengths"]) for c in calls["lm"]] == [(250, None, None)]
    assert torch.equal(wavs[0], U.wrap_pad(srcs[0])[0] / srcs[0].abs().max())
