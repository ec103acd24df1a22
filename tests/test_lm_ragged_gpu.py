"""LLM_SFT.generate(..., enroll_lengths=...) / qa_lm_generate_ragged: one call over sequences whose enrollments differ in length
(DESIGN.md section 23).  Row b must be exactly what the sequence gives ALONE with its own enroll_lengths[b] frames.

(1) bit for bit against the B = 1 call of the existing generate, at its logits (taps) and tokens.  The two calls agree to the bit
    because both run 16 key tiles per attention split: att_tps = max(att_split / 16, ceil(cap_tiles / 4)) with att_split = 256 is 16
    for every cache capacity up to 1024 keys, and every case here stays far below that.  Above 1024 keys a longer neighbour can
    widen the splits and the two agree to fp32 rounding only.
(2) oracle parity per row (tokens: _audit at tol 2e-4; decode logits of one row: the fp64 protocol of tests/test_lm_logits_gpu.py).
(3) padding frames are never read, (4) the all-equal vector is the rectangular call, (5) every launch form, (6) sampled,
(7) errors, (8) neighbouring session / score calls are undisturbed.
"""
import functools

import pytest
import torch

from oracle import llm_ref as L
from tests.test_llm_gpu import SMALL, _audit, _model
from tests.test_lm_logits_gpu import H1024, HD32, _parity, _run, _same

pytestmark = pytest.mark.gpu

# (spec, weight seed, enrollment lengths, n_mix, S, G).  small: L_b = 13, 19, 252, 262, 262 - over the 18 steps row 2 crosses key 256 (a
# split boundary of att_split = 256 and a 16-key tile edge), rows 0 and 1 stay in split 0, rows 3 and 4 start in split 1
CASES = {
    "small": (SMALL, 22, [1, 7, 240, 250, 250], 9, 12, 5),
    "hd32": (HD32, 26, [1, 17, 33], 9, 12, 5),
    "h1024": (H1024, 28, [1, 17, 33], 9, 12, 5),
    "unise": (L.SPEC_UNISE, 33, [5, 40], 20, 20, 5),
}


def _inputs(spec, lens, Nm, seed):
    """enroll_feats [B, max(lens), F] (the frames behind a row's length keep their random values: padding may hold anything) and mix."""
    return L.synth_feats(seed + 1, len(lens), max(lens), spec.feats_dim), L.synth_feats(seed, len(lens), Nm, spec.feats_dim)


def _ragged(lm, spec, dev, enr, mix, lens, S, G, **kw):
    return _run(lm, spec, dev, "tse", enr, mix, S, G, enroll_lengths=lens, **kw)


def _solo(lm, spec, dev, enr, mix, lens, b, S, G, **kw):
    """Sequence b alone through the EXISTING call, with its own frames only."""
    return _run(lm, spec, dev, "tse", enr[b:b + 1, :lens[b]].contiguous(), mix[b:b + 1], S, G, **kw)


def _rows_equal_solo(lm, spec, dev, enr, mix, lens, S, G, got, rows, label=""):
    bad = []
    for b in rows:
        alone = _solo(lm, spec, dev, enr, mix, lens, b, S, G)
        if not _same([t[b:b + 1] for t in got], alone):
            bad.append(b)
    assert not bad, f"{label}: rows whose logits / tokens differ from the same sequence alone: {bad}"


@functools.lru_cache(maxsize=None)
def _case(name, dev):
    """One ragged call and the solo call of every row, computed once and shared by the tests below (never modified)."""
    spec, seed, lens, Nm, S, G = CASES[name]
    sd, lm = _model(spec, seed, dev)
    enr, mix = _inputs(spec, lens, Nm, seed + 100)
    got = _ragged(lm, spec, dev, enr, mix, lens, S, G)
    solo = [_solo(lm, spec, dev, enr, mix, lens, b, S, G) for b in range(len(lens))]
    return sd, lm, enr, mix, got, solo


@pytest.mark.parametrize("name", list(CASES))
def test_each_row_equals_itself_alone_bit_for_bit(qa_lib, gpu_device, name):
    spec, _, lens, _, S, G = CASES[name]
    _, _, _, _, got, solo = _case(name, gpu_device)
    assert all(torch.isfinite(t).all() for t in got[2:])
    assert got[0].shape == (len(lens), G) and got[1].shape == (len(lens), S)
    for b, alone in enumerate(solo):
        for what, x, y in zip(("global ids", "semantic ids", "logits.global", "logits.semantic"), got, alone):
            assert torch.equal(x[b:b + 1], y), f"{name}: row {b} (enrollment {lens[b]}): {what} differ from the sequence alone"


@pytest.mark.parametrize("name", ["small", "unise"])
def test_each_row_matches_the_oracle_on_its_own_enrollment(qa_lib, gpu_device, name):
    spec, _, lens, _, S, G = CASES[name]
    sd, _, enr, mix, got, _ = _case(name, gpu_device)
    for b, n in enumerate(lens):
        free_match, near_ties = _audit(sd, spec, "tse", enr[b:b + 1, :n], mix[b:b + 1], S, G, got[0][b:b + 1], got[1][b:b + 1], tol=2e-4)
        print(f"{name} row {b}: free-running agreement {free_match}, near-tie flips {near_ties}")
        assert near_ties > 0 or free_match == 1.0, (name, b)


def test_decode_logits_of_a_ragged_row_match_the_fp64_oracle(qa_lib, gpu_device):
    """Row 2 of the small case (the one that crosses key 256): C_PARITY * max(e_cpu32, E_FLOOR), teacher-forced on its own stream."""
    spec, _, lens, _, S, G = CASES["small"]
    sd, _, enr, mix, got, _ = _case("small", gpu_device)
    b = 2
    g, s, lg, ls = (t[b:b + 1] for t in got)
    _parity(sd, spec, "tse", enr[b:b + 1, :lens[b]], mix[b:b + 1], S, G, g, s, lg, ls, "ragged_small_row2")


def _poisoned(enr, lens, value):
    out = enr.clone()
    for b, n in enumerate(lens):
        out[b, n:] = value
    return out


def test_padding_frames_are_never_read(qa_lib, gpu_device):
    spec, _, lens, _, S, G = CASES["small"]
    _, lm, enr, mix, got, _ = _case("small", gpu_device)
    for value in (float("nan"), 1e30, 0.0):
        out = _ragged(lm, spec, gpu_device, _poisoned(enr, lens, value), mix, lens, S, G)
        assert all(torch.isfinite(t).all() for t in out[2:]), value
        assert _same(out, got), f"padding frames set to {value} changed the result"


def test_all_equal_lengths_are_the_rectangular_call(qa_lib, gpu_device):
    spec, S, G = SMALL, 12, 5
    _, lm = _model(spec, 22, gpu_device)
    enr, mix = _inputs(spec, [7] * 5, 9, 140)
    for kw in (dict(do_sample=False), dict(do_sample=True)):
        torch.manual_seed(11)
        plain = _run(lm, spec, gpu_device, "tse", enr, mix, S, G, **kw)
        torch.manual_seed(11)
        assert _same(_ragged(lm, spec, gpu_device, enr, mix, [7] * 5, S, G, **kw), plain), kw


def _seeded_lengths(B, seed, top=40):
    gen = torch.Generator().manual_seed(seed)
    lens = torch.randint(1, top + 1, (B,), generator=gen).tolist()
    lens[0], lens[-1] = top, 1  # n_enroll_max is `top` whatever the draw; the last row is the shortest
    return lens


@pytest.mark.parametrize("B,rows", [(12, (0, 7, 8, 11)), (33, (0, 16, 17, 32)), (65, (0, 32, 33, 64))])
def test_every_launch_form_gives_the_same_bits(qa_lib, gpu_device, knob, B, rows):
    """QA_LM_GRAPH 0 / 1, QA_LM_CHAINS 1 / 2 and QA_LM_ROWSPLIT 0 .. 3 on seeded lengths from 1 .. 40: 12 rows take the 8-row split,
    33 two row tiles (two chains of 17 + 16 under QA_LM_CHAINS=2), 65 always two chains of 33 + 32 replaying captured steps - the
    offsets of a chain are its slice at b0, and the lengths differ on both sides of every boundary."""
    spec, Nm, S, G = SMALL, 6, 8, 4
    _, lm = _model(spec, 46, gpu_device)
    lens = _seeded_lengths(B, 50 + B)
    assert len(set(lens[:B // 2])) > 1 and len(set(lens[B // 2:])) > 1 and lens[rows[1]] != lens[rows[2]]
    enr, mix = _inputs(spec, lens, Nm, 60 + B)
    ref = _ragged(lm, spec, gpu_device, enr, mix, lens, S, G)
    _rows_equal_solo(lm, spec, gpu_device, enr, mix, lens, S, G, ref, rows, f"B={B}")
    for graph in (0, 1):
        knob("QA_LM_GRAPH", graph)
        for chains in (1, 2):
            knob("QA_LM_CHAINS", chains)
            assert _same(_ragged(lm, spec, gpu_device, enr, mix, lens, S, G), ref), (graph, chains)
        knob("QA_LM_CHAINS", 0)
        for rs in (0, 1, 2, 3):
            knob("QA_LM_ROWSPLIT", rs)
            assert _same(_ragged(lm, spec, gpu_device, enr, mix, lens, S, G), ref), (graph, rs)


def test_a_captured_step_serves_every_length_vector(qa_lib, gpu_device, knob):
    """Two length vectors of equal n_enroll_max back to back under QA_LM_GRAPH=1: the step graph is keyed by the shapes, never by the
    lengths (they live in device memory), so the second call replays the first one's graph - and is still each row alone."""
    spec, Nm, S, G = SMALL, 6, 8, 4
    _, lm = _model(spec, 46, gpu_device)
    first, second = [40, 3, 17, 40, 1, 22], [2, 40, 40, 9, 31, 5]
    enr, mix = _inputs(spec, first, Nm, 70)
    knob("QA_LM_GRAPH", 1)
    a = _ragged(lm, spec, gpu_device, enr, mix, first, S, G)
    b = _ragged(lm, spec, gpu_device, enr, mix, second, S, G)
    a2 = _ragged(lm, spec, gpu_device, enr, mix, first, S, G)
    assert _same(a, a2)
    knob("QA_LM_GRAPH", 0)
    _rows_equal_solo(lm, spec, gpu_device, enr, mix, second, S, G, b, range(6), "second vector")
    _rows_equal_solo(lm, spec, gpu_device, enr, mix, first, S, G, a, range(6), "first vector")


def test_sampled_ragged_call(qa_lib, gpu_device):
    spec, _, lens, _, S, G = CASES["small"]
    _, lm, enr, mix, _, _ = _case("small", gpu_device)
    torch.manual_seed(7)
    one = _ragged(lm, spec, gpu_device, enr, mix, lens, S, G, do_sample=True)
    torch.manual_seed(7)
    two = _ragged(lm, spec, gpu_device, enr, mix, lens, S, G, do_sample=True)
    assert _same(one, two), "a fixed seed does not repeat"
    # the sampler's Philox stream is keyed by (seed, GLOBAL sequence index, step): row 0 has index 0 in both calls
    torch.manual_seed(7)
    alone = _solo(lm, spec, gpu_device, enr, mix, lens, 0, S, G, do_sample=True)
    assert _same([t[:1] for t in one], alone), "row 0 differs from its solo sampled run with the same seed"
    torch.manual_seed(7)
    poisoned = _ragged(lm, spec, gpu_device, _poisoned(enr, lens, float("nan")), mix, lens, S, G, do_sample=True)
    assert torch.equal(poisoned[0], one[0]) and torch.equal(poisoned[1], one[1]), "poisoned padding changed a sampled token"
    assert int(one[0].min()) >= 0 and int(one[0].max()) < spec.global_size and int(one[1].max()) < spec.semantic_size


def test_errors_name_their_cause_and_leave_the_handle_usable(qa_lib, gpu_device):
    import unified_audio_amd as qa

    spec, S, G = SMALL, 6, 3
    _, lm = _model(spec, 21, gpu_device)
    enr, mix = _inputs(spec, [5, 5, 5], 4, 80)
    mel = torch.zeros(3, S, 80)
    dev = gpu_device

    def plain():
        g, s = lm.generate("tse", mel, enr.to(dev), mel, mix.to(dev), global_length=G, do_sample=False)
        return g.cpu(), s.cpu()

    usual = plain()
    long_enr = torch.zeros(3, 4096, spec.feats_dim)
    for kw, enroll, match in (
            (dict(enroll_lengths=[5, 0, 5]), enr, r"n_enroll\[1\] = 0 .*1 \.\. n_enroll_max = 5"),
            (dict(enroll_lengths=[5, 5, 6]), enr, r"n_enroll\[2\] = 6 .*n_enroll_max = 5"),
            (dict(enroll_lengths=[-3, 5, 5]), enr, r"n_enroll\[0\] = -3"),
            (dict(enroll_lengths=[5, 5]), enr, r"2 entries for a batch of 3"),
            (dict(enroll_lengths=torch.tensor([5, 5, 5])), None, r"need enroll_feats"),
            (dict(enroll_lengths=[4096, 1, 1]), long_enr, r"exceed max_position_embeddings 4096"),
    ):
        for do_sample in (False, True):
            with pytest.raises(qa.QuarkAudioError, match=match):
                lm.generate("tse", None if enroll is None else mel, None if enroll is None else enroll.to(dev), mel, mix.to(dev),
                            global_length=G, do_sample=do_sample, **kw)
            assert _same(plain(), usual), (kw, do_sample)
    # and a good ragged call still works afterwards
    g, s = lm.generate("tse", mel, enr.to(dev), mel, mix.to(dev), global_length=G, do_sample=False, enroll_lengths=[5, 5, 5])
    assert _same((g.cpu(), s.cpu()), usual)


def test_neighbouring_session_and_score_calls_are_undisturbed(qa_lib, gpu_device):
    """The pattern of tests/test_lm_session_gpu.py::test_invariances_are_bit_exact: a ragged call between two session calls, and between
    two score calls, changes neither side - and is itself what it was."""
    import unified_audio_amd as qa
    from tests.test_lm_session_gpu import _embeds, _feed

    spec, dev = SMALL, gpu_device
    sd, lm = _model(spec, 21, dev)
    lens, Nm, S, G = [3, 11, 6, 11], 9, 8, 4
    enr, mix = _inputs(spec, lens, Nm, 90)
    mel = torch.zeros(4, S, 80)

    def ragged():
        g, s = lm.generate("tse", mel, enr.to(dev), mel, mix.to(dev), global_length=G, do_sample=False, enroll_lengths=lens)
        return g.cpu(), s.cpu()

    r0 = ragged()
    x = _embeds(sd, spec, 6, 5, 12)
    schedule = [7, 1, 3, 1]
    cache = qa.KVCache(lm, 5, 16)
    first = _feed(lm, dev, cache, x, schedule)
    cache.reset()
    a = _feed(lm, dev, cache, x, schedule[:2])
    r1 = ragged()
    b = _feed(lm, dev, cache, x[:, 8:], schedule[2:])
    assert torch.equal(torch.cat([a, b], dim=1), first)
    assert _same(r0, r1)
    score = lambda: [t.cpu() for t in lm.score("tse", mel, enr.to(dev), mel, mix.to(dev), r0[0], r0[1])]
    s0 = score()
    r2 = ragged()
    s1 = score()
    assert _same(s0, s1) and _same(r0, r2)
