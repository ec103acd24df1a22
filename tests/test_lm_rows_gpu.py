"""LLM_SFT.generate(..., enroll_lengths=, mix_lengths=, semantic_lengths=) / qa_lm_generate_rows: one call over sequences whose
enrollments, mixtures and semantic lengths differ.  Row b must be exactly what the sequence gives ALONE on its
own frames with its own number of semantic steps.

(1) bit for bit against the B = 1 call of the existing generate, at its logits (taps) and tokens, over the row's own columns; behind
    them the ids are -1 and the tap exactly 0.  Every case stays below 1024 cache positions, where both calls run 16 key tiles per
    attention split (tests/test_lm_ragged_gpu.py explains why that makes "alone" bit-equal).
(2) oracle parity per row (_audit at tol 2e-4; the fp64 protocol of tests/test_lm_logits_gpu.py on the row that crosses key 256),
(3) padding is never read, (4) full-width vectors are the rectangular call and enroll_lengths alone is the ragged call, (5) every launch
form - and call kinds alternating on one handle above 64 rows, (6) sampled neighbour invariance, (7) errors, (8) neighbouring session /
score calls are undisturbed.
"""
import functools

import pytest
import torch

from oracle import llm_ref as L
from tests.test_llm_gpu import SMALL, _audit, _model
from tests.test_lm_logits_gpu import H1024, HD32, _parity, _run, _same

pytestmark = pytest.mark.gpu

# (spec, weight seed, enrollment lengths or None, mixture lengths, semantic lengths, G).  se_small: L_b = 3, 11, 242, 252, 252; row 2 starts
# its semantic phase at position 248 and crosses key 256 (a split boundary of att_split = 256 and a 16-key tile edge) at its step 8, while
# rows 0, 1 and 3 have retired (after 0, 1 and 5 steps)
TSE = ([1, 7, 33], [9, 3, 9], [12, 12, 4])
CASES = {
    "se_small": (SMALL, 22, None, [1, 9, 240, 250, 250], [0, 1, 12, 5, 12], 5),
    "tse_small": (SMALL, 22, *TSE, 5),
    "hd32": (HD32, 26, *TSE, 5),
    "h1024": (H1024, 28, *TSE, 5),
    "unise": (L.SPEC_UNISE, 33, None, [5, 40], [20, 7], 5),
    # 70 rows are two chains of 35: the first one's longest row takes 6 steps, the second one's 3
    "chains": (SMALL, 46, None, [1 + (5 * b) % 11 for b in range(70)], [b % 7 if b < 35 else b % 4 for b in range(70)], 3),
}


def _task(ne):
    return "se" if ne is None else "tse"


def _inputs(spec, ne, nm, seed):
    """enroll_feats [B, max(ne), F] or None, and mix_feats [B, max(nm), F]: the frames behind a row's length keep their random values."""
    enr = None if ne is None else L.synth_feats(seed + 1, len(nm), max(ne), spec.feats_dim)
    return enr, L.synth_feats(seed, len(nm), max(nm), spec.feats_dim)


def _rows(lm, spec, dev, enr, mix, ne, nm, ns, G, **kw):
    return _run(lm, spec, dev, _task(ne), enr, mix, max(ns), G, enroll_lengths=ne, mix_lengths=nm, semantic_lengths=ns, **kw)


def _solo(lm, spec, dev, enr, mix, ne, nm, ns, b, G, **kw):
    """Sequence b alone through the EXISTING rectangular call, on its own frames and with its own number of semantic steps."""
    e = None if ne is None else enr[b:b + 1, :ne[b]].contiguous()
    # a row without semantic steps runs alone with one (the Python call returns no empty tensor): its global phase cannot see it, and
    # _row_mismatch compares the row's own ns[b] = 0 columns only
    return _run(lm, spec, dev, _task(ne), e, mix[b:b + 1, :nm[b]].contiguous(), max(ns[b], 1), G, **kw)


def _row_mismatch(got, alone, b, n):
    """Which of (global ids, semantic ids, logits.global, logits.semantic) of row b differ from the sequence alone over the row's own n
    columns, or break the fill behind them."""
    bad = []
    g, s, lg, ls = (t[b:b + 1] for t in got)
    if not torch.equal(g, alone[0]): bad.append("global ids")
    if not torch.equal(s[:, :n], alone[1][:, :n]): bad.append("semantic ids")
    if not torch.equal(lg, alone[2]): bad.append("logits.global")
    if not torch.equal(ls[:, :n], alone[3][:, :n]): bad.append("logits.semantic")
    if not bool((s[:, n:] == -1).all()): bad.append("ids behind the length are not -1")
    if not bool((ls[:, n:] == 0).all()): bad.append("tap behind the length is not exactly 0")
    return bad


def _rows_equal_solo(lm, spec, dev, enr, mix, ne, nm, ns, G, got, rows, label=""):
    bad = {b: m for b in rows for m in [_row_mismatch(got, _solo(lm, spec, dev, enr, mix, ne, nm, ns, b, G), b, ns[b])] if m}
    assert not bad, f"{label}: rows that differ from the same sequence alone: {bad}"


@functools.lru_cache(maxsize=None)
def _case(name, dev):
    """One call with per-row lengths, computed once and shared by the tests below (never modified)."""
    spec, seed, ne, nm, ns, G = CASES[name]
    sd, lm = _model(spec, seed, dev)
    enr, mix = _inputs(spec, ne, nm, seed + 100)
    return sd, lm, enr, mix, _rows(lm, spec, dev, enr, mix, ne, nm, ns, G)


@pytest.mark.parametrize("name", list(CASES))
def test_each_row_equals_itself_alone_bit_for_bit(qa_lib, gpu_device, name):
    spec, _, ne, nm, ns, G = CASES[name]
    _, lm, enr, mix, got = _case(name, gpu_device)
    B = len(nm)
    assert all(torch.isfinite(t).all() for t in got[2:])
    assert got[0].shape == (B, G) and got[1].shape == (B, max(ns))
    # chains: every row of both chain boundaries and the rows that carry each chain's longest length, a third of the rest
    rows = range(B) if B <= 8 else sorted({0, 6, 13, 34, 35, 38, 69} | set(range(1, B, 3)))
    _rows_equal_solo(lm, spec, gpu_device, enr, mix, ne, nm, ns, G, got, rows, name)


@pytest.mark.parametrize("name", ["se_small", "unise"])
def test_each_row_matches_the_oracle_on_its_own_frames(qa_lib, gpu_device, name):
    spec, _, ne, nm, ns, G = CASES[name]
    sd, _, enr, mix, got = _case(name, gpu_device)
    for b, n in enumerate(ns):
        free_match, near_ties = _audit(sd, spec, "se", None, mix[b:b + 1, :nm[b]], n, G, got[0][b:b + 1], got[1][b:b + 1, :n], tol=2e-4)
        print(f"{name} row {b}: free-running agreement {free_match}, near-tie flips {near_ties}")
        assert near_ties > 0 or free_match == 1.0, (name, b)


def test_decode_logits_of_the_row_that_crosses_key_256_match_the_fp64_oracle(qa_lib, gpu_device):
    spec, _, ne, nm, ns, G = CASES["se_small"]
    sd, _, enr, mix, got = _case("se_small", gpu_device)
    b = 2
    g, s, lg, ls = (t[b:b + 1] for t in got)
    _parity(sd, spec, "se", None, mix[b:b + 1, :nm[b]], ns[b], G, g, s[:, :ns[b]], lg, ls[:, :ns[b]], "rows_se_small_row2")


def _poisoned(x, lens, value):
    if x is None:
        return None
    out = x.clone()
    for b, n in enumerate(lens):
        out[b, n:] = value
    return out


@pytest.mark.parametrize("name", ["se_small", "tse_small"])
def test_padding_is_never_read(qa_lib, gpu_device, name):
    spec, _, ne, nm, ns, G = CASES[name]
    _, lm, enr, mix, got = _case(name, gpu_device)
    for value in (float("nan"), 1e30, 0.0):
        out = _rows(lm, spec, gpu_device, _poisoned(enr, ne, value), _poisoned(mix, nm, value), ne, nm, ns, G)
        assert all(torch.isfinite(t).all() for t in out[2:]), value
        assert _same(out, got), f"padding frames set to {value} changed the result"


def test_full_width_vectors_are_the_rectangular_call_and_enroll_alone_the_ragged_one(qa_lib, gpu_device):
    spec, S, G = SMALL, 12, 5
    _, lm = _model(spec, 22, gpu_device)
    ne = [7, 2, 7, 5, 1]
    enr, mix = _inputs(spec, ne, [9] * 5, 140)
    dev = gpu_device
    for kw in (dict(do_sample=False), dict(do_sample=True)):
        torch.manual_seed(11)
        plain = _run(lm, spec, dev, "tse", enr, mix, S, G, **kw)
        for lens in (dict(mix_lengths=[9] * 5), dict(semantic_lengths=[S] * 5),
                     dict(enroll_lengths=[7] * 5, mix_lengths=[9] * 5, semantic_lengths=[S] * 5)):
            torch.manual_seed(11)
            assert _same(_run(lm, spec, dev, "tse", enr, mix, S, G, **lens, **kw), plain), (kw, lens)
        torch.manual_seed(11)
        ragged = _run(lm, spec, dev, "tse", enr, mix, S, G, enroll_lengths=ne, **kw)
        for lens in (dict(mix_lengths=None, semantic_lengths=None), dict(mix_lengths=[9] * 5, semantic_lengths=[S] * 5)):
            torch.manual_seed(11)
            assert _same(_run(lm, spec, dev, "tse", enr, mix, S, G, enroll_lengths=ne, **lens, **kw), ragged), (kw, lens)


def _seeded(B, seed, lo, top):
    gen = torch.Generator().manual_seed(seed)
    lens = torch.randint(lo, top + 1, (B,), generator=gen).tolist()
    lens[0], lens[-1] = top, lo  # the tensors' widths are `top` whatever the draw; the last row is the shortest
    return lens


@pytest.mark.parametrize("B,rows", [(12, (0, 7, 8, 11)), (33, (0, 16, 17, 32)), (65, (0, 32, 33, 64))])
def test_every_launch_form_gives_the_same_bits(qa_lib, gpu_device, knob, B, rows):
    """QA_LM_GRAPH 0 / 1, QA_LM_CHAINS 1 / 2, QA_LM_ROWSPLIT 0 .. 3 and QA_LM_PF 0 / 15 on seeded lengths, the batches of
    tests/test_lm_ragged_gpu.py: 12 rows take the 8-row split, 33 two row tiles (two chains of 17 + 16 under QA_LM_CHAINS=2), 65 always two
    chains of 33 + 32 replaying captured steps.  The per-row ints of a chain are its slice at b0."""
    spec, G = SMALL, 4
    _, lm = _model(spec, 46, gpu_device)
    ne, nm, ns = _seeded(B, 50 + B, 1, 40), _seeded(B, 51 + B, 1, 6), _seeded(B, 52 + B, 0, 8)
    enr, mix = _inputs(spec, ne, nm, 60 + B)
    dev = gpu_device
    ref = _rows(lm, spec, dev, enr, mix, ne, nm, ns, G)
    _rows_equal_solo(lm, spec, dev, enr, mix, ne, nm, ns, G, ref, rows, f"B={B}")
    for graph in (0, 1):
        knob("QA_LM_GRAPH", graph)
        for chains in (1, 2):
            knob("QA_LM_CHAINS", chains)
            assert _same(_rows(lm, spec, dev, enr, mix, ne, nm, ns, G), ref), (graph, chains)
        knob("QA_LM_CHAINS", 0)
        for rs in (0, 1, 2, 3):
            knob("QA_LM_ROWSPLIT", rs)
            assert _same(_rows(lm, spec, dev, enr, mix, ne, nm, ns, G), ref), (graph, rs)
        knob("QA_LM_ROWSPLIT", 0)
        for pf in (0, 15):
            knob("QA_LM_PF", pf)
            assert _same(_rows(lm, spec, dev, enr, mix, ne, nm, ns, G), ref), (graph, pf)


def test_a_captured_step_serves_every_length_vector(qa_lib, gpu_device, knob):
    """Two sets of vectors of equal widths back to back under QA_LM_GRAPH=1: the step graph is keyed by "stop or not", never by the
    values, so the second call replays the first one's graph - and is still each row alone."""
    spec, G = SMALL, 4
    _, lm = _model(spec, 46, gpu_device)
    first = ([40, 3, 17, 40, 1, 22], [6, 1, 4, 2, 6, 3], [8, 0, 3, 8, 1, 5])
    second = ([2, 40, 40, 9, 31, 5], [1, 6, 2, 6, 5, 3], [0, 8, 8, 2, 7, 1])
    enr, mix = _inputs(spec, first[0], first[1], 70)
    dev = gpu_device
    knob("QA_LM_GRAPH", 1)
    a = _rows(lm, spec, dev, enr, mix, *first, G)
    b = _rows(lm, spec, dev, enr, mix, *second, G)
    assert _same(_rows(lm, spec, dev, enr, mix, *first, G), a)
    knob("QA_LM_GRAPH", 0)
    _rows_equal_solo(lm, spec, dev, enr, mix, *second, G, b, range(6), "second vectors")
    _rows_equal_solo(lm, spec, dev, enr, mix, *first, G, a, range(6), "first vectors")


def test_call_kinds_alternate_on_one_handle_above_64_rows(qa_lib, gpu_device):
    """70 rows are two chains that always replay captured steps, and the ints a call kind puts behind chain 0 (none, B, 4 B) move the
    buffers of chain 1.  At equal shapes on ONE handle: the rectangular call between two semantic_lengths-only calls, the
    enroll_lengths-only call between two enroll + mix_lengths calls, and the rectangular call last - every result equal to the same call
    on a handle that has made no other, and rows of both chains equal to themselves alone.  A step captured at one layout must never be
    replayed at another."""
    spec, B, S, G, dev = SMALL, 70, 5, 3, gpu_device
    ne, nm, ns = _seeded(B, 81, 1, 5), _seeded(B, 82, 1, 4), _seeded(B, 83, 0, S)
    enr, mix = _inputs(spec, ne, nm, 84)
    kinds = {
        "rect": {},
        "sem": dict(semantic_lengths=ns),
        "enr": dict(enroll_lengths=ne),
        "enr_mix": dict(enroll_lengths=ne, mix_lengths=nm),
    }

    def call(lm, kind):
        return _run(lm, spec, dev, "tse", enr, mix, S, G, **kinds[kind])

    fresh = {k: call(_model(spec, 46, dev)[1], k) for k in kinds}
    _, lm = _model(spec, 46, dev)
    for kind in ("sem", "rect", "sem", "enr", "enr_mix", "enr", "enr_mix", "rect", "enr", "sem"):
        assert _same(call(lm, kind), fresh[kind]), f"{kind}: differs from the same call on a fresh handle"
    full = [5] * B, [4] * B, [S] * B
    rows = (0, 34, 35, 52, 69)
    _rows_equal_solo(lm, spec, dev, enr, mix, full[0], full[1], ns, G, fresh["sem"], rows, "semantic_lengths only")
    _rows_equal_solo(lm, spec, dev, enr, mix, ne, nm, full[2], G, fresh["enr_mix"], rows, "enroll + mix_lengths")
    _rows_equal_solo(lm, spec, dev, enr, mix, ne, full[1], full[2], G, fresh["enr"], rows, "enroll_lengths only")


def test_a_sampled_row_does_not_depend_on_its_neighbours(qa_lib, gpu_device):
    """The sampler's Philox stream is keyed by (seed, GLOBAL sequence index, step): row b's stream over its own columns is the same
    whatever the OTHER rows' lengths and padding are, repeats under a fixed seed, and row 0 equals its solo sampled run."""
    spec, _, ne, nm, ns, G = CASES["tse_small"]
    _, lm, enr, mix, _ = _case("tse_small", gpu_device)
    dev = gpu_device

    def sampled(e, m, ne_, nm_, ns_):
        torch.manual_seed(7)
        return _rows(lm, spec, dev, e, m, ne_, nm_, ns_, G, do_sample=True)

    one = sampled(enr, mix, ne, nm, ns)
    assert _same(sampled(enr, mix, ne, nm, ns), one), "a fixed seed does not repeat"
    torch.manual_seed(7)
    alone = _solo(lm, spec, dev, enr, mix, ne, nm, ns, 0, G, do_sample=True)
    assert not _row_mismatch(one, alone, 0, ns[0]), "row 0 differs from its solo sampled run with the same seed"
    assert int(one[0].min()) >= 0 and int(one[0].max()) < spec.global_size and int(one[1].max()) < spec.semantic_size
    for b in range(3):  # every other row shorter in all three lengths (the tensors keep their widths), padding poisoned
        ne2 = [n if i == b else max(1, n // 2) for i, n in enumerate(ne)]
        nm2 = [n if i == b else max(1, n // 2) for i, n in enumerate(nm)]
        ns2 = [n if i == b else n // 3 for i, n in enumerate(ns)]
        two = sampled(_poisoned(enr, ne2, float("nan")), _poisoned(mix, nm2, float("nan")), ne2, nm2, ns2)
        n = ns[b]
        assert torch.equal(two[0][b], one[0][b]) and torch.equal(two[1][b, :n], one[1][b, :n]), f"row {b}: tokens moved with its neighbours"
        assert torch.equal(two[2][b], one[2][b]) and torch.equal(two[3][b, :n], one[3][b, :n]), f"row {b}: logits moved with its neighbours"
        assert bool((two[1][b, n:] == -1).all())


def test_errors_name_their_cause_and_leave_the_handle_usable(qa_lib, gpu_device):
    import unified_audio_amd as qa

    spec, S, G = SMALL, 6, 3
    _, lm = _model(spec, 21, gpu_device)
    ne, nm, ns = [5, 2, 5], [4, 4, 1], [6, 0, 3]
    enr, mix = _inputs(spec, ne, nm, 80)
    mel = torch.zeros(3, S, 80)
    dev = gpu_device

    def good():
        g, s = lm.generate("tse", mel, enr.to(dev), mel, mix.to(dev), global_length=G, do_sample=False, enroll_lengths=ne, mix_lengths=nm,
                           semantic_lengths=ns)
        return g.cpu(), s.cpu()

    usual = good()
    long_mix = torch.zeros(3, 4096, spec.feats_dim)
    for kw, enroll, mixture, match in (
            (dict(mix_lengths=[4, 0, 4]), enr, mix, r"n_mix\[1\] = 0 .*1 \.\. n_mix_max = 4"),
            (dict(mix_lengths=[4, 4, 5]), enr, mix, r"n_mix\[2\] = 5 .*n_mix_max = 4"),
            (dict(semantic_lengths=[-1, 6, 6]), enr, mix, r"n_semantic\[0\] = -1 .*0 \.\. semantic_length_max = 6"),
            (dict(semantic_lengths=[6, 7, 6]), enr, mix, r"n_semantic\[1\] = 7 .*semantic_length_max = 6"),
            (dict(enroll_lengths=[5, 6, 5], mix_lengths=nm), enr, mix, r"n_enroll\[1\] = 6 .*n_enroll_max = 5"),
            (dict(mix_lengths=[4, 4]), enr, mix, r"2 entries for a batch of 3"),
            (dict(enroll_lengths=[5, 5, 5], mix_lengths=nm), None, mix, r"n_enroll\[0\] = 5\) without an enrollment"),
            (dict(mix_lengths=[4090, 1, 1]), None, long_mix, r"exceed max_position_embeddings 4096"),
    ):
        for do_sample in (False, True):
            with pytest.raises(qa.QuarkAudioError, match=match):
                lm.generate("tse" if enroll is not None else "se", None if enroll is None else mel, None if enroll is None else enroll.to(dev),
                            mel, mixture.to(dev), global_length=G, do_sample=do_sample, **kw)
            assert _same(good(), usual), (kw, do_sample)
    # under a caller's stream capture the lengths (host data) are refused, and the capture itself stays intact
    from unified_audio_amd import _lib

    m, e = mix.to(dev), enr.to(dev)
    gi, si = torch.full((3, G), -7, dtype=torch.int64, device=dev), torch.full((3, S), -7, dtype=torch.int64, device=dev)
    lens = (_lib.C.c_int64 * 3)(*nm)
    lm.enable_taps(False)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(qa.QuarkAudioError, match="qa_lm_generate_rows: refused under a stream capture"):
        with torch.cuda.graph(graph, stream=side):
            _lib.check(qa_lib.qa_lm_generate_rows(lm._handle, 1, e.data_ptr(), 5, None, m.data_ptr(), 4, lens, 3, G, S, None, 0.8, 50, 0.95,
                                                  gi.data_ptr(), si.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize()
    assert bool((gi == -7).all()) and bool((si == -7).all())
    assert _same(good(), usual)
    # a NULL pointer where data is needed: the mixture, either output
    st = torch.cuda.current_stream(dev).cuda_stream
    sem = (_lib.C.c_int64 * 3)(*ns)
    for mix_p, g_p, s_p in ((None, gi.data_ptr(), si.data_ptr()), (m.data_ptr(), None, si.data_ptr()), (m.data_ptr(), gi.data_ptr(), None)):
        for fn, seed in ((qa_lib.qa_lm_generate_rows, ()), (qa_lib.qa_lm_generate_rows_sampled, (7,))):
            with pytest.raises(qa.QuarkAudioError, match="qa_lm_generate_rows: null argument"):
                _lib.check(fn(lm._handle, 1, e.data_ptr(), 5, None, mix_p, 4, lens, 3, G, S, sem, 0.8, 50, 0.95, *seed, g_p, s_p, st))
        torch.cuda.synchronize()
        assert bool((gi == -7).all()) and bool((si == -7).all())
        assert _same(good(), usual)
    _rows_equal_solo(lm, spec, dev, enr, mix, ne, nm, ns, G, _rows(lm, spec, dev, enr, mix, ne, nm, ns, G), range(3), "after the refusals")


def test_neighbouring_session_and_score_calls_are_undisturbed(qa_lib, gpu_device):
    """The pattern of tests/test_lm_ragged_gpu.py: a call with per-row lengths between two session calls, and between two score calls,
    changes neither side - and is itself what it was."""
    import unified_audio_amd as qa
    from tests.test_lm_session_gpu import _embeds, _feed

    spec, dev = SMALL, gpu_device
    sd, lm = _model(spec, 21, dev)
    ne, nm, ns, S, G = [3, 11, 6, 11], [9, 2, 9, 5], [8, 3, 0, 8], 8, 4
    enr, mix = _inputs(spec, ne, nm, 90)
    mel = torch.zeros(4, S, 80)

    def rows():
        g, s = lm.generate("tse", mel, enr.to(dev), mel, mix.to(dev), global_length=G, do_sample=False, enroll_lengths=ne, mix_lengths=nm,
                           semantic_lengths=ns)
        return g.cpu(), s.cpu()

    r0 = rows()
    x = _embeds(sd, spec, 6, 5, 12)
    schedule = [7, 1, 3, 1]
    cache = qa.KVCache(lm, 5, 16)
    first = _feed(lm, dev, cache, x, schedule)
    cache.reset()
    a = _feed(lm, dev, cache, x, schedule[:2])
    r1 = rows()
    b = _feed(lm, dev, cache, x[:, 8:], schedule[2:])
    assert torch.equal(torch.cat([a, b], dim=1), first)
    assert _same(r0, r1)
    ids = r0[1].clamp(min=0)  # score reads the ids inside a row's length alone; the -1 fill behind it only has to be a legal id
    score = lambda: [t.cpu() for t in lm.score("tse", mel, enr.to(dev), mel, mix.to(dev), r0[0], ids)]
    s0 = score()
    r2 = rows()
    s1 = score()
    assert _same(s0, s1) and _same(r0, r2)
