"""Per-row lengths on a KV-cache session: llm_forward(..., chunk_lengths=) / qa_lm_forward_ragged, KVCache.get_seq_lengths / crop_rows and
the per-row behaviour of crop / batch_select_indices / reset.

The truth for row b is tests/lm_session_ragged_ref.RowOracle (the oracle over a B = 1 cache of the row's own, pinned on the CPU by
tests/test_lm_session_ragged_cpu.py); the bound is the session tests' own, C_PARITY * max(e_cpu32, E_FLOOR) with _row_err's measure.
Everything else is bit-exact: a row of a ragged batch against the same sequence ALONE in a B = 1 cache of the same max_len, fed through the
ragged call with the same n_max per call.

Shapes: the chunk attention works on 32-query wave tiles and 32-key tiles, the fused step splits keys per att_split = 256 (fixed by
max_len).  The prefill counts 5 / 31 / 32 / 33 sit below, at and past a tile; the n_max = 4 chunks carry an idle row and a row of one
position; row 3 reaches 63 keys before the steps, so its key count crosses 64 during them."""
import functools

import pytest
import torch

from oracle import llm_ref as L
from tests.lm_session_ragged_ref import RowOracle, row_err, valid_rows
from tests.test_llm_gpu import SMALL, _audit, _model
from tests.test_lm_logits_gpu import C_PARITY, E_FLOOR, H512, H1024, HD32, _first_argmax

pytestmark = pytest.mark.gpu

MAX_LEN = 96
N_CHUNKS = 10  # n_max = 4 chunks of [4, 0, 1, 3]: rows at 45 / 31 / 42 / 63 positions before the steps
# (n_max, n): the prefill, the chunks, six steps with one row idle each; the plain llm_forward step follows (n = None)
SCHEDULE = [(33, [5, 31, 32, 33])] + [(4, [4, 0, 1, 3])] * N_CHUNKS + [(1, [int(b != s % 4) for b in range(4)]) for s in range(6)] + [(1, None)]
# (spec, weight seed, knobs): the knobs of the rectangular schedule test (tests/test_lm_session_gpu.py SCHEDULES)
CASES = {
    "small": (SMALL, 21, {}),
    "h512": (H512, 27, {}),
    "h512_unfused": (H512, 27, {"QA_LM_MLP_FUSED": 0}),
}


def _embeds(sd, spec, seed, B, n):
    gen = torch.Generator().manual_seed(seed)
    return sd["codec_embedding.weight"][torch.randint(0, spec.vocab, (B, n), generator=gen)].clone()


def _bound(e_cpu):
    return C_PARITY * max(e_cpu, E_FLOOR)


def _call(lm, dev, cache, x, n, hidden=False):
    """One call -> (last_hidden, all_hidden or None) on the host; n None: the plain llm_forward."""
    kw = {} if n is None else dict(chunk_lengths=n)
    out = lm.llm_forward(x.to(dev), past_key_values=cache, use_cache=True, output_hidden_states=hidden, **kw)
    return out.last_hidden_state.cpu(), (torch.stack(out.hidden_states).cpu() if hidden else None)


def _run(lm, dev, cache, xs, schedule, rows=None, hidden=True):
    """Feed a schedule; rows: the batch rows this cache holds (None: all) - a B = 1 cache gets row b's slice of every call."""
    outs = []
    for x, (n_max, n) in zip(xs, schedule):
        if rows is not None:
            x, n = x[rows], (None if n is None else [n[b] for b in rows])
        outs.append(_call(lm, dev, cache, x, n, hidden))
    return outs


@functools.lru_cache(maxsize=None)
def _case(name, dev):
    """The ragged schedule of a case on the GPU, computed once and shared by the tests below (never modified): the model, the inputs
    (NaN behind every row's count), the outputs of every call."""
    import unified_audio_amd as qa

    spec, seed, _ = CASES[name]
    sd, lm = _model(spec, seed, dev)
    xs = []
    for i, (n_max, n) in enumerate(SCHEDULE):
        x = _embeds(sd, spec, seed + 300 + i, 4, n_max)
        for b, v in enumerate(n or []):
            x[b, v:] = float("nan")
        xs.append(x)
    cache = qa.KVCache(lm, 4, MAX_LEN)
    outs = _run(lm, dev, cache, xs, SCHEDULE)
    return sd, lm, xs, outs, cache.get_seq_lengths()


@pytest.mark.parametrize("name", list(CASES))
def test_every_call_of_a_ragged_schedule_matches_the_fp64_oracle(qa_lib, gpu_device, knob, name):
    """Measured on MI355X, the largest e_hip / bound over the 18 calls: small 0.56, h512 0.74, h512_unfused 0.74; the largest single
    figure is a chunk call (h512 call 5, n_max 4, n [4, 0, 1, 3]): e_hip 4.74e-6 / e_cpu32 1.61e-6, bound 6.43e-6.  The n = 1 steps with
    an idle row sit at or below the fp32 oracle's own error (1.1e-6 .. 1.5e-6 against 1.3e-6 .. 1.9e-6)."""
    spec, _, knobs = CASES[name]
    for k, v in knobs.items():
        knob(k, v)
    sd, lm, xs, outs, lengths = _case(name, gpu_device)
    oracle = RowOracle(sd, spec, 4)
    worst = 0.0
    for i, ((n_max, n), x, (h, _)) in enumerate(zip(SCHEDULE, xs, outs)):
        counts = n if n is not None else [n_max] * 4
        h64, h32 = oracle(torch.nan_to_num(x), counts)
        e_hip = row_err(valid_rows(h, counts), valid_rows(h64, counts))
        e_cpu = row_err(valid_rows(h32, counts), valid_rows(h64, counts))
        worst = max(worst, e_hip / _bound(e_cpu))
        print(f"ragged session parity {name} call {i} n_max {n_max} n {n}: e_hip {e_hip:.3e} e_cpu32 {e_cpu:.3e} bound {_bound(e_cpu):.3e}")
        assert e_hip <= _bound(e_cpu), f"{name} call {i} (n_max {n_max}, n {n}): HIP {e_hip:.3e} from the fp64 truth, bound {_bound(e_cpu):.3e}"
    print(f"ragged session parity {name}: worst e_hip / bound {worst:.3f}")
    assert lengths == oracle.lengths == [45 + 4 + 1, 31 + 4 + 1, 42 + 5 + 1, 63 + 5 + 1]  # rows 0 and 1 idle twice, rows 2 and 3 once


@pytest.mark.parametrize("name", ["small", "h512"])
def test_a_row_equals_itself_alone_bit_for_bit(qa_lib, gpu_device, name):
    """Row b of the ragged schedule against the same sequence in a B = 1 cache of the same max_len, same n_max per call, n = [n_b]:
    last_hidden and all_hidden, both paths (chunks and steps)."""
    import unified_audio_amd as qa

    _, lm, xs, outs, _ = _case(name, gpu_device)
    for b in range(4):
        alone = _run(lm, gpu_device, qa.KVCache(lm, 1, MAX_LEN), xs, SCHEDULE, rows=[b])
        for i, ((h, hs), (h1, hs1)) in enumerate(zip(outs, alone)):
            assert torch.equal(h[b:b + 1], h1), f"{name}: row {b}, call {i} {SCHEDULE[i]}: last_hidden differs from the row alone"
            assert torch.equal(hs[:, b:b + 1], hs1), f"{name}: row {b}, call {i} {SCHEDULE[i]}: all_hidden differs from the row alone"


def test_step_rows_equal_themselves_alone_across_row_groups_of_64(qa_lib, gpu_device):
    """B = 70: the n = 1 steps run in groups of 64 rows; rows of both groups, active and idle, after a ragged prefill."""
    import unified_audio_amd as qa

    spec, dev, B = SMALL, gpu_device, 70
    sd, lm = _model(spec, 21, dev)
    pre = [1 + (7 * b) % 9 for b in range(B)]
    schedule = [(9, pre), (1, [int(b % 5 != 0) for b in range(B)]), (1, [int(b % 3 != 1) for b in range(B)]), (1, None)]
    xs = [_embeds(sd, spec, 40 + i, B, n_max) for i, (n_max, _) in enumerate(schedule)]
    outs = _run(lm, dev, qa.KVCache(lm, B, 16), xs, schedule)
    for b in (0, 1, 5, 63, 64, 65, 69):
        alone = _run(lm, dev, qa.KVCache(lm, 1, 16), xs, schedule, rows=[b])
        for i, ((h, hs), (h1, hs1)) in enumerate(zip(outs, alone)):
            assert torch.equal(h[b:b + 1], h1) and torch.equal(hs[:, b:b + 1], hs1), (b, i)


@pytest.mark.parametrize("n", [1, 7])
def test_a_rectangular_call_is_unchanged(qa_lib, gpu_device, n):
    import unified_audio_amd as qa

    spec, dev, B = SMALL, gpu_device, 3
    sd, lm = _model(spec, 21, dev)
    x = _embeds(sd, spec, 50, B, 5 + n)
    c1, c2 = qa.KVCache(lm, B, 16), qa.KVCache(lm, B, 16)
    for cache in (c1, c2):
        lm.llm_forward(x[:, :5].to(dev), past_key_values=cache, use_cache=True)
    plain = _call(lm, dev, c1, x[:, 5:], None, hidden=True)
    ragged = _call(lm, dev, c2, x[:, 5:], [n] * B, hidden=True)
    assert torch.equal(plain[0], ragged[0]) and torch.equal(plain[1], ragged[1])
    assert c1.get_seq_lengths() == c2.get_seq_lengths() == [5 + n] * B


@pytest.mark.parametrize("name", ["small", "h512"])
def test_padding_is_never_read_and_its_outputs_are_zero(qa_lib, gpu_device, name):
    """The shared run has NaN behind every row's count; a second run has zeros there."""
    import unified_audio_amd as qa

    _, lm, xs, outs, _ = _case(name, gpu_device)
    zeros = _run(lm, gpu_device, qa.KVCache(lm, 4, MAX_LEN), [torch.nan_to_num(x) for x in xs], SCHEDULE)
    for i, ((n_max, n), (h, hs), (hz, hsz)) in enumerate(zip(SCHEDULE, outs, zeros)):
        for b, v in enumerate(n if n is not None else [n_max] * 4):
            assert bool((h[b, v:] == 0).all()) and bool((hs[:, b, v:] == 0).all()), f"call {i}: row {b} has non-zero outputs behind its count {v}"
            assert torch.equal(h[b, :v], hz[b, :v]) and torch.equal(hs[:, b, :v], hsz[:, b, :v]), f"call {i}: row {b} read its padding"
            assert torch.isfinite(h[b, :v]).all()


def test_nothing_is_written_behind_a_rows_length(qa_lib, gpu_device):
    """max_len 40: row 0 ends exactly at 40 with n = [3, 8] at n_max 8 (5 padded positions that would land in row 1's storage), then
    idles at max_len through a step.  Row 1 stays equal to itself alone."""
    import unified_audio_amd as qa

    spec, dev = SMALL, gpu_device
    sd, lm = _model(spec, 21, dev)
    schedule = [(37, [37, 20]), (8, [3, 8]), (4, [0, 4]), (1, [0, 1]), (1, [0, 1])]
    xs = [_embeds(sd, spec, 60 + i, 2, n_max) for i, (n_max, _) in enumerate(schedule)]
    cache = qa.KVCache(lm, 2, 40)
    outs = _run(lm, dev, cache, xs, schedule)
    assert cache.get_seq_lengths() == [40, 34]
    for b in (0, 1):
        alone = _run(lm, dev, qa.KVCache(lm, 1, 40), xs, schedule, rows=[b])
        for i, ((h, hs), (h1, hs1)) in enumerate(zip(outs, alone)):
            assert torch.equal(h[b:b + 1], h1) and torch.equal(hs[:, b:b + 1], hs1), (b, i)


def _continue(lm, dev, cache, rows, x):
    """Two more calls (a chunk and a step) on `cache`, whose rows are `rows` of x's batch."""
    return torch.cat([_call(lm, dev, cache, x[rows][:, :3], None)[0], _call(lm, dev, cache, x[rows][:, 3:4], None)[0]], dim=1)


def test_lengths_bookkeeping_crop_select_reset(qa_lib, gpu_device):
    import unified_audio_amd as qa

    spec, dev = SMALL, gpu_device
    sd, lm = _model(spec, 21, dev)
    x = _embeds(sd, spec, 70, 3, 9)
    more = _embeds(sd, spec, 71, 3, 4)
    n = [9, 2, 6]

    def fresh():
        cache = qa.KVCache(lm, 4, 32)
        _call(lm, dev, cache, x, n)
        return cache

    def alone(b, keep):  # row b alone, its first `keep` positions
        cache = qa.KVCache(lm, 1, 32)
        _call(lm, dev, cache, x[b:b + 1, :keep], None)
        return cache

    cache = fresh()
    assert cache.get_seq_lengths() == n and cache.get_seq_length() == 9 and cache.batch_size == 3
    # crop_rows: every row to a length of its own; continuing equals the row alone on that prefix
    cache.crop_rows([4, 2, 0])
    assert cache.get_seq_lengths() == [4, 2, 0] and cache.get_seq_length() == 4
    got = _continue(lm, dev, cache, [0, 1, 2], more)
    for b, keep in enumerate([4, 2]):
        assert torch.equal(got[b:b + 1], _continue(lm, dev, alone(b, keep), [b], more)), b
    assert torch.equal(got[2:3], _continue(lm, dev, qa.KVCache(lm, 1, 32), [2], more)), "a row cropped to 0 starts over"
    # crop(len): the per-row minimum; above the longest row it is refused
    cache = fresh()
    cache.crop(5)
    assert cache.get_seq_lengths() == [5, 2, 5] and cache.get_seq_length() == 5
    cache.crop(-1)
    assert cache.get_seq_lengths() == [4, 2, 4]
    with pytest.raises(qa.QuarkAudioError, match="current length"):
        cache.crop(5)
    got = _continue(lm, dev, cache, [0, 1, 2], more)
    for b, keep in enumerate([4, 2, 4]):
        assert torch.equal(got[b:b + 1], _continue(lm, dev, alone(b, keep), [b], more)), b
    # select carries lengths and contents
    cache = fresh()
    cache.batch_select_indices([2, 2, 0])
    assert cache.get_seq_lengths() == [6, 6, 9] and cache.batch_size == 3
    got = _continue(lm, dev, cache, [0, 1, 2], more)
    for j, src in enumerate([2, 2, 0]):
        assert torch.equal(got[j:j + 1], _continue(lm, dev, alone(src, n[src]), [j], more)), (j, src)
    # a permutation with a cycle (the spare row) and a grown batch
    cache = fresh()
    cache.batch_select_indices([1, 2, 0, 1])
    assert cache.get_seq_lengths() == [2, 6, 9, 2] and cache.batch_size == 4
    more4 = _embeds(sd, spec, 72, 4, 4)
    got = _continue(lm, dev, cache, [0, 1, 2, 3], more4)
    for j, src in enumerate([1, 2, 0, 1]):
        assert torch.equal(got[j:j + 1], _continue(lm, dev, alone(src, n[src]), [j], more4)), (j, src)
    # reset clears every length and frees the batch
    cache.reset()
    assert cache.get_seq_length() == 0 and cache.batch_size == 0 and cache.get_seq_lengths() == []
    assert torch.equal(_call(lm, dev, cache, x[:2, :3], None)[0], _call(lm, dev, qa.KVCache(lm, 2, 32), x[:2, :3], None)[0])
    assert cache.get_seq_lengths() == [3, 3]


def test_a_row_joins_a_running_batch(qa_lib, gpu_device):
    """Three rows step while a fourth is created by a select, cropped to 0 and prefilled in the same calls."""
    import unified_audio_amd as qa

    spec, dev = SMALL, gpu_device
    sd, lm = _model(spec, 21, dev)
    pre = [7, 12, 3]
    x0 = _embeds(sd, spec, 80, 3, 12)
    cache = qa.KVCache(lm, 4, 48)
    _call(lm, dev, cache, x0, pre)
    cache.batch_select_indices([0, 1, 2, 0])
    cache.crop_rows(pre + [0])
    assert cache.get_seq_lengths() == pre + [0]
    # the join: rows 0 - 2 idle while row 3 takes its 19-position prompt, then a chunk call where the old rows step inside n_max = 2,
    # then plain steps for all four
    schedule = [(19, [0, 0, 0, 19]), (2, [1, 1, 1, 2]), (1, None), (1, [1, 0, 1, 1]), (1, None)]
    xs = [_embeds(sd, spec, 81 + i, 4, n_max) for i, (n_max, _) in enumerate(schedule)]
    outs = _run(lm, dev, cache, xs, schedule, hidden=False)
    assert cache.get_seq_lengths() == [pre[0] + 4, pre[1] + 3, pre[2] + 4, 19 + 2 + 3]
    for b in range(4):
        solo = qa.KVCache(lm, 1, 48)
        if b < 3:
            _call(lm, dev, solo, x0[b:b + 1], [pre[b]])
        alone = _run(lm, dev, solo, xs, schedule, rows=[b], hidden=False)
        for i, ((h, _), (h1, _)) in enumerate(zip(outs, alone)):
            assert torch.equal(h[b:b + 1], h1), (b, i)


def test_greedy_loop_over_a_ragged_prompt_matches_generate(qa_lib, gpu_device):
    """_greedy_from_primitives of tests/test_lm_session_gpu.py over a ragged TSE prompt (enrollments 7 and 12 frames): build_prompt per
    row, left-aligned, prefilled with chunk_lengths; then the plain n = 1 loop.  Token for token generate(..., enroll_lengths=[7, 12]),
    up to _audit's near-tie rule (the prefill of generate runs over the padded prompt: another summation order)."""
    import unified_audio_amd as qa

    spec, dev = SMALL, gpu_device
    sd, lm = _model(spec, 21, dev)
    lens, Nm, S, G, B = [7, 12], 9, 12, 5, 2
    enr = L.synth_feats(91, B, max(lens), spec.feats_dim)
    mix = L.synth_feats(90, B, Nm, spec.feats_dim)
    prompts = [lm.build_prompt("tse", enr[b:b + 1, :lens[b]].contiguous().to(dev), mix[b:b + 1].to(dev)) for b in range(B)]
    plen = [int(p.shape[1]) for p in prompts]
    prompt = torch.full((B, max(plen), spec.hidden), float("nan"), device=dev)
    for b, p in enumerate(prompts):
        prompt[b, :plen[b]] = p[0]
    cache = qa.KVCache(lm, B, max(plen) + G + 1 + S)
    lm.llm_forward(prompt, past_key_values=cache, use_cache=True, chunk_lengths=plen)
    assert cache.get_seq_lengths() == plen
    streams = []
    for first_id, steps, lo, width in ((0, G + 1, spec.global_offset, spec.global_size), (1, S, spec.semantic_offset, spec.semantic_size)):
        ids, toks = torch.full((B,), first_id, dtype=torch.int64), []
        for _ in range(steps):
            h = lm.llm_forward(lm.codec_embedding(ids)[:, None], past_key_values=cache, use_cache=True).last_hidden_state[:, 0]
            ids = _first_argmax(lm.output_head(h, lo, width).cpu()) + lo
            toks.append(ids)
        streams.append(torch.stack(toks, dim=1) - lo)
    gids, sids = streams[0][:, :G], streams[1]
    mel = torch.zeros(B, S, 80)
    g_ref, s_ref = lm.generate("tse", mel, enr.to(dev), mel, mix.to(dev), global_length=G, do_sample=False, enroll_lengths=lens)
    for b in range(B):
        same = torch.equal(gids[b], g_ref[b].cpu()) and torch.equal(sids[b], s_ref[b].cpu())
        # wherever the two streams part, both must sit at an audited near-tie of the oracle on the row's own enrollment
        _audit(sd, spec, "tse", enr[b:b + 1, :lens[b]], mix[b:b + 1], S, G, gids[b:b + 1], sids[b:b + 1])
        if not same:
            _audit(sd, spec, "tse", enr[b:b + 1, :lens[b]], mix[b:b + 1], S, G, g_ref[b:b + 1].cpu(), s_ref[b:b + 1].cpu())
            print(f"row {b}: the session loop and generate part at a near-tie")


def test_errors_name_the_row_and_leave_the_cache_usable(qa_lib, gpu_device):
    import unified_audio_amd as qa

    spec, dev = SMALL, gpu_device
    sd, lm = _model(spec, 21, dev)
    x = _embeds(sd, spec, 95, 3, 8).to(dev)
    pre = [4, 2, 6]
    cache, ref = qa.KVCache(lm, 3, 8), qa.KVCache(lm, 3, 8)
    for c in (cache, ref):
        lm.llm_forward(x[:, :6], past_key_values=c, use_cache=True, chunk_lengths=pre)
    want = lm.llm_forward(x[:, 6:8], past_key_values=ref, use_cache=True, chunk_lengths=[2, 1, 2]).last_hidden_state

    def good():  # the cache still holds exactly its rows: the next valid call gives the bits the undisturbed cache gave
        assert cache.get_seq_lengths() == pre and cache.batch_size == 3
        h = lm.llm_forward(x[:, 6:8], past_key_values=cache, use_cache=True, chunk_lengths=[2, 1, 2]).last_hidden_state
        assert torch.equal(h, want)
        cache.crop_rows(pre)

    good()
    with pytest.raises(qa.QuarkAudioError, match=r"n\[1\] = 3 is outside 0 \.\. n_max = 2"):
        lm.llm_forward(x[:, 6:8], past_key_values=cache, use_cache=True, chunk_lengths=[1, 3, 1])
    good()
    with pytest.raises(qa.QuarkAudioError, match=r"n\[0\] = -1 is outside"):
        lm.llm_forward(x[:, 6:8], past_key_values=cache, use_cache=True, chunk_lengths=[-1, 1, 1])
    good()
    with pytest.raises(qa.QuarkAudioError, match=r"row 2 holds 6 positions, \+ n\[2\] = 3 exceed the cache's max_len 8"):
        lm.llm_forward(x[:, 4:8], past_key_values=cache, use_cache=True, chunk_lengths=[1, 1, 3])
    good()
    with pytest.raises(qa.QuarkAudioError, match="qa_lm_forward_ragged: a qa_lm_cache is required"):
        lm.llm_forward(x[:, 6:8], chunk_lengths=[1, 1, 1])
    good()
    with pytest.raises(qa.QuarkAudioError, match="holds 3 sequences"):
        lm.llm_forward(x[:2, 6:8], past_key_values=cache, use_cache=True, chunk_lengths=[1, 1])
    good()
    with pytest.raises(qa.QuarkAudioError, match="max_batch 3"):
        lm.llm_forward(torch.cat([x, x])[:, 6:8], past_key_values=cache, use_cache=True, chunk_lengths=[1] * 6)
    good()
    with pytest.raises(qa.QuarkAudioError, match="3 lengths|2 entries"):
        lm.llm_forward(x[:, 6:8], past_key_values=cache, use_cache=True, chunk_lengths=[1, 1])
    good()
    with pytest.raises(qa.QuarkAudioError, match=r"lens\[1\] = 3 outside \[0, 2\] \(the length of row 1\)"):
        cache.crop_rows([4, 3, 6])
    good()
    # the plain call on rows of unequal length: the longest row decides
    with pytest.raises(qa.QuarkAudioError, match="max_len 8"):
        lm.llm_forward(x[:, 5:8], past_key_values=cache, use_cache=True)
    good()
    # a call whose counts are all zero succeeds and changes nothing
    h = lm.llm_forward(x[:, 6:8], past_key_values=cache, use_cache=True, chunk_lengths=[0, 0, 0])
    assert h.last_hidden_state.shape == (3, 2, spec.hidden)
    good()
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(qa.QuarkAudioError, match="stream capture"):
        with torch.cuda.graph(graph, stream=side):
            lm.llm_forward(x[:, 6:8], past_key_values=cache, use_cache=True, chunk_lengths=[2, 1, 2])
    torch.cuda.synchronize()
    good()
