"""CustomLlamaModel.llm_forward over a library-owned KV cache (qa_lm_forward / qa_lm_cache_*), and LLM_SFT's submodules as device calls.

(1) fp64 parity per call, the protocol of tests/test_lm_logits_gpu.py: for a row, e = max |h - h64| / rms(h64); the HIP rows of every call
    of a chunk schedule must be within C_PARITY * max(e_cpu32, E_FLOOR) of oracle.llm_ref.llm_forward in float64 (e_cpu32: the same
    oracle in float32).
(2) output_hidden_states, (3) bit-exact invariances, (4) the cache select, (5) the reference's token goldens rebuilt from the
    primitives, (6) errors that name their cause and leave the cache usable.
"""
import os

import numpy as np
import pytest
import torch

from oracle import llm_ref as L
from tests.test_llm_gpu import SMALL, _audit, _model
from tests.test_lm_logits_gpu import C_PARITY, E_FLOOR, H512, H1024, HD32, _first_argmax

pytestmark = pytest.mark.gpu


def _embeds(sd, spec, seed, B, n):
    """[B, n, hidden] rows of codec_embedding (what a decode loop feeds), fp32 on the host."""
    gen = torch.Generator().manual_seed(seed)
    return sd["codec_embedding.weight"][torch.randint(0, spec.vocab, (B, n), generator=gen)].clone()


def _row_err(h, truth):
    truth = truth.double()
    rms = truth.pow(2).mean(-1).sqrt()
    return float(((h.double() - truth).abs().amax(-1) / rms).max())


class _Oracle:
    """oracle.llm_ref.llm_forward over its own KVCache, in float64 (the truth) and float32 (the yardstick), call by call."""

    def __init__(self, sd, spec):
        self.spec = spec
        self.sd = {torch.float32: sd, torch.float64: {k: v.double() for k, v in sd.items()}}
        self.cache = {t: L.KVCache(spec.n_layers) for t in self.sd}

    def __call__(self, x, hidden=False):
        """-> (h64, h32) or, with hidden, the n_layers + 1 hidden states of each: the input of every layer is what llm_forward hands
        to the layer's input RMSNorm (every second _rms call), the last entry the returned final norm."""
        out = []
        for t in (torch.float64, torch.float32):
            seen = []
            rms = L._rms

            def spy(xx, w, eps, dtype=torch.float32):
                seen.append(xx)
                return rms(xx, w, eps, dtype)

            L._rms = spy
            try:
                h = L.llm_forward(self.sd[t], x.to(t), self.cache[t], self.spec, t)
            finally:
                L._rms = rms
            out.append([seen[2 * i] for i in range(self.spec.n_layers)] + [h] if hidden else h)
        return out


def _bound(e_cpu):
    return C_PARITY * max(e_cpu, E_FLOOR)


def _run_schedule(lm, sd, spec, dev, B, schedule, seed, label):
    import unified_audio_amd as qa

    x = _embeds(sd, spec, seed, B, sum(schedule))
    cache = qa.KVCache(lm, B, sum(schedule))
    oracle = _Oracle(sd, spec)
    pos, worst = 0, (0.0, 0.0)
    for n in schedule:
        chunk = x[:, pos:pos + n]
        out = lm.llm_forward(chunk.to(dev), past_key_values=cache, use_cache=True)
        assert out.past_key_values is cache and cache.get_seq_length() == pos + n
        h = out.last_hidden_state.cpu()
        assert h.shape == (B, n, spec.hidden) and torch.isfinite(h).all()
        h64, h32 = oracle(chunk)
        e_hip, e_cpu = _row_err(h, h64), _row_err(h32, h64)
        print(f"session parity {label} pos {pos} n {n}: e_hip {e_hip:.3e} e_cpu32 {e_cpu:.3e} bound {_bound(e_cpu):.3e}")
        assert e_hip <= _bound(e_cpu), f"{label} pos {pos} n {n}: HIP {e_hip:.3e} from the fp64 truth, bound {_bound(e_cpu):.3e}"
        if e_hip > worst[0]:
            worst = (e_hip, e_cpu)
        pos += n
    print(f"session parity {label}: worst e_hip / e_cpu32 {worst[0]:.3e} / {worst[1]:.3e}")


# (spec, weight seed, B, chunk schedule, knobs)
SCHEDULES = {
    # empty cache, the n = 1 fused step, n > 1 over a non-empty past, chunks that start and end inside a 16-key tile, keys 16 / 32 / 64
    "small_b3": (SMALL, 21, 3, [7, 1, 1, 5, 1, 40, 1, 16, 1], {}),
    "hd32_b3": (HD32, 26, 3, [9, 1, 6, 1, 1], {}),
    "h1024_b3": (H1024, 28, 3, [9, 1, 6, 1, 1], {}),                     # hd 128, no fused MLP at this width
    "unise_b2": (L.SPEC_UNISE, 33, 2, [9, 1, 6, 1, 1], {}),
    "h512_unfused_b3": (H512, 27, 3, [9, 1, 6, 1, 1], {"QA_LM_MLP_FUSED": 0}),
    "small_b65": (SMALL, 25, 65, [3, 1, 1], {}),                         # n = 1 above one group of 64 rows, and n = 3
}


@pytest.mark.parametrize("case", list(SCHEDULES))
def test_every_call_of_a_schedule_matches_the_fp64_oracle(qa_lib, gpu_device, knob, case):
    """Measured on MI355X, the call of the schedule with the largest e_hip, e_hip / e_cpu32: small_b3 2.68e-6 / 1.83e-6, hd32_b3
    2.77e-6 / 1.68e-6, h1024_b3 5.70e-6 / 2.07e-6, unise_b2 6.80e-6 / 3.40e-6, h512_unfused_b3 4.01e-6 / 1.83e-6, small_b65
    3.24e-6 / 1.92e-6.  The largest are n >= 2 chunks (the implicit GEMM's fp32 chain); the n = 1 steps sit at or below the fp32
    oracle's own error (e.g. small_b65 1.47e-6 / 1.58e-6), as the decode step does in tests/test_lm_logits_gpu.py.  Hidden states
    (test below): 2.64e-6 / 1.36e-6 at n = 5, 1.24e-6 / 1.30e-6 at n = 1; prefix reuse: 2.29e-6 / 1.34e-6."""
    spec, seed, B, schedule, knobs = SCHEDULES[case]
    for k, v in knobs.items():
        knob(k, v)
    sd, lm = _model(spec, seed, gpu_device)  # after the knobs: QA_LM_MLP_FUSED is read at create
    _run_schedule(lm, sd, spec, gpu_device, B, schedule, seed + 200, case)


def test_output_hidden_states_of_a_chunk_and_of_a_step(qa_lib, gpu_device):
    import unified_audio_amd as qa

    spec, B = SMALL, 3
    sd, lm = _model(spec, 21, gpu_device)
    x = _embeds(sd, spec, 5, B, 6)
    cache = qa.KVCache(lm, B, 16)
    oracle = _Oracle(sd, spec)
    for lo, n in ((0, 5), (5, 1)):  # the n = 5 chunk, then the n = 1 step over it
        chunk = x[:, lo:lo + n]
        out = lm.llm_forward(chunk.to(gpu_device), past_key_values=cache, use_cache=True, output_hidden_states=True)
        hs = [h.cpu() for h in out.hidden_states]
        assert len(hs) == spec.n_layers + 1 and all(h.shape == (B, n, spec.hidden) for h in hs)
        assert torch.equal(hs[0], chunk), "entry 0 is the input"
        assert torch.equal(hs[-1], out.last_hidden_state.cpu()), "the last entry is last_hidden_state"
        hs64, hs32 = oracle(chunk, hidden=True)
        for i, (h, h64, h32) in enumerate(zip(hs, hs64, hs32)):
            e_hip, e_cpu = _row_err(h, h64), _row_err(h32, h64)
            print(f"hidden state {i} n {n}: e_hip {e_hip:.3e} e_cpu32 {e_cpu:.3e}")
            assert e_hip <= _bound(e_cpu), (i, n, e_hip, e_cpu)
        plain = lm.llm_forward(chunk.to(gpu_device), use_cache=False)  # the defaults return neither hidden states nor a cache
        assert plain.hidden_states is None and plain.past_key_values is None
    # the capture changes no bit of the result
    c1, c2 = qa.KVCache(lm, B, 16), qa.KVCache(lm, B, 16)
    for lo, n in ((0, 5), (5, 1)):
        a = lm.llm_forward(x[:, lo:lo + n].to(gpu_device), past_key_values=c1, use_cache=True, output_hidden_states=True)
        b = lm.llm_forward(x[:, lo:lo + n].to(gpu_device), past_key_values=c2, use_cache=True)
        assert torch.equal(a.last_hidden_state, b.last_hidden_state)


def _feed(lm, dev, cache, x, schedule):
    outs, pos = [], 0
    for n in schedule:
        outs.append(lm.llm_forward(x[:, pos:pos + n].to(dev), past_key_values=cache, use_cache=cache is not None).last_hidden_state)
        pos += n
    return torch.cat(outs, dim=1)


def test_invariances_are_bit_exact(qa_lib, gpu_device):
    import unified_audio_amd as qa

    spec, dev = SMALL, gpu_device
    sd, lm = _model(spec, 21, dev)
    x = _embeds(sd, spec, 6, 5, 12)
    # cache = None equals a fresh cache (a chunk and a single position)
    for n in (7, 1):
        fresh = lm.llm_forward(x[:, :n].to(dev), past_key_values=qa.KVCache(lm, 5, 16), use_cache=True).last_hidden_state
        assert torch.equal(lm.llm_forward(x[:, :n].to(dev)).last_hidden_state, fresh), n
    # a row of a B = 5 call equals the same sequence run alone (n >= 2 chunks; the n = 1 steps too)
    schedule = [7, 1, 3, 1]
    full = _feed(lm, dev, qa.KVCache(lm, 5, 16), x, schedule)
    for b in (0, 3, 4):
        alone = _feed(lm, dev, qa.KVCache(lm, 1, 16), x[b:b + 1], schedule)
        assert torch.equal(alone[0], full[b]), b
    # test_generate equals one position at a time through llm_forward
    step = _feed(lm, dev, qa.KVCache(lm, 5, 16), x, [1] * 12)
    assert torch.equal(lm.test_generate(x.to(dev)), step)
    # crop(k), then the positions k .. again: the first run's outputs
    cache = qa.KVCache(lm, 5, 16)
    first = _feed(lm, dev, cache, x, schedule)
    cache.crop(7)
    assert cache.get_seq_length() == 7
    assert torch.equal(_feed(lm, dev, cache, x[:, 7:], schedule[1:]), first[:, 7:])
    # reset(), then everything again
    cache.reset()
    assert cache.get_seq_length() == 0
    assert torch.equal(_feed(lm, dev, cache, x, schedule), first)
    # a generate call between two session calls changes neither side
    mix = L.synth_feats(3, 4, 9, spec.feats_dim).to(dev)
    mel = torch.zeros(4, 8, 80)
    g0 = lm.generate("se", None, None, mel, mix, global_length=4, do_sample=False)
    cache.reset()
    a = _feed(lm, dev, cache, x, schedule[:2])
    g1 = lm.generate("se", None, None, mel, mix, global_length=4, do_sample=False)
    b = _feed(lm, dev, cache, x[:, 8:], schedule[2:])
    assert torch.equal(torch.cat([a, b], dim=1), first)
    assert torch.equal(g0[0], g1[0]) and torch.equal(g0[1], g1[1])


@pytest.mark.parametrize("B", [3, 65])
def test_a_cacheless_step_equals_the_step_over_a_fresh_cache(qa_lib, gpu_device, B):
    """The n = 1 step with its buffers and keys in the call's workspace (use_cache=False, capacity 16) against the same step over a
    fresh KVCache of 16 positions, which brings its own: every hidden state bit for bit.  65 rows: the smallest batch that crosses
    one group of 64, where the layer stride of the workspace's keys must be the whole call's and not the group's."""
    import unified_audio_amd as qa

    spec, dev = SMALL, gpu_device
    sd, lm = _model(spec, 21, dev)
    x = _embeds(sd, spec, 7, B, 1).to(dev)
    plain = lm.llm_forward(x, use_cache=False, output_hidden_states=True)
    cached = lm.llm_forward(x, past_key_values=qa.KVCache(lm, B, 16), use_cache=True, output_hidden_states=True)
    assert torch.equal(plain.last_hidden_state, cached.last_hidden_state)
    assert len(plain.hidden_states) == len(cached.hidden_states) == spec.n_layers + 1
    for i, (a, b) in enumerate(zip(plain.hidden_states, cached.hidden_states)):
        assert torch.equal(a, b), i


@pytest.mark.parametrize("idx", [[3, 1, 0, 2], [1, 1, 1, 1], [2, 0], [0, 0, 1, 1, 2, 2, 3, 3]])
def test_cache_select_equals_running_the_selected_sequences(qa_lib, gpu_device, idx):
    import unified_audio_amd as qa

    spec, dev = SMALL, gpu_device
    sd, lm = _model(spec, 21, dev)
    x = _embeds(sd, spec, 7, 4, 10)
    more = _embeds(sd, spec, 8, len(idx), 4)
    cache = qa.KVCache(lm, 8, 16)
    _feed(lm, dev, cache, x, [10])
    cache.batch_select_indices(idx)
    assert cache.batch_size == len(idx) and cache.get_seq_length() == 10
    got = _feed(lm, dev, cache, more, [1, 3])
    direct = qa.KVCache(lm, 8, 16)
    _feed(lm, dev, direct, x[idx], [10])
    assert torch.equal(got, _feed(lm, dev, direct, more, [1, 3]))


def test_a_prefix_run_once_serves_every_segment(qa_lib, gpu_device):
    """The SE prompt at B = 1, selected to B = 4 (batch_repeat_interleave), then four different continuations: each within the
    parity bound of the oracle run on the repeated prompt."""
    import unified_audio_amd as qa

    spec, dev = SMALL, gpu_device
    sd, lm = _model(spec, 21, dev)
    mix = L.synth_feats(9, 1, 9, spec.feats_dim)
    prompt = lm.build_prompt("se", None, mix.to(dev))
    want = L.build_prompt(sd, L.TASK_MAP["se"], None, mix)
    assert prompt.shape == want.shape and float((prompt.cpu() - want).abs().max()) <= 1e-5 * float(want.abs().max())
    cache = qa.KVCache(lm, 4, 32)
    lm.llm_forward(prompt, past_key_values=cache, use_cache=True)
    cache.batch_repeat_interleave(4)
    assert cache.batch_size == 4
    cont = _embeds(sd, spec, 10, 4, 6)
    oracle = _Oracle(sd, spec)
    oracle(prompt.cpu().repeat(4, 1, 1))
    pos = 0
    for n in (1, 4, 1):
        h = lm.llm_forward(cont[:, pos:pos + n].to(dev), past_key_values=cache, use_cache=True).last_hidden_state.cpu()
        h64, h32 = oracle(cont[:, pos:pos + n])
        e_hip, e_cpu = _row_err(h, h64), _row_err(h32, h64)
        print(f"prefix reuse n {n}: e_hip {e_hip:.3e} e_cpu32 {e_cpu:.3e}")
        assert e_hip <= _bound(e_cpu), (n, e_hip, e_cpu)
        pos += n


def _greedy_from_primitives(lm, spec, dev, task, enr, mix, S, G):
    """LLM_SFT.generate (llm_sft.py:93-195, do_sample=False) written with build_prompt / llm_forward / codec_embedding / output_head."""
    import unified_audio_amd as qa

    B = mix.shape[0]
    prompt = lm.build_prompt(task, None if enr is None else enr.to(dev), mix.to(dev))
    cache = qa.KVCache(lm, B, prompt.shape[1] + G + 1 + S)
    lm.llm_forward(prompt, past_key_values=cache, use_cache=True)
    streams = []
    for first_id, steps, lo, width in ((0, G + 1, spec.global_offset, spec.global_size), (1, S, spec.semantic_offset, spec.semantic_size)):
        ids, toks = torch.full((B,), first_id, dtype=torch.int64), []
        for _ in range(steps):
            h = lm.llm_forward(lm.codec_embedding(ids)[:, None], past_key_values=cache, use_cache=True).last_hidden_state[:, 0]
            ids = _first_argmax(lm.output_head(h, lo, width).cpu()) + lo
            toks.append(ids)
        streams.append(torch.stack(toks, dim=1) - lo)
    return streams[0][:, :G], streams[1]


@pytest.mark.parametrize("name", ["lm_small_se", "lm_small_tse", "lm_unise_se"])
def test_greedy_loop_from_the_primitives_matches_reference_goldens(qa_lib, gpu_device, name):
    """golden_stream_parity's rule: identical to the reference's own stream up to the first step whose stored top-2 gap is <= 2e-4,
    audited teacher-forced (_audit) after such a step."""
    from oracle import gen_golden_lm as GG

    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".npz"))
    spec, sd, task, mix, enr, S, G = GG.case_tensors(name)
    _, lm = _model(spec, GG.CASES[name][1], gpu_device)
    gids, sids = _greedy_from_primitives(lm, spec, gpu_device, task, enr, mix, S, G)
    got = torch.cat([gids, sids], dim=1).numpy()
    want = np.concatenate([g["global_ids"], g["semantic_ids"]], axis=1).astype(np.int64)
    gaps = np.delete(g["gaps"], G, axis=1)
    for b in range(got.shape[0]):
        diff = np.nonzero(got[b] != want[b])[0]
        if diff.size:
            assert gaps[b, diff[0]] <= 2e-4, f"sequence {b} leaves the reference stream at step {diff[0]} (gap {gaps[b, diff[0]]:.2e})"
    _audit(sd, spec, task, enr, mix, S, G, gids, sids)


def test_errors_name_their_cause_and_leave_the_cache_usable(qa_lib, gpu_device):
    import unified_audio_amd as qa

    spec, dev = SMALL, gpu_device
    sd, lm = _model(spec, 21, dev)
    x = _embeds(sd, spec, 11, 3, 12).to(dev)
    cache = qa.KVCache(lm, 3, 8)
    ref = qa.KVCache(lm, 3, 8)
    want = _feed(lm, dev, ref, x, [4, 1])

    def good():  # the cache still holds exactly its 4 positions: one more step gives what the undisturbed cache gave
        assert cache.get_seq_length() == 4 and cache.batch_size == 3
        h = lm.llm_forward(x[:, 4:5], past_key_values=cache, use_cache=True).last_hidden_state
        assert torch.equal(h, want[:, 4:5])
        cache.crop(4)

    lm.llm_forward(x[:, :4], past_key_values=cache, use_cache=True)
    with pytest.raises(qa.QuarkAudioError, match="max_len 8"):
        lm.llm_forward(x[:, 4:9], past_key_values=cache, use_cache=True)
    good()
    with pytest.raises(qa.QuarkAudioError, match="holds 3 sequences"):
        lm.llm_forward(x[:2, 4:5], past_key_values=cache, use_cache=True)
    good()
    with pytest.raises(qa.QuarkAudioError, match="max_batch 3"):
        lm.llm_forward(torch.cat([x, x])[:, 4:5], past_key_values=cache, use_cache=True)
    good()
    with pytest.raises(qa.QuarkAudioError, match="hidden = 256"):
        lm.llm_forward(x[:, 4:5, :128], past_key_values=cache, use_cache=True)
    good()
    with pytest.raises(qa.QuarkAudioError, match="current length"):
        cache.crop(5)
    good()
    for idx in ([0, 3], [-1], [0, 1, 2, 0]):  # a row that does not exist, a negative one, more rows than max_batch
        with pytest.raises(qa.QuarkAudioError, match="outside the cache's 3 rows|max_batch 3"):
            cache.batch_select_indices(idx)
        good()
    for kw in (dict(attention_mask=torch.ones(3, 5)), dict(position_ids=torch.arange(1)[None]), dict(cache_position=torch.arange(1)),
               dict(output_attentions=True)):
        with pytest.raises(qa.QuarkAudioError, match="not supported"):
            lm.llm_forward(x[:, 4:5], past_key_values=cache, use_cache=True, **kw)
        good()
    with pytest.raises(IndexError):
        lm.codec_embedding(torch.tensor([0, spec.vocab]))
    # a caller's stream capture: refused with the reason (the length is host state)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(qa.QuarkAudioError, match="stream capture"):
        with torch.cuda.graph(graph, stream=side):
            lm.llm_forward(x[:, 4:5], past_key_values=cache, use_cache=True)
    torch.cuda.synchronize()
    good()
