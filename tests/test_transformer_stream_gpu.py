"""unified_audio_amd.Transformer on the GPU: the offline forward, the reference's cache mode and the streaming state
against the float64 restatement of tests/transformer_stream_ref.py and the golden of the reference's own module.

Tolerance, everywhere: e = max|y - y64| / max|y64| against the float64 restatement, bound 4 max(e_cpu32, 1e-6) with e_cpu32 the float32 CPU
restatement's own error on the same inputs, computed here.  Where the unchanged offline forward on that shape measures
worse than that, the streamed bound is 2 e_offline: a stream may not be worse than twice what the codec path already delivers.  Every
figure is printed before it is asserted.  Weights are seeded and scaled so that activations are O(1)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import lstm_ref as L
from tests import transformer_stream_ref as TR

pytestmark = pytest.mark.gpu

CONFIGS = {"hd64": (128, 2), "hd96": (384, 4), "hd128": (256, 2)}  # hidden, heads
MIX = (1,) * 5 + (7, 16, 3, 33, 6)  # T = 1 carries, a 16-frame chunk, offsets 28 -> 31 -> 64 across key tiles, a 33-frame chunk on attention_kernel
# "n17": 16 | 17 frames, either side of the short-chunk switch, alternating
CHUNKINGS = {"mix": MIX, "whole": (70,), "frames": (1,) * 70, "n17": (16, 17, 16, 17, 4)}


@functools.lru_cache(maxsize=None)
def case(hidden, heads, layers, B, T, causal, left_context, seed=31):
    """Inputs, the float64 truth of the offline form and the bound 4 max(e_cpu32, 1e-6) - computed once, shared, never modified."""
    sd = TR.random_state_dict(seed, hidden, 2 * hidden, layers)
    x = torch.randn(B, T, hidden, generator=torch.Generator().manual_seed(seed + 1))
    y64 = TR.forward(sd, x.double(), layers, heads, causal, left_context)
    e32 = TR.rel_err(TR.forward(sd, x, layers, heads, causal, left_context), y64)
    return dict(sd=sd, x=x, y64=y64, e32=e32, bound=4 * max(e32, 1e-6))


def build(dev, hidden, heads, layers, causal=False, left_context=0, sd=None):
    import unified_audio_amd as qa

    m = qa.Transformer(hidden, 2 * hidden, heads, layers, causal=causal, use_sliding_window=left_context > 0, left_context=left_context, device=dev)
    return m.load_state_dict(sd)


def stream(m, x, chunks, max_frames=None):
    """x through m.streaming() chunk by chunk -> the concatenated outputs (host)."""
    out, t = [], 0
    with m.streaming(x.shape[0], max_frames=max_frames or sum(chunks)):
        for n in chunks:
            out.append(m(x[:, t:t + n]))
            t += n
        assert m.streaming_offset == t
    return torch.cat(out, 1).cpu()


def check(what, y, c, e_offline=None):
    e = TR.rel_err(y.cpu(), c["y64"])
    bound = c["bound"]
    if e_offline is not None and e_offline > bound:
        bound = 2 * e_offline
    print(f"{what}: e {e:.2e}  e_cpu32 {c['e32']:.2e}" + (f"  e_offline {e_offline:.2e}" if e_offline is not None else "") + f"  bound {bound:.2e}")
    assert e <= bound, f"{what}: {e:.3e} > {bound:.3e}"
    return e


# ------------------------------------------------------------------------------------------------ 1. offline
@pytest.mark.parametrize("causal,left_context", [(False, 0), (True, 0), (True, 24)], ids=["noncausal", "causal", "window24"])
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_offline_forward(gpu_device, cfg, causal, left_context):
    hidden, heads = CONFIGS[cfg]
    c = case(hidden, heads, 2, 3, 70, causal, left_context)
    m = build(gpu_device, hidden, heads, 2, causal, left_context, c["sd"])
    y = m(c["x"].to(gpu_device))
    check(f"offline {cfg} causal={causal} left_context={left_context}", y, c)
    assert torch.equal(y, m(c["x"].to(gpu_device)))  # and again: the same bits


def golden_case():
    g = np.load(TR.GOLDEN)
    sd, x = TR.golden_inputs(int(g["seed"]))
    return g, sd, x


@pytest.mark.parametrize("name,causal", [("offline_noncausal", False), ("offline_causal", True)])
def test_offline_forward_against_the_golden(gpu_device, name, causal):
    """The reference module's own output is the float32 yardstick here: bound 4 max(e_golden, 1e-6)."""
    g, sd, x = golden_case()
    S = TR.GOLDEN_SHAPE
    y64 = TR.forward(sd, x.double(), S["layers"], S["heads"], causal)
    e_g = TR.rel_err(torch.from_numpy(g[name]), y64)
    m = build(gpu_device, S["hidden"], S["heads"], S["layers"], causal, 0, sd)
    check(f"golden {name}", m(x.to(gpu_device)), dict(y64=y64, e32=e_g, bound=4 * max(e_g, 1e-6)))


# ------------------------------------------------------------------------------------------------ 2. cache mode
def test_cache_mode_against_the_golden(gpu_device):
    import unified_audio_amd as qa

    g, sd, x = golden_case()
    S = TR.GOLDEN_SHAPE
    state, ys64, t = TR.new_state(S["layers"]), [], 0
    for n in TR.GOLDEN_CHUNKS:
        ys64.append(TR.forward_cached(sd, x[:, t:t + n].double(), state, S["layers"], S["heads"]))
        t += n
    y64 = torch.cat(ys64, 1)
    e_g = TR.rel_err(torch.from_numpy(g["cached_noncausal"]), y64)
    m = build(gpu_device, S["hidden"], S["heads"], S["layers"], False, 0, sd)
    cache, ys, t = None, [], 0
    for n in TR.GOLDEN_CHUNKS:
        y, cache = m(x[:, t:t + n].to(gpu_device), past_key_values=cache, use_cache=True)
        assert isinstance(cache, qa.TransformerCache)
        ys.append(y)
        t += n
        assert cache.get_seq_length() == t
    check("cache mode (5, 7, 1, 11) vs golden", torch.cat(ys, 1), dict(y64=y64, e32=e_g, bound=4 * max(e_g, 1e-6)))
    # without use_cache the cache is still extended and the hidden states alone come back (transformer.py:486-489)
    cache.reset()
    assert cache.get_seq_length() == 0
    y = m(x[:, :5].to(gpu_device), past_key_values=cache)
    assert torch.is_tensor(y) and cache.get_seq_length() == 5 and torch.equal(y, ys[0])
    # a cache of another model is refused
    other = build(gpu_device, S["hidden"], S["heads"], S["layers"], False, 0, sd)
    with pytest.raises(qa.QuarkAudioError, match="another Transformer"):
        other(x[:, :5].to(gpu_device), past_key_values=cache, use_cache=True)
    assert cache.get_seq_length() == 5
    cache.free()
    with pytest.raises(qa.QuarkAudioError):
        m(x[:, :5].to(gpu_device), past_key_values=cache, use_cache=True)


def test_cache_mode_causal_fills_an_empty_cache_and_refuses_a_second_chunk(gpu_device):
    import unified_audio_amd as qa

    c = case(128, 2, 2, 3, 70, True, 0)
    m = build(gpu_device, 128, 2, 2, True, 0, c["sd"])
    x = c["x"].to(gpu_device)
    y, cache = m(x, use_cache=True)
    check("causal, empty cache", y, c)
    assert torch.equal(y, m(x))  # the offline causal call, bit for bit
    assert cache.get_seq_length() == 70
    with pytest.raises(qa.QuarkAudioError, match="qa_transformer_stream_begin"):
        m(x[:, :3], past_key_values=cache, use_cache=True)
    assert cache.get_seq_length() == 70


# ------------------------------------------------------------------------------------------------ 3. streaming equals offline
@pytest.mark.parametrize("left_context", [0, 24], ids=["full", "window24"])
@pytest.mark.parametrize("chunking", list(CHUNKINGS))
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_streaming_equals_offline(gpu_device, cfg, chunking, left_context):
    hidden, heads = CONFIGS[cfg]
    c = case(hidden, heads, 2, 3, 70, True, left_context)
    m = build(gpu_device, hidden, heads, 2, True, left_context, c["sd"])
    x = c["x"].to(gpu_device)
    e_off = TR.rel_err(m(x).cpu(), c["y64"])
    check(f"stream {cfg} {chunking} left_context={left_context}", stream(m, x, CHUNKINGS[chunking]), c, e_off)
    assert not m.is_streaming and m.streaming_offset == -1


def test_streaming_second_lstm_batch_tile(gpu_device):
    c = case(128, 2, 2, 17, 70, True, 0)
    m = build(gpu_device, 128, 2, 2, True, 0, c["sd"])
    x = c["x"].to(gpu_device)
    check("stream B = 17 mix", stream(m, x, MIX), c, TR.rel_err(m(x).cpu(), c["y64"]))


# ------------------------------------------------------------------------------------------------ 4. long history
def test_long_history_capacity_and_refusal(gpu_device):
    import unified_audio_amd as qa

    chunks = (1,) * 300 + (13,) * 20
    c = case(128, 2, 2, 2, 560, True, 0)
    m = build(gpu_device, 128, 2, 2, True, 0, c["sd"])
    x = c["x"].to(gpu_device)
    e_off = TR.rel_err(m(x).cpu(), c["y64"])
    out, t = [], 0
    with m.streaming(2, max_frames=560):
        for n in chunks:
            out.append(m(x[:, t:t + n]))
            t += n
        assert m.streaming_offset == 560  # max_frames reached exactly
        with pytest.raises(qa.QuarkAudioError, match="capacity 560"):
            m(x[:, :1])
        assert m.streaming_offset == 560
        y = torch.cat(out, 1)
        check("stream 300 x 1 + 20 x 13 = 560 frames", y, c, e_off)
        m.reset_streaming()
        again = torch.cat([m(x[:, i:i + 1]) for i in range(9)], 1)
        assert m.streaming_offset == 9 and torch.equal(again, y[:, :9])


# ------------------------------------------------------------------------------------------------ 5. reset and re-entry
def test_reset_and_reentry_reproduce_a_fresh_stream(gpu_device):
    c = case(128, 2, 2, 3, 70, True, 0)
    m = build(gpu_device, 128, 2, 2, True, 0, c["sd"])
    x = c["x"].to(gpu_device)
    head = (1, 1, 4, 16)

    def run(n_frames_before_reset):
        with m.streaming(3, max_frames=70):
            if n_frames_before_reset:
                m(x[:, 40:40 + n_frames_before_reset])  # other frames: LSTM state and cached rows to forget
                m.reset_streaming()
                assert m.streaming_offset == 0
            out, t = [], 0
            for n in head:
                out.append(m(x[:, t:t + n]))
                t += n
        return torch.cat(out, 1)

    fresh = run(0)
    assert torch.equal(fresh, run(0))    # two identical streams (leaving and re-entering streaming())
    assert torch.equal(fresh, run(30))   # after reset_streaming(): state zeroed, stale keys invisible
    assert torch.equal(fresh, run(5))


# ------------------------------------------------------------------------------------------------ 6. real widths
@pytest.mark.parametrize("hidden,heads", [(512, 8), (768, 8), (1536, 24)], ids=["d512_team", "d768_hd96", "d1536_persistent"])
def test_real_widths_stream_agrees_with_the_codecs_recurrence(gpu_device, hidden, heads):
    """Offline runs whichever recurrence the codec itself uses at this width (team / persistent kernel), the stream the per-step carry."""
    c = case(hidden, heads, 1, 2, 40, True, 0)
    m = build(gpu_device, hidden, heads, 1, True, 0, c["sd"])
    x = c["x"].to(gpu_device)
    e_off = check(f"offline d = {hidden}", m(x), c)
    check(f"stream d = {hidden} (1, 1, 6, 16, 16)", stream(m, x, (1, 1, 6, 16, 16)), c, e_off)


# ------------------------------------------------------------------------------------------------ 7. the short-chunk kernel alone
def test_short_chunk_kernel_against_attention_kernel(gpu_device, knob):
    c = case(128, 2, 2, 3, 70, True, 0)
    m = build(gpu_device, 128, 2, 2, True, 0, c["sd"])
    x = c["x"].to(gpu_device)
    e_off = TR.rel_err(m(x).cpu(), c["y64"])
    chunks = (1,) * 6 + (4,) * 4 + (16,) * 3
    res = {}
    for on in (2, 0):
        knob("QA_TR_SHORT_ATTN", on)
        res[on] = stream(m, x, chunks)
        check(f"QA_TR_SHORT_ATTN={on}", res[on], c, e_off)
    assert not torch.equal(res[0], res[2])  # two kernels: the knob does select
    knob("QA_TR_SHORT_ATTN", 2)
    # the same 4-frame chunk at offset 40 in caches of capacity 64 and 560: other split lengths, the same result within the bound
    for cap in (64, 560):
        y = stream(m, x[:, :44], (40, 4), max_frames=cap)
        check(f"4 frames at offset 40, capacity {cap}", y[:, 40:], dict(c, y64=c["y64"][:, 40:44]), e_off)


@pytest.mark.parametrize("B,same_as", [(16, 2), (17, 0)], ids=["B16_short", "B17_attention_kernel"])
def test_short_chunk_selection_by_batch_times_frames(gpu_device, knob, B, same_as):
    """The default (QA_TR_SHORT_ATTN = 1) takes the short-chunk kernel up to batch x frames = 256 and attention_kernel above: 16-frame steps at
    B = 16 hold the bits of the forced short-chunk kernel (2), at B = 17 those of attention_kernel (0); both within the bound."""
    c = case(128, 2, 2, B, 70, True, 0)
    m = build(gpu_device, 128, 2, 2, True, 0, c["sd"])
    x = c["x"].to(gpu_device)[:, :64]
    c64 = dict(c, y64=c["y64"][:, :64])
    e_off = TR.rel_err(m(c["x"].to(gpu_device)).cpu()[:, :64], c64["y64"])
    res = {}
    for mode in (1, same_as, 2 - same_as):
        knob("QA_TR_SHORT_ATTN", mode)
        res[mode] = stream(m, x, (16,) * 4)
    check(f"B = {B}, 16-frame steps, default selection", res[1], c64, e_off)
    assert torch.equal(res[1], res[same_as]) and not torch.equal(res[1], res[2 - same_as])


def test_short_chunk_step_is_chunking_invariant_bit_for_bit(gpu_device, knob):
    """A 1-frame step at offset 40 whether the offset is reached by 40 single steps or by (33, 7).  One layer: its LSTM state and cached K / V
    rows come from the row-wise GEMMs and the per-step recurrence alone, so they hold the same bits however the history was chunked, and the
    short-chunk kernel's fixed key ranges make the step a function of (cache, offset).  (A second layer reads the first one's attention output,
    which for the 33-frame chunk comes from attention_kernel: equal within the bound, not bit for bit.)"""
    knob("QA_TR_SHORT_ATTN", 2)
    c = case(128, 2, 1, 3, 70, True, 0)
    m = build(gpu_device, 128, 2, 1, True, 0, c["sd"])
    x = c["x"].to(gpu_device)
    a = stream(m, x[:, :41], (1,) * 41, max_frames=70)
    b = stream(m, x[:, :41], (33, 7, 1), max_frames=70)
    assert torch.equal(a[:, 40], b[:, 40])


# ------------------------------------------------------------------------------------------------ 8. launch_lstm_carry directly
@pytest.mark.parametrize("d", [128, 512])
@pytest.mark.parametrize("B", [3, 17])
def test_lstm_carry_in_pieces(qa_lib, gpu_device, B, d):
    T, pieces = 37, (1, 1, 2, 33)
    g = torch.Generator().manual_seed(100 * B + d)
    xw = torch.randn(B, T, 4 * d, generator=g)
    w_hh = (torch.rand(4 * d, d, generator=g) * 2 - 1) * (2.0 / d ** 0.5)
    h64, c64 = L.recurrence(xw.double(), w_hh.double())
    h32, c32 = L.recurrence(xw, w_hh)
    e32 = max(TR.rel_err(h32, h64), TR.rel_err(c32[:, -1], c64[:, -1]))
    bound = 4 * max(e32, 1e-6)
    w_ug = L.unit_gate_rows(w_hh).to(gpu_device)
    xw_ug = L.unit_gate_rows(xw.movedim(2, 0)).movedim(0, 2).contiguous()
    hs = torch.zeros(B, d, device=gpu_device)
    cs = torch.zeros(B, d, device=gpu_device)
    out, t = [], 0
    s = torch.cuda.current_stream().cuda_stream
    for n in pieces:
        piece = xw_ug[:, t:t + n].contiguous().to(gpu_device)
        h = torch.empty(B, n, d, device=gpu_device)
        st = qa_lib.qa_debug_lstm_carry(piece.data_ptr(), w_ug.data_ptr(), h.data_ptr(), hs.data_ptr(), cs.data_ptr(), B, n, d, s)
        assert st == 0, qa_lib.qa_last_error()
        torch.cuda.synchronize()
        assert torch.equal(hs, h[:, -1])  # the carried state is the chunk's last row
        out.append(h)
        t += n
    h = torch.cat(out, 1).cpu()
    e_h, e_c = TR.rel_err(h, h64), TR.rel_err(cs.cpu(), c64[:, -1])
    print(f"lstm carry B = {B} d = {d}: h {e_h:.2e} c_T {e_c:.2e}  e_cpu32 {e32:.2e}  bound {bound:.2e}")
    assert e_h <= bound and e_c <= bound
