"""Streams without an end on the GPU: the ring forms of rope_append_kernel / attn_short_kernel through
qa_debug_stream_attn, the ring stream of unified_audio_amd.Transformer and the windowed ring stream of the causal H-Codec 1.0 encoder.

Bounds.  Block level: e = max|y - y64| / max|y64| against the float64 restatement, at most 4 max(e_cpu32, 1e-6) with e_cpu32 the float32
CPU restatement's own error on the same inputs; where the unchanged offline forward on the shape measures worse, 2 e_offline (the rule
of tests/test_transformer_stream_gpu.py).  Codec level: STAGE_TOL = 5e-5 relative RMS, as in tests/test_hcodec_stream_gpu.py, and EQUAL
codes (the case has no near-tie: tests/test_stream_ring_cpu.py).  Every figure is printed before it is asserted."""
import functools

import pytest
import torch

from tests import hcodec_stream_ref as S
from tests import ring_stream_ref as RS
from tests import transformer_stream_ref as TR
from tests.test_transformer_stream_gpu import build, check
from tests.util import rel_err, with_knob

pytestmark = pytest.mark.gpu

STAGE_TOL = 5e-5
HIDDEN, HEADS, LAYERS = 128, 2, 2  # the block of the stream tests
NEAR_2_24 = RS.MAX_POSITIONS - 20


def _stream_ptr(dev):
    return torch.cuda.current_stream(dev).cuda_stream


# ------------------------------------------------------------------------------------------------ 6. the kernels alone
class Rings:
    """The caches of B items on the device (NaN to begin with) beside their float64 and float32 twins on the host.  step() runs one
    qa_debug_stream_attn and the restatements of the same step; fill() brings every item to its position by such appends from position
    0 - or, for a position far away, from the last `cap` positions in front of it: earlier ones would be overwritten anyway."""

    def __init__(self, qa_lib, dev, B, hd, cap, seed):
        self.lib, self.dev, self.B, self.hd, self.cap, self.d = qa_lib, dev, B, hd, cap, 2 * hd
        self.g = torch.Generator().manual_seed(seed)
        self.kc = torch.full((B, cap, self.d), float("nan"), device=dev)
        self.vc = torch.full((B, cap, self.d), float("nan"), device=dev)
        self.ref = {dt: [torch.full((B, cap, self.d), float("nan"), dtype=dt) for _ in range(2)] for dt in (torch.float64, torch.float32)}

    def step(self, n, context, pos, nq, ring=1, long_form=0, rows=True):
        """pos / nq: per item.  rows: through the per-row arrays; else every item shares pos[0] and takes all n frames."""
        B, d = self.B, self.d
        qkv = torch.randn(B, n, 3 * d, generator=self.g)
        q_dev, out = qkv.to(self.dev), torch.full((B, n, d), float("nan"), device=self.dev)
        if rows:
            p_dev = torch.tensor(pos, dtype=torch.int32, device=self.dev)
            n_dev = torch.tensor(nq, dtype=torch.int32, device=self.dev)
            args = (0, p_dev.data_ptr(), n_dev.data_ptr())
        else:
            assert all(p == pos[0] for p in pos) and all(c == n for c in nq)
            args = (pos[0], None, None)
        st = self.lib.qa_debug_stream_attn(q_dev.data_ptr(), self.kc.data_ptr(), self.vc.data_ptr(), out.data_ptr(), B, n, HEADS, self.hd, self.cap,
                                           context, ring, *args, long_form, _stream_ptr(self.dev))
        assert st == 0, self.lib.qa_last_error()
        res = {}
        for dt, (kc, vc) in self.ref.items():
            ys = []
            for b in range(B):
                y, kc[b], vc[b] = RS.attn_step_ref(qkv[b], kc[b], vc[b], HEADS, self.cap, context, pos[b], nq[b], ring, dt)
                ys.append(y)
            res[dt] = torch.stack(ys)
        return out.cpu(), res[torch.float64], res[torch.float32]

    def fill(self, context, start, upto):
        """Appends of up to 16 frames per item from start[b] to upto[b] (the attention outputs of these steps are not looked at)."""
        at = list(start)
        while any(a < u for a, u in zip(at, upto)):
            nq = [min(16, u - a) for a, u in zip(at, upto)]
            self.step(16, min(context, self.cap - 15), at, nq)  # a window these 16-frame appends fit under; their outputs are not used
            at = [a + c for a, c in zip(at, nq)]


def _edge_cases(cap):
    """(name, B, window, n, positions, live frames, long_form).  Splits of a (row, head) are 64 rows, tiles 32."""
    W_tight = lambda n: cap - n + 1  # noqa: E731
    same = lambda p, n: ([p] * 3, [n] * 3)  # noqa: E731
    return [
        ("first step, ring mostly unwritten", 3, 40, 4, *same(0, 4), 0),
        ("end inside a tile", 3, 40, 4, *same(2 * cap + 6, 4), 0),              # e mod cap = 10
        ("end on a tile edge", 3, 40, 16, *same(3 * cap + 16, 16), 0),          # e mod cap = 32
        ("end on the split edge", 3, 40, 4, *same(cap + 60, 4), 0),             # e mod cap = 64 (cap 96) / 0 (cap 64)
        ("end on the physical end", 3, 40, 1, *same(4 * cap - 1, 1), 0),        # e mod cap = 0
        ("window of 5, one frame", 3, 5, 1, *same(cap + 33, 1), 0),
        ("window of 5, 16 frames across the end", 3, 5, 16, *same(2 * cap - 7, 16), 0),
        ("tightest window, n = 1", 3, W_tight(1), 1, *same(5 * cap + 3, 1), 0),
        ("tightest window, n = 4", 3, W_tight(4), 4, *same(2 * cap - 2, 4), 0),
        ("tightest window, n = 16", 3, W_tight(16), 16, *same(cap + 20, 16), 0),
        ("visible keys straddle the physical end", 3, 40, 4, *same(cap + 8, 4), 0),
        ("before the first wrap, tight window", 3, W_tight(16), 16, *same(cap - 30, 16), 0),
        # rows at offset 0 (a first step), below cap, several wraps, about 1e6, and an idle row, in one launch
        ("rows far apart", 5, 40, 16, [0, cap - 20, 3 * cap + 11, 1000003, cap + 5], [16, 7, 16, 1, 0], 0),
        ("rows, the live frames differ", 3, 33, 4, [2 * cap + 30, 17, 7 * cap - 2], [1, 4, 3], 0),
        ("near 2^24", 3, 40, 16, [NEAR_2_24, NEAR_2_24 + 4, NEAR_2_24 - 50], [16, 16, 9], 0),
        ("long form, 33 frames", 3, cap - 33, 33, *same(2 * cap + 9, 33), 1),
    ]


@pytest.mark.parametrize("hd,cap", [(64, 64), (128, 96)], ids=["hd64_cap64", "hd128_cap96"])
def test_ring_kernel_edges(qa_lib, gpu_device, hd, cap):
    """One rope-append plus attention over NaN-initialised rings at chosen positions: float64 parity and every output finite.  A row that
    is never written stays NaN in the cache, so a kernel that multiplied it by a zero probability would show it."""
    worst = 0.0
    for i, (name, B, W, n, pos, nq, long_form) in enumerate(_edge_cases(cap)):
        assert cap >= RS.min_rows(W, n) + long_form and all(p + c <= RS.MAX_POSITIONS for p, c in zip(pos, nq))
        r = Rings(qa_lib, gpu_device, B, hd, cap, 1000 * cap + i)
        # the long form reads every row of the ring, so its ring is full (pos >= cap); the short kernel's may hold NaN
        r.fill(W, [max(0, p - cap) for p in pos], pos)
        together = len(set(pos)) == 1 and all(c == n for c in nq)  # the rectangular launch where the case allows it
        y, y64, y32 = r.step(n, W, pos, nq, long_form=long_form, rows=not together)
        scale = float(y64.abs().max())
        e, e32 = float((y.double() - y64).abs().max()) / scale, float((y32.double() - y64).abs().max()) / scale
        bound = 4 * max(e32, 1e-6)
        unwritten = int(torch.isnan(r.kc[:, :, 0]).sum())
        print(f"hd {hd} cap {cap} {name}: W {W} n {n} pos {pos} nq {nq}: e {e:.2e}  e_cpu32 {e32:.2e}  bound {bound:.2e}  ({unwritten} rows unwritten)")
        assert torch.isfinite(y).all(), name
        assert all(bool((y[b, c:] == 0).all()) for b, c in enumerate(nq)), name  # behind a row's frames: exact zeros
        assert e <= bound, f"{name}: {e:.3e} > {bound:.3e}"
        # the appended rows: the cache holds the restatement's keys where it has any, NaN where it has none
        kc, kc64 = r.kc.cpu().double(), r.ref[torch.float64][0]
        assert torch.equal(torch.isnan(kc), torch.isnan(kc64)), name
        ek = float((kc - kc64).nan_to_num().abs().max() / kc64.nan_to_num().abs().max())
        assert ek <= 1e-6, f"{name}: cached keys off by {ek:.2e}"  # two fp32 products and a sum per element
        worst = max(worst, e)
    print(f"hd {hd} cap {cap}: worst e {worst:.2e}")


def test_ring_kernel_before_the_wrap_is_the_linear_kernel_bit_for_bit(qa_lib, gpu_device):
    """The same appends and the same step into a ring and into a linear cache of the same rows: while e <= cap the outputs hold the
    same bits, whatever the ring holds behind e."""
    hd, cap, W, B = 64, 96, 40, 3
    for rows in (False, True):
        a, b = Rings(qa_lib, gpu_device, B, hd, cap, 7), Rings(qa_lib, gpu_device, B, hd, cap, 7)
        at = [0] * B
        for n, nq in ((16, [16] * B), (4, [4] * B), (16, [16] * B), (1, [1] * B), (16, [16] * B), (16, [16] * B), (16, [16] * B), (11, [11] * B)):
            if rows and n == 4:
                nq = [4, 0, 3]
            ya, _, _ = a.step(n, W, at, nq, ring=1, rows=rows)
            yb, _, _ = b.step(n, W, at, nq, ring=0, rows=rows)
            assert torch.equal(ya, yb), (rows, at, nq)
            at = [p + c for p, c in zip(at, nq)]
        assert max(at) == cap


# ------------------------------------------------------------------------------------------------ the block
@functools.lru_cache(maxsize=None)
def block_case(B, T, W, seed=31):
    sd = TR.random_state_dict(seed, HIDDEN, 2 * HIDDEN, LAYERS)
    x = torch.randn(B, T, HIDDEN, generator=torch.Generator().manual_seed(seed + 1))
    y64 = TR.forward(sd, x.double(), LAYERS, HEADS, True, W)
    e32 = TR.rel_err(TR.forward(sd, x, LAYERS, HEADS, True, W), y64)
    return dict(sd=sd, x=x, y64=y64, e32=e32, bound=4 * max(e32, 1e-6))


def ring_steps(m, x, chunks):
    """x through the CURRENT stream of m, chunk by chunk -> the list of outputs (device)."""
    out, t = [], 0
    for n in chunks:
        out.append(m(x[:, t:t + n]))
        t += n
    return out


# 7.
def test_ring_stream_before_the_wrap_is_the_linear_stream(gpu_device):
    W = 40
    c = block_case(2, 96, W)
    m = build(gpu_device, HIDDEN, HEADS, LAYERS, True, W, c["sd"])
    x = c["x"].to(gpu_device)
    e_off = TR.rel_err(m(x).cpu(), c["y64"])
    for max_chunk, chunks, short in ((16, (1, 1, 4, 16, 7, 16, 3, 16), True), (40, (33, 17, 40, 6), False)):
        T = sum(chunks)
        with m.streaming(2, max_chunk=max_chunk):
            cap = m.streaming_capacity
            assert cap == RS.capacity(W, max_chunk) == T
            ring = ring_steps(m, x[:, :T], chunks)
            assert m.streaming_offset == T
        with m.streaming(2, max_frames=cap):
            assert m.streaming_capacity == cap
            lin = ring_steps(m, x[:, :T], chunks)
        same = [torch.equal(a, b) for a, b in zip(ring, lin)]
        cT = dict(c, y64=c["y64"][:, :T])
        check(f"ring, max_chunk {max_chunk}, before the wrap", torch.cat(ring, 1), cT, e_off)
        check(f"linear, capacity {cap}", torch.cat(lin, 1), cT, e_off)
        print(f"max_chunk {max_chunk} chunks {chunks}: steps bit-equal to the linear stream: {same}")
        if short:  # every step on the short-chunk kernel: the bits of the linear stream
            assert all(same)
    assert m.streaming_capacity == -1


# 8.
def test_ring_stream_against_the_windowed_offline_truth(gpu_device):
    """704 frames in mixed chunks of 1 .. 16 through a ring of 64 rows, eleven turns, against TR.forward(..., left_context = 40) in
    float64 (600 frames, which the ring of 64 rows that this window and chunk get would turn 9.4 times, are not ten wraps)."""
    W, T = 40, 704
    chunks = (1, 16, 3, 7, 16, 2, 11, 4, 16, 12) * 8
    assert sum(chunks) == T and set(range(1, 17)) >= set(chunks) and {1, 16} <= set(chunks)
    c = block_case(2, T, W)
    m = build(gpu_device, HIDDEN, HEADS, LAYERS, True, W, c["sd"])
    x = c["x"].to(gpu_device)
    e_off = TR.rel_err(m(x).cpu(), c["y64"])
    with m.streaming(2, max_chunk=16):
        assert m.streaming_capacity == 64 and T >= 10 * m.streaming_capacity
        y = torch.cat(ring_steps(m, x, chunks), 1)
        assert m.streaming_offsets == [T, T]
    check(f"ring stream, {T} frames, {T / 64:.0f} turns", y, c, e_off)
    e_tail = TR.rel_err(y[:, -64:].cpu(), c["y64"][:, -64:])
    print(f"last turn alone: {e_tail:.2e}")


# 9.
@functools.lru_cache(maxsize=None)
def table_case():
    """B = 1, W = 40, 8192 + 300 frames: the float64 and float32 STREAMING restatements with a carried state (no 8492^2 offline matrix)."""
    W, T = 40, 8192 + 300
    chunks = (512,) * 15 + (1, 16) * 31 + (1,) * 29 + (256,)
    assert sum(chunks) == T and sum(chunks[:15]) == 7680 and 7680 + 17 * 31 > 8192 + 1
    sd = TR.random_state_dict(41, HIDDEN, 2 * HIDDEN, LAYERS)
    x = torch.randn(1, T, HIDDEN, generator=torch.Generator().manual_seed(42))
    coarse = (512,) * 16 + (300,)  # the restatement's own chunking does not matter (tests/test_transformer_stream_cpu.py)
    y64 = TR.stream(sd, x.double(), coarse, LAYERS, HEADS, W)
    e32 = TR.rel_err(TR.stream(sd, x, coarse, LAYERS, HEADS, W), y64)
    return dict(sd=sd, x=x, y64=y64, e32=e32, bound=4 * max(e32, 1e-6), chunks=chunks, W=W)


def test_ring_stream_past_the_static_rope_table(gpu_device):
    """Steps of 512 (attention_kernel's ring mode) up to 7680, steps of 1 and 16 (the ring kernels) across position 8192, a step of 256
    behind it: beyond the table the angles come from the table's formula in the kernel."""
    c = table_case()
    m = build(gpu_device, HIDDEN, HEADS, LAYERS, True, c["W"], c["sd"])
    x = c["x"].to(gpu_device)
    with m.streaming(1, max_chunk=512):
        assert m.streaming_capacity == 576
        y = torch.cat(ring_steps(m, x, c["chunks"]), 1).cpu()
        assert m.streaming_offset == 8192 + 300
    check("ring stream, 8492 frames", y, c)
    for name, a, b in (("below the table's end", 7680, 8192), ("beyond it", 8192, 8492)):
        e = float((y[:, a:b].double() - c["y64"][:, a:b]).abs().max() / c["y64"].abs().max())
        print(f"positions {a} .. {b - 1} ({name}): e {e:.2e}")
        assert e <= c["bound"]


# 10.
def test_rows_across_the_wrap(gpu_device):
    """B = 3 on a ring of 64 rows, 16-frame rectangles.  Rows 1 and 2 carry row 0's signal: row 1 starts three steps late, row 2 idles
    twice on the way; both must repeat row 0 bit for bit, turns of the ring included.  Then row 0, which has wrapped, is reset and
    repeats its own first steps bit for bit while the others go on: stale rows of the ring are invisible."""
    W, T, n = 40, 160, 16
    c = block_case(1, T, W, seed=51)
    m = build(gpu_device, HIDDEN, HEADS, LAYERS, True, W, c["sd"])
    sig = c["x"][0].to(gpu_device)
    steps = T // n
    #            row 0             row 1 (late)      row 2 (idles at steps 4 and 7)
    plan = []  # per step: the segment index of every row, or None
    seg = [0, 0, 0]
    for s in range(steps + 3):
        take = [s < steps, 3 <= s, s not in (4, 7) and seg[2] < steps]
        take = [t and seg[b] < steps for b, t in enumerate(take)]
        plan.append([seg[b] if t else None for b, t in enumerate(take)])
        seg = [v + 1 if t else v for v, t in zip(seg, take)]
    assert seg == [steps] * 3
    got = [[None] * steps for _ in range(3)]
    with with_knob("QA_TR_SHORT_ATTN", 2):
        with m.streaming(3, max_chunk=n):
            assert m.streaming_capacity == 64
            offs = [0, 0, 0]
            for row in plan:
                x = torch.full((3, n, HIDDEN), float("nan"), device=gpu_device)  # behind a row's frames nothing is read
                for b, k in enumerate(row):
                    if k is not None:
                        x[b] = sig[k * n:(k + 1) * n]
                y = m(x, lengths=[n if k is not None else 0 for k in row])
                offs = [o + (n if k is not None else 0) for o, k in zip(offs, row)]
                assert m.streaming_offsets == offs  # an idle row keeps its offset
                for b, k in enumerate(row):
                    if k is None:
                        assert bool((y[b] == 0).all())
                    else:
                        got[b][k] = y[b].clone()
            # row 0 has turned the ring 2.5 times: reset it, and let it repeat its first steps beside row 1 going on alone
            m.reset_streaming(rows=[0])
            assert m.streaming_offsets == [0, T, T]
            again = []
            for k in range(4):
                x = torch.full((3, n, HIDDEN), float("nan"), device=gpu_device)
                x[0] = sig[k * n:(k + 1) * n]
                x[1] = sig[k * n:(k + 1) * n]
                y = m(x, lengths=[n, n, 0])
                assert torch.isfinite(y).all()
                again.append(y[0].clone())
            assert m.streaming_offsets == [4 * n, T + 4 * n, T]
    y0 = torch.cat(got[0], 0)
    check("row 0 across the wrap", y0[None], c)
    for b in (1, 2):
        assert all(torch.equal(got[b][k], got[0][k]) for k in range(steps)), f"row {b} differs from row 0"
    assert all(torch.equal(again[k], got[0][k]) for k in range(4)), "a reset row does not repeat a fresh stream's first steps"


# ------------------------------------------------------------------------------------------------ 11. H-Codec
@pytest.fixture(scope="module")
def codec_case(gpu_device):
    import unified_audio_amd as qa

    ospec, sd, wav = RS.codec_inputs()
    codec = qa.Codec(None, None, None, spec=qa.HCodecSpec(**RS.CAUSAL_MINI), device=gpu_device).load_state_dict(sd)
    return dict(ospec=ospec, sd=sd, wav=wav, codec=codec, oracle={W: RS.windowed_oracle(sd, wav, ospec, W) for W in RS.CODEC_WINDOWS},
                full=S.oracle_emb_and_codes(sd, wav, ospec))


def codec_steps(codec, ospec, wav, chunks, dev):
    hop, t, acs, embs = ospec.enc_hop, 0, [], []
    for n in chunks:
        ac, emb = codec.encode_stream(wav[..., t * hop:(t + n) * hop].to(dev), return_emb=True)
        acs.append(ac)
        embs.append(emb)
        t += n
    return torch.cat(acs, 2), torch.cat(embs, 1)


@pytest.mark.parametrize("W", RS.CODEC_WINDOWS)
def test_windowed_codec_stream_equals_the_windowed_oracle(gpu_device, codec_case, W):
    """Codec.streaming(3, left_context = W, max_chunk = 5): not the shipped full-causal encoder but the SEANet encoder whose Transformer
    has use_sliding_window=True, left_context=W.  72 code frames = 144 Transformer frames through a ring of 32 rows."""
    codec, ospec, wav = codec_case["codec"], codec_case["ospec"], codec_case["wav"]
    emb_o, ac_o = codec_case["oracle"][W]
    N = RS.CODEC_CASE["frames"]
    for name, chunks in RS.CODEC_CHUNKINGS.items():
        with codec.streaming(3, left_context=W, max_chunk=RS.CODEC_MAX_CHUNK):
            assert codec.streaming_capacity == RS.capacity(W, 2 * RS.CODEC_MAX_CHUNK) // 2 == 16
            ac, emb = codec_steps(codec, ospec, wav, chunks, gpu_device)
            assert codec.streaming_offset == N
        e = rel_err(emb, emb_o.transpose(1, 2))
        diff = int((ac.cpu() != ac_o).sum())
        print(f"W {W} {name}: emb against the windowed oracle {e:.2e}; {diff} of {ac_o.numel()} codes differ")
        assert e < STAGE_TOL
        assert ac_o.numel() == 648 and diff == 0
    # the window is live: the linear (full-causal) stream of the same signal gives other codes, and so does the full-causal oracle
    with codec.streaming(3, max_frames=N):
        ac_full, emb_full = codec_steps(codec, ospec, wav, RS.CODEC_CHUNKINGS["2+5x14"], gpu_device)
    n_lin, n_or = int((ac_full.cpu() != ac_o).sum()), int((codec_case["full"][1] != ac_o).sum())
    print(f"W {W}: the linear stream differs from the windowed oracle in {n_lin} codes (the full-causal oracle in {n_or}); "
          f"its emb against the full-causal oracle {rel_err(emb_full, codec_case['full'][0].transpose(1, 2)):.2e}")
    assert n_lin >= 1


# ------------------------------------------------------------------------------------------------ 12. refusals
def test_transformer_ring_refusals_leave_the_stream_as_it_was(qa_lib, gpu_device):
    import unified_audio_amd as qa

    W = 40
    c = block_case(2, 96, W)
    m = build(gpu_device, HIDDEN, HEADS, LAYERS, True, W, c["sd"])
    x = c["x"].to(gpu_device)
    e_off = TR.rel_err(m(x).cpu(), c["y64"])
    # a ring on a handle without a window; a capacity above the cache limit
    for other in (build(gpu_device, HIDDEN, HEADS, LAYERS, True, 0, c["sd"]), build(gpu_device, HIDDEN, HEADS, LAYERS, False, 0, c["sd"])):
        with pytest.raises(qa.QuarkAudioError, match="left_context = 0"):
            other.streaming_forever(2, max_chunk=16)
        assert not other.is_streaming and other.streaming_capacity == -1
    with pytest.raises(qa.QuarkAudioError, match="8160"):
        m.streaming_forever(2, max_chunk=8160)  # 40 + 8160 = 8200 rows -> 8224 > 8192
    with pytest.raises(qa.QuarkAudioError, match="one of them"):
        m.streaming_forever(2, max_frames=96, max_chunk=16)
    assert not m.is_streaming
    with m.streaming(2, max_chunk=16):
        out = [m(x[:, :16])]
        with pytest.raises(qa.QuarkAudioError, match="takes 17 frames.*max_chunk 16"):  # a chunk above max_chunk
            m(x[:, 16:33])
        with pytest.raises(qa.QuarkAudioError, match="row 1 takes 17 frames"):
            m(x[:, 16:33], lengths=[3, 17])
        with pytest.raises(qa.QuarkAudioError, match="short-chunk attention"), with_knob("QA_TR_SHORT_ATTN", 0):  # per-row lengths off the short kernel
            m(x[:, 16:32], lengths=[3, 16])
        side = torch.cuda.Stream(gpu_device)  # a stream under capture
        side.wait_stream(torch.cuda.current_stream(gpu_device))
        graph, x1 = torch.cuda.CUDAGraph(), x[:, 16:17].contiguous()
        with pytest.raises(qa.QuarkAudioError, match="stream capture"):
            with torch.cuda.graph(graph, stream=side):
                m(x1)
        torch.cuda.synchronize()
        assert m.streaming_offsets == [16, 16]
        out += ring_steps(m, x[:, 16:], (16,) * 5)
    check("after the refusals, 96 frames", torch.cat(out, 1), c, e_off)
    # a row past 2^24 positions: nothing short of 2^24 frames gets a stream there, so the check is exercised through the kernels' entry
    r = Rings(qa_lib, gpu_device, 3, 64, 64, 5)
    qkv = torch.zeros(3, 16, 3 * 128, device=gpu_device)
    st = qa_lib.qa_debug_stream_attn(qkv.data_ptr(), r.kc.data_ptr(), r.vc.data_ptr(), qkv.data_ptr(), 3, 16, HEADS, 64, 64, 40, 1,
                                     RS.MAX_POSITIONS - 15, None, None, 0, _stream_ptr(gpu_device))
    assert st != 0 and str(RS.MAX_POSITIONS - 15) in qa_lib.qa_last_error().decode()
    assert bool(torch.isnan(r.kc).all())  # refused before any launch


def test_codec_ring_refusals_leave_the_stream_as_it_was(gpu_device, codec_case):
    import unified_audio_amd as qa

    codec, ospec, wav = codec_case["codec"], codec_case["ospec"], codec_case["wav"].to(gpu_device)
    hop, W = ospec.enc_hop, 12
    emb_o, ac_o = codec_case["oracle"][W]
    with pytest.raises(qa.QuarkAudioError, match="left_context 0"):
        codec.streaming_forever(3, left_context=0, max_chunk=5)
    with pytest.raises(qa.QuarkAudioError, match="max_chunk_frames 1 "):  # below the first-chunk minimum
        codec.streaming_forever(3, left_context=W, max_chunk=1)
    with pytest.raises(qa.QuarkAudioError, match="ring of 8224 rows"):
        codec.streaming_forever(3, left_context=8000, max_chunk=100)
    assert not codec.is_streaming and codec.streaming_capacity == -1
    with codec.streaming(3, left_context=W, max_chunk=9):
        ac_a, emb_a = codec.encode_stream(wav[..., :2 * hop], return_emb=True)
        with pytest.raises(qa.QuarkAudioError, match="takes 10 code frames.*max_chunk 9"):
            codec.encode_stream(wav[..., 2 * hop:12 * hop])
        with pytest.raises(qa.QuarkAudioError, match="short-chunk attention"):  # 9 code frames = 18 Transformer frames with per-row lengths
            codec.encode_stream(wav[..., 2 * hop:11 * hop], lengths=[9, 9, 4])
        assert codec.streaming_offsets == [2, 2, 2]
        ac_b, emb_b = codec_steps(codec, ospec, wav[..., 2 * hop:], (9, 1, 5) * 4 + (9, 1), gpu_device)
        assert codec.streaming_offset == 72
    emb, ac = torch.cat((emb_a, emb_b), 1), torch.cat((ac_a, ac_b), 2)
    e = rel_err(emb, emb_o.transpose(1, 2))
    print(f"after the refusals: emb {e:.2e}, {int((ac.cpu() != ac_o).sum())} codes differ")
    assert e < STAGE_TOL and torch.equal(ac.cpu(), ac_o)
