"""Per-row lengths, offsets and resets of the H-Codec 1.0 stream on the GPU (Codec.encode_stream(lengths=) / reset_streaming(rows=) ->
qa_hcodec_stream_encode_rows / _reset_rows), and the block-level twin on Transformer.

The definition of correct, per row: between two of its resets, the row's concatenated outputs equal one offline causal encode of its own
waveform - whatever its neighbours did.  The yardstick is the oracle of the offline causal graph (tests/hcodec_stream_ref.oracle_emb_and_codes).
The schedule (tests/hcodec_stream_rows_ref.SCHEDULE; code frames per step, rows 0 - 3, rows 0 and 1 carrying one waveform three steps apart):

    step 0   2 0 3 0    row 2 longer than the others; rows 1, 3 not started
    step 1   2 0 1 2    row 3 joins mid-stream
    step 2   2 0 0 1    row 2 idles
    step 3   2 2 2 1    row 1 joins beside three running rows
             reset row 2
    step 4   2 2 2 1    row 2 is first again
    step 5   2 2 1 0
    step 6   1 2 1 3    rectangle wider than rows 0 - 2
    step 7   1 2 1 1

Every step's rectangle is 3 code frames wide (the schedule's longest entry), so that rows 0 and 1 meet their chunks in rectangles of the
same width; the samples behind a row's frames are NaN in every step.

Measured on one MI355X (QA_TR_SHORT_ATTN = 1 | 0 | 2): emb against the oracle 6.7e-07 - 8.0e-07 per segment (bound 5e-05), 0 of 132 codes
differ; block level e = 2.9e-07 - 4.1e-07 against bounds of 4.0e-06, 3.0e-07 - 3.5e-07 across 1 - 3 key splits."""
import ctypes as C
import functools

import pytest
import torch

from oracle import hcodec_ref as R
from oracle import synth
from tests import hcodec_stream_ref as S
from tests import hcodec_stream_rows_ref as RR
from tests import transformer_stream_ref as TR
from tests.util import CODE_TIE_TOL, MINI, audit_codes_bnq, check_guarded_out, guarded_out, rel_err, with_knob

pytestmark = pytest.mark.gpu

STAGE_TOL = 5e-5  # relative RMS: the bound the rectangular stream and the offline graph are held to against the same oracle
CAUSAL_MINI = dict(MINI, causal=True)
MAX_FRAMES = 16
CODE_GUARD = -(1 << 40)  # sentinel around the int64 code outputs


def _stream_ptr(dev):
    return torch.cuda.current_stream(dev).cuda_stream


@functools.lru_cache(maxsize=None)
def _case(dev):
    """The codec, the schedule's waveforms and the oracle's offline encode of every segment: computed once, shared, left unchanged."""
    import unified_audio_amd as qa

    ospec, sd, segs, waves = RR.case_inputs(RR.GPU_ROWS_CASE, CAUSAL_MINI)
    codec = qa.Codec(None, None, None, spec=qa.HCodecSpec(**CAUSAL_MINI), device=dev).load_state_dict(sd)
    oracle = [S.oracle_emb_and_codes(sd, w, ospec) for w in waves]
    rect = [(x[:, 0].contiguous().to(dev), fr) for x, fr in RR.rectangles(ospec, segs, waves)]
    return dict(ospec=ospec, sd=sd, segs=segs, waves=waves, codec=codec, oracle=oracle, rect=rect,
                cb=R.rvq_codebooks(sd, "quantizer", ospec.num_quantizers))


def _step_guarded(qa_lib, codec, ospec, x, lengths, dev):
    """One qa_hcodec_stream_encode_rows with both outputs between sentinels -> (codes [B, nq, n], emb [B, n, D])."""
    B, n = x.shape[0], x.shape[1] // ospec.enc_hop
    Q, D = ospec.num_quantizers, ospec.code_dim
    ebuf, emb = guarded_out(B * n, D, D, 4, dev)
    cbuf = torch.full((B * Q * n + 16,), CODE_GUARD, dtype=torch.int64, device=dev)
    ac = cbuf[8:8 + B * Q * n]
    ac.fill_(CODE_GUARD + 1)
    st = qa_lib.qa_hcodec_stream_encode_rows(codec._handle, x.data_ptr(), x.shape[1], (C.c_int64 * B)(*lengths), ac.data_ptr(),
                                             emb.data_ptr(), _stream_ptr(dev))
    assert st == 0, qa_lib.qa_last_error()
    check_guarded_out(ebuf, emb, 4)
    assert bool((cbuf[:8] == CODE_GUARD).all()) and bool((cbuf[-8:] == CODE_GUARD).all()) and not bool((ac == CODE_GUARD + 1).any())
    return ac.view(B, Q, n).clone(), emb.contiguous().view(B, n, D).clone()


@functools.lru_cache(maxsize=None)
def _run(qa_lib, dev, short_attn):
    """The whole schedule once per value of QA_TR_SHORT_ATTN: per step (codes, emb), and the offsets seen after every step."""
    c = _case(dev)
    codec, ospec = c["codec"], c["ospec"]
    steps, offsets = [], []
    with with_knob("QA_TR_SHORT_ATTN", short_attn):
        with codec.streaming(4, max_frames=MAX_FRAMES):
            assert codec.streaming_offsets == [0, 0, 0, 0]
            for s, (x, fr) in enumerate(c["rect"]):
                if s in RR.RESETS:
                    codec.reset_streaming(rows=list(RR.RESETS[s]))
                    assert all(codec.streaming_offsets[b] == 0 for b in RR.RESETS[s])
                steps.append(_step_guarded(qa_lib, codec, ospec, x, fr, dev))
                offsets.append(codec.streaming_offsets)
                assert codec.streaming_offset == max(offsets[-1])
    return steps, offsets


def _segment_outputs(steps, b, seg_steps):
    ac = torch.cat([steps[s][0][b:b + 1, :, :n] for s, n in seg_steps], 2)
    emb = torch.cat([steps[s][1][b:b + 1, :n] for s, n in seg_steps], 1)
    return ac, emb


@pytest.mark.parametrize("short_attn", [1, 0, 2])
def test_every_row_equals_its_own_offline_encode(qa_lib, gpu_device, short_attn):
    """(1) parity per row and segment against the oracle; (2) the tails: NaN behind every row's samples, -1 / 0 behind its frames."""
    c = _case(gpu_device)
    steps, offsets = _run(qa_lib, gpu_device, short_attn)
    want_off = [0, 0, 0, 0]
    for s, fr in enumerate(RR.SCHEDULE):
        want_off = [0 if b in RR.RESETS.get(s, ()) else o for b, o in enumerate(want_off)]
        want_off = [o + f for o, f in zip(want_off, fr)]
        assert offsets[s] == want_off, (s, offsets[s], want_off)
        ac, emb = steps[s]
        assert torch.isfinite(emb).all()
        for b, f in enumerate(fr):
            assert bool((ac[b, :, f:] == -1).all()) and bool((emb[b, f:] == 0).all()), (s, b)
            assert bool((ac[b, :, :f] >= 0).all()) and bool((ac[b, :, :f] < c["ospec"].codebook_size).all()), (s, b)
    differing = 0
    for (b, seg_steps), (emb_o, ac_o) in zip(c["segs"], c["oracle"]):
        ac, emb = _segment_outputs(steps, b, seg_steps)
        e = rel_err(emb, emb_o.transpose(1, 2))
        diff = int((ac.cpu() != ac_o).sum())
        differing += diff
        print(f"QA_TR_SHORT_ATTN={short_attn} row {b} ({ac.shape[-1]} frames in {len(seg_steps)} steps): emb against the oracle {e:.2e}, "
              f"{diff} of {ac.numel()} codes differ")
        assert e <= STAGE_TOL
        audit_codes_bnq(emb_o, c["cb"], ac, ac_o, rel_tol=CODE_TIE_TOL)
    # no decision of the oracle is a near-tie for these seeds (tests/test_hcodec_stream_rows_cpu.py)
    assert differing == 0


@pytest.mark.parametrize("short_attn", [1, 0, 2])
def test_delayed_duplicate_is_bit_for_bit(qa_lib, gpu_device, short_attn):
    """(3) rows 0 and 1 consume the same chunks in rectangles of the same width, three steps apart: nothing a row computes depends on its
    neighbours' offsets or on which state buffer is current.  (The caches here hold 32 Transformer rows, one key split in every step:
    independence from the split count is pinned by test_transformer_rows_across_key_splits.)"""
    steps, _ = _run(qa_lib, gpu_device, short_attn)
    for s in range(4):
        n = RR.SCHEDULE[s][0]
        assert steps[s][1].shape == steps[s + RR.DELAY][1].shape and n == RR.SCHEDULE[s + RR.DELAY][1]
        assert torch.equal(steps[s + RR.DELAY][1][1, :n], steps[s][1][0, :n]), f"emb of row 1 at step {s + RR.DELAY} != row 0 at step {s}"
        assert torch.equal(steps[s + RR.DELAY][0][1, :, :n], steps[s][0][0, :, :n]), f"codes of row 1 at step {s + RR.DELAY}"


def test_rows_call_with_full_lengths_is_the_rectangular_step(qa_lib, gpu_device):
    """(4a) every row at one offset with all its frames: the bits of encode_stream without lengths, over a (2, 1, 5) chunking."""
    c = _case(gpu_device)
    codec, hop = c["codec"], c["ospec"].enc_hop
    wav = synth.synth_wav(71, 4, 8 * hop).unsqueeze(1).to(gpu_device)
    outs = []
    for lengths in (False, True):
        with codec.streaming(4, max_frames=MAX_FRAMES):
            t, acs, embs = 0, [], []
            for n in (2, 1, 5):
                ac, emb = codec.encode_stream(wav[..., t * hop:(t + n) * hop], return_emb=True, lengths=[n] * 4 if lengths else None)
                acs.append(ac)
                embs.append(emb)
                t += n
                assert codec.streaming_offsets == [t] * 4 and codec.streaming_offset == t
            outs.append((torch.cat(acs, 2), torch.cat(embs, 1)))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_an_idle_step_leaves_a_row_untouched(qa_lib, gpu_device):
    """(4b) row 1's next step after a step it idled in equals, bit for bit, the step it takes when that step never happened.  Both runs
    are ragged (row 3 starts late), so both take the per-row launches."""
    c = _case(gpu_device)
    codec, hop = c["codec"], c["ospec"].enc_hop
    wav = synth.synth_wav(72, 4, 6 * hop).unsqueeze(1).to(gpu_device)

    def x(t0, n):
        return wav[..., t0 * hop:(t0 + n) * hop].contiguous()

    with codec.streaming(4, max_frames=MAX_FRAMES):
        codec.encode_stream(x(0, 2), lengths=[2, 2, 2, 0])
        codec.encode_stream(x(2, 2), lengths=[1, 1, 1, 2])
        codec.encode_stream(x(3, 1), lengths=[1, 0, 1, 1])  # row 1 idles
        assert codec.streaming_offsets == [4, 3, 4, 3]
        ac_a, emb_a = codec.encode_stream(x(3, 2), return_emb=True, lengths=[2, 2, 2, 2])
    with codec.streaming(4, max_frames=MAX_FRAMES):
        codec.encode_stream(x(0, 2), lengths=[2, 2, 2, 0])
        codec.encode_stream(x(2, 2), lengths=[1, 1, 1, 2])
        ac_b, emb_b = codec.encode_stream(x(3, 2), return_emb=True, lengths=[0, 2, 0, 0])
        assert codec.streaming_offsets == [3, 5, 3, 2]
    assert torch.equal(emb_a[1], emb_b[1]) and torch.equal(ac_a[1], ac_b[1])
    assert bool((emb_b[0] == 0).all()) and bool((ac_b[2] == -1).all())


def test_refusals_leave_every_offset_and_the_state_as_they_were(qa_lib, gpu_device):
    """(8) every refusal comes before a launch: the offsets stay, and the following step reproduces an undisturbed run bit for bit."""
    import unified_audio_amd as qa

    c = _case(gpu_device)
    codec, ospec = c["codec"], c["ospec"]
    (x0, fr0), (x1, fr1) = c["rect"][0], c["rect"][1]
    with codec.streaming(4, max_frames=5):
        codec.encode_stream(x0, lengths=fr0)
        want = codec.encode_stream(x1, return_emb=True, lengths=fr1)
    with codec.streaming(4, max_frames=5):
        with pytest.raises(qa.QuarkAudioError, match="every row idles"):
            codec.encode_stream(x0, lengths=[0, 0, 0, 0])
        with pytest.raises(qa.QuarkAudioError, match="row 1 starts its stream with 1 code frames"):
            codec.encode_stream(x0, lengths=[2, 1, 3, 0])
        assert codec.streaming_offsets == [0, 0, 0, 0]
        codec.encode_stream(x0, lengths=fr0)
        off = codec.streaming_offsets
        assert off == [2, 0, 3, 0]
        for lengths, word in (([2, 0, 4, 2], r"frames\[2\] = 4 is outside 0 .. 3"),   # beyond the rectangle (x1 holds 3 frames)
                              ([2, -1, 1, 2], r"frames\[1\] = -1"),
                              ([2, 1, 1, 2], "row 1 starts its stream with 1"),        # a first chunk below the minimum
                              ([2, 0, 1], "entries for a batch of 4")):
            with pytest.raises(qa.QuarkAudioError, match=word):
                codec.encode_stream(x1, lengths=lengths)
            assert codec.streaming_offsets == off
        with pytest.raises(qa.QuarkAudioError, match="row 2 has 3 streamed \\+ 3 new code frames, beyond the capacity 5"):
            codec.encode_stream(x1, lengths=[2, 0, 3, 2])
        with pytest.raises(qa.QuarkAudioError, match="capacity"):  # the call without lengths on rows at different offsets: 3 frames each
            codec.encode_stream(torch.nan_to_num(x1))
        for rows, word in (([4], "outside 0 .. 3"), ([-1], "outside 0 .. 3"), ([2, 2], "named twice"), ([], "rows to reset")):
            with pytest.raises(qa.QuarkAudioError, match=word):
                codec.reset_streaming(rows=rows)
        assert codec.streaming_offsets == off and codec.streaming_offset == 3
        side = torch.cuda.Stream(gpu_device)
        side.wait_stream(torch.cuda.current_stream(gpu_device))
        graph = torch.cuda.CUDAGraph()
        with pytest.raises(qa.QuarkAudioError, match="stream capture"):
            with torch.cuda.graph(graph, stream=side):
                codec.encode_stream(x1, lengths=fr1)
        torch.cuda.synchronize()
        assert codec.streaming_offsets == off
        got = codec.encode_stream(x1, return_emb=True, lengths=fr1)
        assert codec.streaming_offsets == [4, 0, 4, 2]
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    # handles without a stream are refused as before
    with pytest.raises(qa.QuarkAudioError, match="not streaming"):
        codec.encode_stream(x1, lengths=fr1)
    nc = qa.Codec(None, None, None, spec=qa.HCodecSpec(**MINI), device=gpu_device).load_state_dict(c["sd"])
    with pytest.raises(qa.QuarkAudioError, match="causal"):
        nc.streaming_forever(4)
    with pytest.raises(qa.QuarkAudioError, match="not streaming"):
        nc.encode_stream(x1, lengths=fr1)


def test_handles_that_cannot_stream_refuse_the_rows_calls(qa_lib, gpu_device):
    """(8) an H-Codec 1.5 and an H-Codec 2.0 handle cannot begin a stream (status -4, as before), so the three new calls find none."""
    import unified_audio_amd as qa
    from tests import hcodec20_ragged_cases as K
    from tests.test_hcodec15_ragged_gpu import _mini15

    c15 = _mini15(gpu_device)[2]
    c20 = qa.Codec(None, None, None, spec=K.product_spec(K.SMALL, True), device=gpu_device).load_state_dict(synth.hcodec20_state_dict(5, K.SMALL))
    x = torch.zeros(2, 2 * K.HOP, device=gpu_device)
    ac = torch.empty(2, 8, 2, dtype=torch.int64, device=gpu_device)
    frames, rows, out = (C.c_int64 * 2)(2, 2), (C.c_int64 * 1)(0), (C.c_int64 * 2)(7, 7)
    for codec, word in ((c15, "1.5"), (c20, "2.0")):
        with pytest.raises(qa.QuarkAudioError, match=word) as e:
            codec.streaming_forever(2)
        assert e.value.status == -4 and not codec.is_streaming
        assert qa_lib.qa_hcodec_stream_encode_rows(codec._handle, x.data_ptr(), x.shape[1], frames, ac.data_ptr(), None, _stream_ptr(gpu_device)) != 0
        assert b"not streaming" in qa_lib.qa_last_error()
        assert qa_lib.qa_hcodec_stream_reset_rows(codec._handle, rows, 1) != 0 and b"not streaming" in qa_lib.qa_last_error()
        assert qa_lib.qa_hcodec_stream_offsets(codec._handle, out) != 0 and list(out) == [7, 7]
        with pytest.raises(qa.QuarkAudioError, match="not streaming"):
            codec.encode_stream(x, lengths=[2, 2])


# ------------------------------------------------------------------------------------------------ (6) block level
TR_SCHEDULE = ((3, 0, 2), (1, 0, 5), (2, 4, 0), (1, 1, 3), (5, 2, 1), (0, 3, 2))  # frames per step, rows 0 - 2; row 0 ends at 12 = max_frames
TR_RESETS = {3: (2,)}
TR_CAP = 12


@functools.lru_cache(maxsize=None)
def _tr_case(left_context):
    """Per segment: its input [1, T, d], the fp64 offline truth and the bound 4 max(e_cpu32, 1e-6) of tests/test_transformer_stream_gpu.py."""
    hidden, heads, layers = 128, 2, 2
    sd = TR.random_state_dict(31, hidden, 2 * hidden, layers)
    segs = RR.segments(TR_SCHEDULE, TR_RESETS)
    g = torch.Generator().manual_seed(77)
    out = []
    for b, steps in segs:
        x = torch.randn(1, sum(n for _, n in steps), hidden, generator=g)
        y64 = TR.forward(sd, x.double(), layers, heads, True, left_context)
        e32 = TR.rel_err(TR.forward(sd, x, layers, heads, True, left_context), y64)
        out.append(dict(row=b, steps=steps, x=x, y64=y64, e32=e32, bound=4 * max(e32, 1e-6)))
    return sd, out


@pytest.mark.parametrize("short_attn", [1, 0])
@pytest.mark.parametrize("left_context", [0, 5], ids=["full", "window5"])
def test_transformer_rows_against_the_fp64_restatement(gpu_device, short_attn, left_context):
    import unified_audio_amd as qa
    from tests.test_transformer_stream_gpu import build

    sd, segs = _tr_case(left_context)
    m = build(gpu_device, 128, 2, 2, True, left_context, sd)
    B, d = 3, 128
    rect = [torch.full((B, max(fr), d), float("nan")) for fr in TR_SCHEDULE]
    for c in segs:
        t = 0
        for s, n in c["steps"]:
            rect[s][c["row"], :n] = c["x"][0, t:t + n]
            t += n
    ys = []
    with with_knob("QA_TR_SHORT_ATTN", short_attn):
        with m.streaming(B, max_frames=TR_CAP):
            if left_context and not short_attn:  # the long-chunk attention has no per-item form under a window: refused, nothing moves
                with pytest.raises(qa.QuarkAudioError, match="sliding window"):
                    m(rect[0].to(gpu_device), lengths=list(TR_SCHEDULE[0]))
                assert m.streaming_offsets == [0, 0, 0]
                return
            for s, fr in enumerate(TR_SCHEDULE):
                if s in TR_RESETS:
                    m.reset_streaming(rows=list(TR_RESETS[s]))
                y = m(rect[s].to(gpu_device), lengths=list(fr))
                assert torch.isfinite(y).all() and all(bool((y[b, f:] == 0).all()) for b, f in enumerate(fr))
                ys.append(y.cpu())
            off = m.streaming_offsets
            assert off == [12, 10, 6] and m.streaming_offset == 12  # row 0 sits at max_frames exactly, the others went on
            with pytest.raises(qa.QuarkAudioError, match="row 0 has 12 streamed \\+ 1 new frames, beyond the capacity 12"):
                m(rect[0][:, :1].to(gpu_device), lengths=[1, 1, 1])
            with pytest.raises(qa.QuarkAudioError, match="every row idles"):
                m(rect[0][:, :1].to(gpu_device), lengths=[0, 0, 0])
            for lengths, word in (([0, 2, 1], r"frames\[1\] = 2 is outside 0 .. 1"), ([0, 1, -1], r"frames\[2\] = -1"),
                                  ([0, 1], "entries for a batch of 3")):
                with pytest.raises(qa.QuarkAudioError, match=word):
                    m(rect[0][:, :1].to(gpu_device), lengths=lengths)
            for rows, word in (([1, 1], "named twice"), ([3], "outside 0 .. 2"), ([-1], "outside 0 .. 2"), ([], "rows to reset")):
                with pytest.raises(qa.QuarkAudioError, match=word):
                    m.reset_streaming(rows=rows)
            side = torch.cuda.Stream(gpu_device)
            side.wait_stream(torch.cuda.current_stream(gpu_device))
            graph, x_dev = torch.cuda.CUDAGraph(), rect[0][:, :1].to(gpu_device)
            with pytest.raises(qa.QuarkAudioError, match="stream capture"):
                with torch.cuda.graph(graph, stream=side):
                    m(x_dev, lengths=[0, 1, 1])
            torch.cuda.synchronize()
            assert m.streaming_offsets == off
            # ... and the step behind the refusals is the step of a stream that never met them
            y_after = m(torch.nan_to_num(rect[0][:, :1]).to(gpu_device), lengths=[0, 1, 1])
            assert m.streaming_offsets == [12, 11, 7] and bool((y_after[0] == 0).all()) and torch.isfinite(y_after).all()
    for c in segs:
        y = torch.cat([ys[s][c["row"]:c["row"] + 1, :n] for s, n in c["steps"]], 1)
        e = TR.rel_err(y, c["y64"])
        x = c["x"].to(gpu_device)
        e_off = TR.rel_err(m(x).cpu(), c["y64"])
        bound = c["bound"] if e_off <= c["bound"] else 2 * e_off
        print(f"QA_TR_SHORT_ATTN={short_attn} left_context={left_context} row {c['row']} steps {c['steps']}: e {e:.2e}  e_cpu32 {c['e32']:.2e}  "
              f"e_offline {e_off:.2e}  bound {bound:.2e}")
        assert e <= bound


# ------------------------------------------------------------------------------------------------ (6b) more than one key split
# The short attention splits a row's keys into fixed ranges of L = attn_short_split_keys(capacity) >= 64 keys; the grid has
# ceil(max_b(keys) / L) splits.  The cases above hold at most 32 keys, one split.  Here capacity 208 gives L = 64 and the rows sit on
# both sides of key 64 and key 128: frames per step for rows 0 - 3, every rectangle 16 frames wide, QA_TR_SHORT_ATTN = 2.
#   row 0   16 per step: 160 keys in the end, splits 1 / 2 / 3 from steps 0 / 4 / 8 on
#   row 1   row 0's input, four steps late: at step s + 4 it consumes the chunk row 0 consumed at step s (s = 0 .. 3) - in a grid of 2
#           splits where row 0 had 1, its second split wholly behind its keys; then 5 and 3 frames across key 64 in a grid of 3
#   row 2   joins at step 8: 7 + 4 frames, about 10 keys beside rows at about 70 and about 140
#   row 3   3 frames at step 0, idle for eight steps, 2 frames at step 9
SPLIT_CAP = 208
SPLIT_SCHEDULE = tuple((16, 16 if 4 <= s < 8 else (5, 3)[s - 8] if s >= 8 else 0, (7, 4)[s - 8] if s >= 8 else 0, 3 if s == 0 else 2 if s == 9 else 0)
                       for s in range(10))
SPLIT_DELAY = 4


@functools.lru_cache(maxsize=None)
def _split_case():
    hidden, heads, layers = 128, 2, 2
    sd = TR.random_state_dict(31, hidden, 2 * hidden, layers)
    segs = RR.segments(SPLIT_SCHEDULE, {})
    g = torch.Generator().manual_seed(78)
    out = []
    for b, steps in segs:
        T = sum(n for _, n in steps)
        x = out[0]["x"][:, :T].clone() if b == 1 else torch.randn(1, T, hidden, generator=g)
        y64 = TR.forward(sd, x.double(), layers, heads, True, 0)
        e32 = TR.rel_err(TR.forward(sd, x, layers, heads, True, 0), y64)
        out.append(dict(row=b, steps=steps, x=x, y64=y64, e32=e32, bound=4 * max(e32, 1e-6)))
    return sd, out


def test_transformer_rows_across_key_splits(qa_lib, gpu_device):
    from tests.test_transformer_stream_gpu import build

    assert [sum(fr[b] for fr in SPLIT_SCHEDULE) for b in range(4)] == [160, 72, 11, 5]
    sd, segs = _split_case()
    m = build(gpu_device, 128, 2, 2, True, 0, sd)
    B, d, W = 4, 128, 16
    rect = [torch.full((B, W, d), float("nan")) for _ in SPLIT_SCHEDULE]
    for c in segs:
        t = 0
        for s, n in c["steps"]:
            rect[s][c["row"], :n] = c["x"][0, t:t + n]
            t += n
    ys, keys = [], [0] * B
    with with_knob("QA_TR_SHORT_ATTN", 2):
        with m.streaming(B, max_frames=SPLIT_CAP):
            for s, fr in enumerate(SPLIT_SCHEDULE):
                y = m(rect[s].to(gpu_device), lengths=list(fr))
                keys = [k + f for k, f in zip(keys, fr)]
                assert m.streaming_offsets == keys
                assert torch.isfinite(y).all() and all(bool((y[b, f:] == 0).all()) for b, f in enumerate(fr))
                ys.append(y.cpu())
    # the splits of the grids, from the capacity as the library derives them: 16 splits of whole 64-key steps, 64 .. 256 keys each
    L = min(256, max(64, -(-(-(-SPLIT_CAP // 16)) // 64) * 64))
    ns = [-(-16 * (s + 1) // L) for s in range(10)]
    assert L == 64 and ns == [1, 1, 1, 1, 2, 2, 2, 2, 3, 3]
    for c in segs:
        y = torch.cat([ys[s][c["row"]:c["row"] + 1, :n] for s, n in c["steps"]], 1)
        e = TR.rel_err(y, c["y64"])
        e_off = TR.rel_err(m(c["x"].to(gpu_device)).cpu(), c["y64"])
        bound = c["bound"] if e_off <= c["bound"] else 2 * e_off
        print(f"key splits: row {c['row']} ({c['x'].shape[1]} frames in {len(c['steps'])} steps): e {e:.2e}  e_cpu32 {c['e32']:.2e}  "
              f"e_offline {e_off:.2e}  bound {bound:.2e}")
        assert e <= bound
    # the delayed duplicate, bit for bit, across DIFFERENT split counts: row 1 in a grid of 2 splits against row 0 in a grid of 1
    for s in range(4):
        assert ns[s] != ns[s + SPLIT_DELAY] and SPLIT_SCHEDULE[s][0] == SPLIT_SCHEDULE[s + SPLIT_DELAY][1] == 16
        assert torch.equal(ys[s + SPLIT_DELAY][1], ys[s][0]), f"row 1 at step {s + SPLIT_DELAY} (ns {ns[s + SPLIT_DELAY]}) != row 0 at step {s} (ns {ns[s]})"


# ------------------------------------------------------------------------------------------------ (7) the kernels directly
def _window_rows_ref(state, chunk, ctx, n_rows, first):
    B, n, Cc = chunk.shape
    win = torch.zeros(B, ctx + n, Cc)
    sout = torch.empty(B, ctx, Cc)
    for b in range(B):
        nb = n_rows[b]
        win[b, :ctx] = chunk[b, 1:ctx + 1].flip(0) if first[b] else state[b]
        win[b, ctx:ctx + nb] = chunk[b, :nb]
        sout[b] = win[b, nb:nb + ctx]
    return win, sout


@pytest.mark.parametrize("Cc", [1, 32, 132])
def test_stream_window_rows_kernel_is_copies_and_zeros(qa_lib, gpu_device, Cc):
    """qa_debug_stream_window_rows against a torch restatement, by equality, outputs between sentinels, the chunk NaN behind every row's
    length.  One row per length in {0, 1, ctx - 1, ctx, n} (those that fit), first flags where the row is long enough to reflect."""
    g = torch.Generator().manual_seed(200 + Cc)
    stream = _stream_ptr(gpu_device)
    for ctx in (2, 6):
        for n in sorted({1, ctx - 1, ctx + 1, 9}):
            n_rows = sorted({v for v in (0, 1, ctx - 1, ctx, n) if v <= n}) + [n]
            B = len(n_rows)
            first = [int(v > ctx and i % 2 == 0) for i, v in enumerate(n_rows)]
            if n > ctx:
                first[-1] = 1
            for head in ((0, 1) if Cc == 132 else (0,)):  # head 1: unaligned buffers take the scalar path
                state = torch.randn(B, ctx, Cc, generator=g)
                chunk = torch.randn(B, n, Cc, generator=g)
                dirty = chunk.clone()
                for b, nb in enumerate(n_rows):
                    dirty[b, nb:] = float("nan")
                wbuf, win = guarded_out(B * (ctx + n), Cc, Cc, head, gpu_device)
                sbuf, sout = guarded_out(B * ctx, Cc, Cc, head, gpu_device)
                nd = torch.tensor(n_rows, dtype=torch.int32, device=gpu_device)
                fd = torch.tensor(first, dtype=torch.int32, device=gpu_device)
                sd_, cd = state.to(gpu_device), dirty.to(gpu_device)
                st = qa_lib.qa_debug_stream_window_rows(sd_.data_ptr(), cd.data_ptr(), win.data_ptr(), sout.data_ptr(), B, ctx, n, Cc,
                                                        nd.data_ptr(), fd.data_ptr(), stream)
                assert st == 0, (ctx, n, qa_lib.qa_last_error())
                check_guarded_out(wbuf, win, head)
                check_guarded_out(sbuf, sout, head)
                want_win, want_state = _window_rows_ref(state, chunk, ctx, n_rows, first)
                assert torch.equal(win.cpu().view(B, ctx + n, Cc), want_win), (ctx, n, n_rows, first, head)
                assert torch.equal(sout.cpu().view(B, ctx, Cc), want_state), (ctx, n, n_rows, first, head)
    # updating the state in place is refused, not raced
    state = torch.randn(2, 6, Cc).to(gpu_device)
    chunk = torch.randn(2, 2, Cc).to(gpu_device)
    win = torch.empty(2, 8, Cc, device=gpu_device)
    z = torch.zeros(2, dtype=torch.int32, device=gpu_device)
    assert qa_lib.qa_debug_stream_window_rows(state.data_ptr(), chunk.data_ptr(), win.data_ptr(), state.data_ptr(), 2, 6, 2, Cc, z.data_ptr(),
                                              z.data_ptr(), stream) != 0


def test_lstm_carry_rows_equals_the_carried_chunk_of_each_row_alone(qa_lib, gpu_device):
    """d = 512, B = 5, T = 4, nq = [4, 0, 1, 3, 4], row 3 zero-started: each row equals qa_debug_lstm_carry on that row's first nq steps
    alone, bit for bit; the nq = 0 row's (h, c) are bit-unchanged."""
    d, B, T = 512, 5, 4
    nq, zero = [4, 0, 1, 3, 4], [0, 0, 0, 1, 0]
    g = torch.Generator().manual_seed(5)
    xw = (torch.randn(B, T, 4 * d, generator=g) * 0.5).to(gpu_device)
    w = (torch.randn(4 * d, d, generator=g) / d ** 0.5).to(gpu_device)
    h0 = (torch.randn(B, d, generator=g) * 0.3).to(gpu_device)
    c0 = (torch.randn(B, d, generator=g) * 0.3).to(gpu_device)
    stream = _stream_ptr(gpu_device)
    h, c, out = h0.clone(), c0.clone(), torch.full((B, T, d), float("nan"), device=gpu_device)
    nd = torch.tensor(nq, dtype=torch.int32, device=gpu_device)
    zd = torch.tensor(zero, dtype=torch.int32, device=gpu_device)
    st = qa_lib.qa_debug_lstm_carry_rows(xw.data_ptr(), w.data_ptr(), out.data_ptr(), h.data_ptr(), c.data_ptr(), B, T, d, nd.data_ptr(),
                                         zd.data_ptr(), stream)
    assert st == 0, qa_lib.qa_last_error()
    for b in range(B):
        if nq[b] == 0:
            assert torch.equal(h[b], h0[b]) and torch.equal(c[b], c0[b])
            continue
        xb = xw[b:b + 1, :nq[b]].contiguous()
        hb = torch.zeros(1, d, device=gpu_device) if zero[b] else h0[b:b + 1].clone()
        cb = torch.zeros(1, d, device=gpu_device) if zero[b] else c0[b:b + 1].clone()
        ob = torch.empty(1, nq[b], d, device=gpu_device)
        assert qa_lib.qa_debug_lstm_carry(xb.data_ptr(), w.data_ptr(), ob.data_ptr(), hb.data_ptr(), cb.data_ptr(), 1, nq[b], d, stream) == 0
        assert torch.equal(out[b, :nq[b]], ob[0]) and torch.equal(h[b], hb[0]) and torch.equal(c[b], cb[0]), b
        assert torch.isfinite(out[b]).all()
