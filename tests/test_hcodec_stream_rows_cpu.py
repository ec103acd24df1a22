"""Per-row lengths, offsets and resets of the H-Codec 1.0 stream without a GPU: the per-row schedule driver
(tests/hcodec_stream_rows_ref.py) against the offline causal restatement in fp64, the new C-ABI on a null handle, and the near-tie
condition of the seeds that tests/test_hcodec_stream_rows_gpu.py compares codes with."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import hcodec_ref as R
from oracle import rvq_c
from tests import hcodec_stream_ref as S
from tests import hcodec_stream_rows_ref as RR
from tests import transformer_stream_ref as TR
from tests.util import CODE_TIE_TOL, MINI

CAUSAL_MINI = dict(MINI, causal=True)


def test_schedule_is_the_one_the_gpu_test_documents():
    segs = RR.segments()
    assert [(b, sum(f for _, f in st)) for b, st in segs] == [(0, 14), (1, 10), (2, 6), (2, 5), (3, 9)]
    assert segs[2][1] == [(0, 3), (1, 1), (3, 2)] and segs[3][1][0] == (4, 2)  # row 2 idles in step 2 and is first again in step 4
    # rows 0 and 1: the same chunks in rectangles of the same width, DELAY steps apart
    for s in range(4):
        assert RR.SCHEDULE[s][0] == RR.SCHEDULE[s + RR.DELAY][1] and max(RR.SCHEDULE[s]) >= 2
    ospec, _, segs, waves = RR.case_inputs(RR.GPU_ROWS_CASE, CAUSAL_MINI)
    assert torch.equal(waves[1], waves[0][..., :waves[1].shape[-1]]) and not torch.equal(waves[2][..., :64], waves[0][..., :64])
    rect = RR.rectangles(ospec, segs, waves)
    assert [x.shape[-1] // ospec.enc_hop for x, _ in rect] == [3] * 8  # one width: steps s and s + DELAY are the same rectangle shape
    x6, len6 = rect[6]
    assert len6 == [1, 2, 1, 3] and torch.isnan(x6[0, 0, ospec.enc_hop:]).all() and torch.isfinite(x6[3]).all()
    # every first chunk of a segment meets the first-chunk minimum
    assert all(st[0][1] >= S.first_min_frames(ospec) for _, st in segs)


def test_every_row_of_the_schedule_equals_its_own_offline_encode_in_fp64():
    ospec, sd, segs, waves = RR.case_inputs(RR.GPU_ROWS_CASE, CAUSAL_MINI)
    got = RR.run_schedule(sd, ospec, segs, waves, torch.float64)
    for (b, steps), wav, y in zip(segs, waves, got):
        n = wav.shape[-1] // ospec.enc_hop
        y64 = S.stream(sd, wav, ospec, (n,), dtype=torch.float64)
        e = TR.rel_err(y, y64)
        print(f"row {b}, steps {steps}: {e:.2e}")
        assert y.shape == y64.shape == (1, ospec.dimension, n) and e < 1e-12


def test_new_symbols_refuse_a_null_handle(qa_lib):
    import unified_audio_amd as qa

    frames, rows, out = (C.c_int64 * 4)(1, 1, 1, 1), (C.c_int64 * 1)(0), (C.c_int64 * 4)()
    assert qa_lib.qa_hcodec_stream_encode_rows(None, None, 640, frames, None, None, None) != 0
    assert qa_lib.qa_hcodec_stream_reset_rows(None, rows, 1) != 0
    assert qa_lib.qa_hcodec_stream_offsets(None, out) != 0
    assert qa_lib.qa_transformer_stream_step_rows(None, None, 1, frames, None, None) != 0
    assert qa_lib.qa_transformer_stream_reset_rows(None, rows, 1) != 0
    assert qa_lib.qa_transformer_stream_offsets(None, out) != 0
    assert qa_lib.qa_debug_stream_window_rows(None, None, None, None, 1, 2, 1, 1, None, None, None) != 0
    assert qa_lib.qa_debug_lstm_carry_rows(None, None, None, None, None, 1, 1, 512, None, None, None) != 0
    assert qa_lib.qa_last_error()
    codec = qa.Codec(spec=qa.HCodecSpec(**CAUSAL_MINI))
    with pytest.raises(qa.QuarkAudioError, match="not streaming"):
        codec.encode_stream(torch.zeros(1, 1, 32), lengths=[2])
    with pytest.raises(qa.QuarkAudioError):
        codec.reset_streaming(rows=[0])
    with pytest.raises(qa.QuarkAudioError, match="not streaming"):
        codec.streaming_offsets


def test_gpu_code_cases_have_no_near_tie():
    """tests/test_hcodec_stream_rows_gpu.py expects EQUAL codes against the oracle on every segment: fair only where no decision of the
    oracle's own RVQ is a near-tie, as tests/test_hcodec_stream_cpu.py asserts for the rectangular stream's seeds."""
    ospec, sd, segs, waves = RR.case_inputs(RR.GPU_ROWS_CASE, CAUSAL_MINI)
    cb = R.rvq_codebooks(sd, "quantizer", ospec.num_quantizers).numpy()
    for (b, _), wav in zip(segs, waves):
        emb, ac = S.oracle_emb_and_codes(sd, wav, ospec)
        _, D, N = emb.shape
        x = emb.transpose(1, 2).reshape(N, D).numpy()
        got = ac.transpose(1, 2).reshape(N, -1).numpy()
        excess, best, gap = rvq_c.check_f64(x, cb, got)
        tol = CODE_TIE_TOL * float((x.astype(np.float64) ** 2).sum(1).mean())
        print(f"row {b}, {N} frames: smallest decision gap {gap.min():.3e} against {tol:.3e}")
        assert (got == best).all() and gap.min() > tol
