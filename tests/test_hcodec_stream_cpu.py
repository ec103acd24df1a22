"""The chunked causal H-Codec 1.0 encoder without a GPU: the streaming restatement (tests/hcodec_stream_ref.py) against
the oracle and against itself over chunkings, the library's host-side geometry against the restatement's, the C-ABI on a null handle,
and the near-tie condition of the seeds that tests/test_hcodec_stream_gpu.py compares codes with."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import hcodec_ref as R
from oracle import rvq_c
from tests import hcodec_stream_ref as S
from tests import transformer_stream_ref as TR
from tests.util import CODE_TIE_TOL, MINI

CAUSAL_MINI = dict(MINI, causal=True)


def _mini(B, frames=S.FRAMES, seed=11, wav_seed=31):
    return S.case_inputs(dict(seed=seed, wav_seed=wav_seed, B=B, frames=frames), CAUSAL_MINI)


def test_offline_fp32_equals_the_oracle():
    """One chunk of the whole length is the offline causal forward.  Every convolution of the restatement issues the call the oracle issues
    on the tensor the oracle builds, so with the oracle's own Transformer in the middle the whole encoder equals R.seanet_encoder BIT FOR
    BIT, every stage tap included.  With the restatement's dtype-following block (its own LSTM loop where the oracle runs nn.LSTM) the
    convolution ladder in front of the block still equals it bit for bit, and the embedding agrees to the rounding the two LSTM
    evaluations differ by - the relation tests/test_transformer_stream_cpu.py::test_offline_fp32_equals_the_oracle holds the block to."""
    ospec, sd, wav = _mini(2)
    t_or, t_a, t_b = {}, {}, {}
    y_or = R.seanet_encoder(sd, wav, ospec, t_or)
    tp = f"encoder.model.{3 * len(ospec.ratios) + 2}"
    y_a = S.stream(sd, wav, ospec, (S.FRAMES,), block=lambda x: R.transformer(sd, tp, x, ospec.enc_layers, ospec.enc_heads, None, True),
                   taps=t_a)
    assert torch.equal(y_a, y_or)
    for name in ["enc.conv0", "enc.transformer"] + [f"enc.stage{i}" for i in range(len(ospec.ratios))]:
        assert torch.equal(t_a[name], t_or[name]), name
    y_b = S.stream(sd, wav, ospec, (S.FRAMES,), taps=t_b)
    for name in ["enc.conv0"] + [f"enc.stage{i}" for i in range(len(ospec.ratios))]:
        assert torch.equal(t_b[name], t_or[name]), name
    y64 = S.stream(sd, wav, ospec, (S.FRAMES,), dtype=torch.float64)
    e_or, e_b = TR.rel_err(y_or, y64), TR.rel_err(y_b, y64)
    print(f"fp32 offline against fp64: oracle {e_or:.2e}, restatement {e_b:.2e}")
    assert e_or < 1e-5 and e_b <= 4 * max(e_or, 1e-6)


@pytest.mark.parametrize("name", list(S.CHUNKINGS))
def test_every_chunking_equals_offline_causal_in_fp64(name):
    ospec, sd, wav = _mini(2)
    y64 = S.stream(sd, wav, ospec, (S.FRAMES,), dtype=torch.float64)
    y = S.stream(sd, wav, ospec, S.CHUNKINGS[name], dtype=torch.float64)
    e = TR.rel_err(y, y64)
    print(f"{name}: {e:.2e}")
    assert y.shape == y64.shape == (2, ospec.dimension, S.FRAMES) and e < 1e-12


def test_one_frame_first_chunk_is_another_function():
    """Why the library refuses it: a first chunk of one code frame hands the out conv 2 Transformer frames for a context of 2, the offline
    graph then pads by pad1d's short-input rule, and the whole utterance reflects a frame the chunk does not have yet."""
    ospec, sd, wav = _mini(2)
    assert S.first_min_frames(ospec) == 2
    y64 = S.stream(sd, wav, ospec, (S.FRAMES,), dtype=torch.float64)
    y = S.stream(sd, wav, ospec, (1,) * S.FRAMES, dtype=torch.float64)
    e0, e_rest = TR.rel_err(y[..., :1], y64[..., :1]), TR.rel_err(y[..., 1:], y64[..., 1:])
    print(f"first chunk of one frame: code frame 0 off by {e0:.2e}, the frames behind it by {e_rest:.2e}")
    # the out conv sits behind the Transformer, so for this geometry the wrong padding stays in code frame 0
    assert e0 > 1e-3 and e_rest < 1e-12


def _geometry(qa_lib, spec):
    samples, first, n = C.c_int64(), C.c_int64(), C.c_int32()
    ctx = (C.c_int32 * 32)()
    spec_c = spec.to_c()
    st = qa_lib.qa_hcodec_stream_geometry(C.byref(spec_c), C.byref(samples), C.byref(first), ctx, 32, C.byref(n))
    return st, samples.value, first.value, list(ctx[: n.value])


def test_geometry_equals_the_restatements(qa_lib):
    import unified_audio_amd as qa

    shipped = dict(n_filters=32, ratios=(2, 4, 5, 8), dimension=512)
    for kw, want_ctx in ((CAUSAL_MINI, [6, 2, 2, 2, 4, 2]), (dict(causal=True, **shipped), [6, 2, 2, 2, 4, 2, 5, 2, 8, 2]),
                         (dict(causal=True, n_filters=32, ratios=(8, 5, 4, 2), dimension=512), [6, 2, 8, 2, 5, 2, 4, 2, 2, 2]),
                         (dict(causal=True, n_filters=32, ratios=(3,), dimension=64), None)):
        spec = qa.HCodecSpec(**kw)
        ospec = R.HCodecSpec(**{k: v for k, v in kw.items()})
        st, samples, first, ctx = _geometry(qa_lib, spec)
        assert st == 0, qa_lib.qa_last_error()
        assert samples == ospec.enc_hop and ctx == S.contexts(ospec) and first == S.first_min_frames(ospec), kw
        if want_ctx is not None:  # the figures of DESIGN.md section 43, written out
            assert ctx == want_ctx and first == 2
    # the size query alone, and a ctx array that is too small
    spec_c = qa.HCodecSpec(**CAUSAL_MINI).to_c()
    n = C.c_int32()
    assert qa_lib.qa_hcodec_stream_geometry(C.byref(spec_c), None, None, None, 0, C.byref(n)) == 0 and n.value == 6
    assert qa_lib.qa_hcodec_stream_geometry(C.byref(spec_c), None, None, (C.c_int32 * 2)(), 2, None) != 0
    # the models without a stream: non-causal, H-Codec 1.5, H-Codec 2.0 - refused with what to call instead
    for kw, word in ((dict(MINI), "causal"), (dict(MINI, causal=True, adaptive=True), "1.5"), (dict(MINI, causal=True, version=15), "1.5"),
                     (dict(MINI, causal=True, version=20), "2.0")):
        st, *_ = _geometry(qa_lib, qa.HCodecSpec(**kw))
        msg = qa_lib.qa_last_error().decode()
        assert st == -4 and word in msg and "qa_hcodec_encode" in msg, (kw, st, msg)
    with pytest.raises(qa.QuarkAudioError):
        qa.Codec(spec=qa.HCodecSpec(**MINI)).stream_first_min_frames
    assert qa.Codec(spec=qa.HCodecSpec(**CAUSAL_MINI)).stream_first_min_frames == 2


def test_abi_on_a_null_handle(qa_lib):
    import unified_audio_amd as qa

    assert qa_lib.qa_hcodec_stream_encode(None, None, 640, None, None, None) != 0
    assert qa_lib.qa_hcodec_stream_reset(None) != 0
    assert qa_lib.qa_hcodec_stream_begin(None, 1, 16) != 0
    assert qa_lib.qa_hcodec_stream_offset(None) == -1
    assert qa_lib.qa_hcodec_stream_end(None) == 0
    codec = qa.Codec(spec=qa.HCodecSpec(**CAUSAL_MINI))
    assert not codec.is_streaming and codec.streaming_offset == -1
    with pytest.raises(qa.QuarkAudioError, match="not streaming"):
        codec.encode_stream(torch.zeros(1, 1, 32))
    with pytest.raises(qa.QuarkAudioError):
        codec.reset_streaming()
    with pytest.raises(qa.QuarkAudioError):
        with codec.streaming(1):
            pass
    assert not codec.is_streaming


def test_gpu_code_cases_have_no_near_tie():
    """tests/test_hcodec_stream_gpu.py asserts EQUAL codes against the oracle.  That is only a fair demand where no decision of the oracle's
    own RVQ is a near-tie: every gap between the best and the second-best code, on the oracle's own embeddings in double precision, above
    CODE_TIE_TOL x E|emb|^2 (audit_codes' cap of 0.2 % flipped vectors is below one vector at these sizes and cannot stand in for it)."""
    ospec, sd, wav = S.case_inputs(S.GPU_MINI_CASE, CAUSAL_MINI)
    emb, ac = S.oracle_emb_and_codes(sd, wav, ospec)
    B, D, N = emb.shape
    x = emb.transpose(1, 2).reshape(B * N, D).numpy()
    got = ac.transpose(1, 2).reshape(B * N, -1).numpy()
    excess, best, gap = rvq_c.check_f64(x, R.rvq_codebooks(sd, "quantizer", ospec.num_quantizers).numpy(), got)
    tol = CODE_TIE_TOL * float((x.astype(np.float64) ** 2).sum(1).mean())
    print(f"smallest decision gap {gap.min():.3e} against {tol:.3e}")
    assert (got == best).all() and gap.min() > tol
