"""The ring K / V cache under a sliding window without a GPU: the host geometry as a stand-alone program under the
host sanitizers, its Python mirror and the literal-ring restatement against the growing-list stream of tests/transformer_stream_ref.py,
the windowed H-Codec stream against its windowed offline form, the near-tie condition of the case tests/test_stream_ring_gpu.py
compares codes with, and the new C-ABI on null / CPU handles."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from oracle import hcodec_ref as R
from oracle import rvq_c
from tests import ring_stream_ref as RS
from tests import transformer_stream_ref as TR
from tests.util import CODE_TIE_TOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ 1. the selftest
def test_geometry_selftest_is_clean_under_the_host_sanitizers(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler: tools/ring_geometry_selftest.cpp cannot be built")
    exe = str(tmp_path / "ring_geometry_selftest")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-I",
           os.path.join(ROOT, "unified_audio_amd", "csrc"), os.path.join(ROOT, "tools", "ring_geometry_selftest.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "ring_geometry_selftest: ok" in r.stdout


# ------------------------------------------------------------------------------------------------ 2. the Python mirror
def test_capacity_rule():
    for W in (1, 5, 7, 12, 40, 250, 1500):
        for n in (1, 4, 10, 16, 512):
            cap = RS.capacity(W, n)
            assert cap % 32 == 0 and RS.min_rows(W, n) < cap < W + n + 32
    assert (RS.capacity(250, 16), RS.capacity(1500, 16), RS.capacity(40, 512), RS.capacity(40, 16)) == (288, 1536, 576, 64)
    # a ring of min_rows never loses a key the first query of a chunk sees; one row fewer does
    for cap, W, n, pos0 in ((20, 5, 16, 37), (20, 17, 4, 100), (7, 7, 1, 50)):
        assert cap == RS.min_rows(W, n)
        for c, lost in ((cap, False), (cap - 1, True)):
            e = pos0 + n
            held = {RS.pos_of_row(s, e, c) for s in range(c)}
            assert (not set(range(pos0 - W + 1, pos0 + 1)) <= held) == lost
    # p(s) near 2^24 and on a fresh ring
    assert RS.pos_of_row(RS.row_of(RS.MAX_POSITIONS - 1, 96), RS.MAX_POSITIONS, 96) == RS.MAX_POSITIONS - 1
    assert [RS.pos_of_row(s, 3, 8) for s in range(8)] == [0, 1, 2, -5, -4, -3, -2, -1]


RING_CHUNKINGS = {  # 128 frames each; (W, max_chunk): the tight capacity W - 1 + max_chunk is wrapped at least four times
    "tight_16": (13, 16, (16, 1, 1, 4, 16, 7, 16, 3, 16, 16, 16, 16)),
    "tight_5": (7, 5, (5, 1, 2) * 16),
    "frames": (12, 1, (1,) * 128),
}


@pytest.mark.parametrize("name", list(RING_CHUNKINGS))
def test_literal_ring_equals_the_growing_key_list_in_fp64(name):
    """Append at p mod cap, read through p(s) and the visibility rule over NaN-initialised rows: the windowed stream of
    transformer_stream_ref, below 1e-12 - at the tight capacity (with a chunk of exactly max_chunk) and at the library's own."""
    W, max_chunk, chunks = RING_CHUNKINGS[name]
    assert sum(chunks) == 128 and max(chunks) == max_chunk and 128 >= 4 * RS.min_rows(W, max_chunk)
    hidden, heads, layers = 128, 2, 2
    sd = TR.random_state_dict(31, hidden, 2 * hidden, layers)
    x = torch.randn(2, 128, hidden, generator=torch.Generator().manual_seed(32)).double()
    want = TR.stream(sd, x, chunks, layers, heads, W)
    for cap in (RS.min_rows(W, max_chunk), RS.capacity(W, max_chunk)):
        got = RS.ring_stream(sd, x, chunks, layers, heads, W, cap)
        e = TR.rel_err(got, want)
        print(f"{name}: W {W} cap {cap} ({128 / cap:.1f} turns): {e:.2e}")
        assert torch.isfinite(got).all() and e < 1e-12
    # and the windowed stream is the windowed offline form
    assert TR.rel_err(want, TR.forward(sd, x, layers, heads, True, W)) < 1e-12


# ------------------------------------------------------------------------------------------------ 3. the offline definition of the codec case
@pytest.fixture(scope="module")
def codec_case():
    ospec, sd, wav = RS.codec_inputs()
    return dict(ospec=ospec, sd=sd, wav=wav, oracle={W: RS.windowed_oracle(sd, wav, ospec, W) for W in RS.CODEC_WINDOWS})


@pytest.mark.parametrize("W", RS.CODEC_WINDOWS)
def test_windowed_codec_stream_equals_the_windowed_offline_form(codec_case, W):
    ospec, sd, wav = codec_case["ospec"], codec_case["sd"], codec_case["wav"]
    y64 = RS.windowed_offline(sd, wav, ospec, W, torch.float64)
    for name, chunks in RS.CODEC_CHUNKINGS.items():
        e = TR.rel_err(RS.windowed_stream(sd, wav, ospec, W, chunks, torch.float64), y64)
        print(f"W {W} {name}: {e:.2e}")
        assert e < 1e-12
    # fp32: the oracle's own Transformer in the middle against the float64 form, and the dtype-following block beside it
    e_or = TR.rel_err(codec_case["oracle"][W][0], y64)
    e_32 = TR.rel_err(RS.windowed_offline(sd, wav, ospec, W, torch.float32), y64)
    print(f"W {W}: fp32 oracle {e_or:.2e}, fp32 restatement {e_32:.2e}")
    assert e_or < 1e-5 and e_32 <= 4 * max(e_or, 1e-6)


def test_the_window_is_not_the_shipped_model(codec_case):
    """The windowed encoder is another function than the full-causal one: a test that forgets the window fails."""
    from tests import hcodec_stream_ref as S

    ospec, sd, wav = codec_case["ospec"], codec_case["sd"], codec_case["wav"]
    emb_full, ac_full = S.oracle_emb_and_codes(sd, wav, ospec)
    for W in RS.CODEC_WINDOWS:
        emb, ac = codec_case["oracle"][W]
        d = float((emb - emb_full).abs().max() / emb_full.abs().max())
        n = int((ac != ac_full).sum())
        print(f"W {W}: max|emb - emb_full| / max|emb_full| = {d:.3f}, {n} of {ac.numel()} codes differ")
        assert ac.numel() == 648 and d > 0.01 and n > 0


# ------------------------------------------------------------------------------------------------ 4. near-tie audit
@pytest.mark.parametrize("W", RS.CODEC_WINDOWS)
def test_gpu_code_cases_have_no_near_tie(codec_case, W):
    """tests/test_stream_ring_gpu.py asserts EQUAL codes against the windowed oracle.  Fair only where no decision of the oracle's own RVQ
    is a near-tie: every gap between the best and the second-best code, on the oracle's embeddings in double precision, above
    CODE_TIE_TOL x E|emb|^2 (the assertion of tests/test_hcodec_stream_cpu.py::test_gpu_code_cases_have_no_near_tie)."""
    ospec, sd = codec_case["ospec"], codec_case["sd"]
    emb, ac = codec_case["oracle"][W]
    B, D, N = emb.shape
    x = emb.transpose(1, 2).reshape(B * N, D).numpy()
    got = ac.transpose(1, 2).reshape(B * N, -1).numpy()
    excess, best, gap = rvq_c.check_f64(x, R.rvq_codebooks(sd, "quantizer", ospec.num_quantizers).numpy(), got)
    tol = CODE_TIE_TOL * float((x.astype(np.float64) ** 2).sum(1).mean())
    print(f"W {W}: smallest decision gap {gap.min():.3e} against {tol:.3e}")
    assert (got == best).all() and gap.min() > tol


# ------------------------------------------------------------------------------------------------ 5. the C-ABI without a device
def test_abi_on_null_and_cpu_handles(qa_lib):
    import unified_audio_amd as qa

    assert qa_lib.qa_version() == 103
    assert qa_lib.qa_transformer_stream_begin_ring(None, 1, 4) != 0 and b"null handle" in qa_lib.qa_last_error()
    assert qa_lib.qa_transformer_stream_capacity(None) == -1
    assert qa_lib.qa_hcodec_stream_begin_ring(None, 1, 12, 5) != 0 and b"null handle" in qa_lib.qa_last_error()
    assert qa_lib.qa_hcodec_stream_capacity(None) == -1
    assert qa_lib.qa_debug_stream_attn(None, None, None, None, 1, 1, 2, 64, 64, 5, 1, 0, None, None, 0, None) != 0
    assert b"null argument" in qa_lib.qa_last_error()
    # Python, no weights loaded: both or neither of the ring keywords, and not beside max_frames
    codec = qa.Codec(spec=qa.HCodecSpec(**RS.CAUSAL_MINI))
    assert codec.streaming_capacity == -1
    for kw in (dict(left_context=12), dict(max_chunk=5), dict(max_frames=24, left_context=12, max_chunk=5)):
        with pytest.raises(qa.QuarkAudioError):
            codec.streaming_forever(1, **kw)
    assert not codec.is_streaming
    m = qa.Transformer(128, 256, 2, 1, causal=True, use_sliding_window=True, left_context=8)
    assert m.streaming_capacity == -1
    with pytest.raises(qa.QuarkAudioError):
        m.streaming_forever(1, max_chunk=4)  # no weights
    assert not m.is_streaming
