"""The restatement the GPU tests of the codec Transformer are judged against (tests/transformer_stream_ref.py), pinned on
the CPU: its offline form against oracle.hcodec_ref.transformer and the reference's own module, its cache mode against the module driven
with a DynamicCache, its streaming form against its own offline causal form in float64, and all of it against the committed golden."""
import numpy as np
import pytest
import torch

from oracle import hcodec_ref as R
from oracle import ref_shim
from tests import transformer_stream_ref as TR

needs_reference = pytest.mark.skipif(not ref_shim.reference_available(), reason="/root/reference is only mounted in the build container")

CHUNK_MIXES = [(1,) * 5 + (7, 16, 3, 33, 6), (1,) * 40 + (13,) * 20]
S = TR.GOLDEN_SHAPE


def test_public_class_exists(qa_lib):
    """The class and its cache are exported (every other test of this file needs only the restatement)."""
    import unified_audio_amd as qa

    m = qa.Transformer(128, 256, 2, 2, causal=True)
    assert not m.is_streaming and m.streaming_offset == -1
    with pytest.raises(qa.QuarkAudioError):
        qa.Transformer(128, 256, 2, 2, use_moe=True)
    with pytest.raises(qa.QuarkAudioError):
        qa.Transformer(128, 256, 2, 2, head_dim=32)
    with pytest.raises(qa.QuarkAudioError):
        m(torch.zeros(1, 4, 128))  # no weights loaded
    assert qa.TransformerCache.get_seq_length is not None


@pytest.mark.parametrize("causal,left_context", [(False, 0), (True, 0), (True, 5)])
def test_offline_fp32_equals_the_oracle(causal, left_context):
    """Same graph as oracle.hcodec_ref.transformer, which runs nn.LSTM where the restatement runs its own dtype-following loop: equal to
    within the project's rule 4 max(e32, 1e-6), e32 the oracle's own distance from the float64 form."""
    sd, x = TR.golden_inputs(11)
    y64 = TR.forward(sd, x.double(), S["layers"], S["heads"], causal, left_context)
    y_or = R.transformer({"." + k: v for k, v in sd.items()}, "", x, S["layers"], S["heads"], causal=causal, left_context=left_context)
    y32 = TR.forward(sd, x, S["layers"], S["heads"], causal, left_context)
    e_or, e32 = TR.rel_err(y_or, y64), TR.rel_err(y32, y64)
    print(f"oracle fp32 vs fp64 {e_or:.2e}, restatement fp32 vs fp64 {e32:.2e}")
    assert e32 <= 4 * max(e_or, 1e-6) and e_or < 1e-5
    assert float((y32 - y_or).abs().max() / y_or.abs().max()) <= 4 * max(e_or, 1e-6)


@needs_reference
@pytest.mark.parametrize("causal,window,left_context", [(False, False, 0), (True, False, 0), (True, True, 5)])
def test_offline_oracle_equals_the_reference_module_bit_for_bit(causal, window, left_context):
    sd, x = TR.golden_inputs(12)
    m, _ = TR.load_reference_transformer(S["hidden"], S["inter"], S["heads"], S["layers"], causal, window, left_context)
    m.load_state_dict(sd)
    with torch.no_grad():
        y_ref = m(x)
    y_or = R.transformer({"." + k: v for k, v in sd.items()}, "", x, S["layers"], S["heads"], causal=causal, left_context=left_context)
    assert torch.equal(y_or, y_ref)
    y64 = TR.forward(sd, x.double(), S["layers"], S["heads"], causal, left_context)
    assert TR.rel_err(y_ref, y64) < 1e-5


@needs_reference
def test_cache_mode_equals_the_reference_module_over_a_dynamic_cache():
    """Chunks (5, 7) through the reference's own cache: the LSTM restarts on every call, RoPE continues, every query sees every key."""
    sd, x = TR.golden_inputs(13)
    x = x[:, :12]
    m, cache_cls = TR.load_reference_transformer(S["hidden"], S["inter"], S["heads"], S["layers"])
    m.load_state_dict(sd)
    cache, state64, state32, t = cache_cls(), TR.new_state(S["layers"]), TR.new_state(S["layers"]), 0
    for n in (5, 7):
        with torch.no_grad():
            y_ref, cache = m(x[:, t:t + n], past_key_values=cache, use_cache=True)
        y64 = TR.forward_cached(sd, x[:, t:t + n].double(), state64, S["layers"], S["heads"])
        y32 = TR.forward_cached(sd, x[:, t:t + n], state32, S["layers"], S["heads"])
        e_ref, e32 = TR.rel_err(y_ref, y64), TR.rel_err(y32, y64)
        print(f"chunk of {n} at {t}: module fp32 vs fp64 restatement {e_ref:.2e}, fp32 restatement {e32:.2e}")
        assert e_ref < 1e-5 and e32 <= 4 * max(e_ref, 1e-6)
        t += n
        assert cache.get_seq_length() == TR.state_length(state64) == t
    # the chunked result is NOT the offline one: the restarted LSTM has forgotten the first chunk
    y_off = TR.forward(sd, x.double(), S["layers"], S["heads"])
    assert TR.rel_err(y64, y_off[:, 5:]) > 1e-3


@needs_reference
def test_reference_causal_second_cached_chunk_raises():
    sd, x = TR.golden_inputs(14)
    m, cache_cls = TR.load_reference_transformer(S["hidden"], S["inter"], S["heads"], S["layers"], causal=True)
    m.load_state_dict(sd)
    with torch.no_grad():
        y, cache = m(x[:, :5], past_key_values=cache_cls(), use_cache=True)
        with pytest.raises(RuntimeError, match="expanded size"):
            m(x[:, 5:12], past_key_values=cache, use_cache=True)
    state = TR.new_state(S["layers"])
    y0 = TR.forward_cached(sd, x[:, :5], state, S["layers"], S["heads"], causal=True)
    assert TR.rel_err(y0, TR.forward(sd, x[:, :5].double(), S["layers"], S["heads"], True)) < 1e-5  # an empty cache: the offline causal call
    assert TR.rel_err(y, y0.double()) < 1e-5
    with pytest.raises(RuntimeError):
        TR.forward_cached(sd, x[:, 5:12], state, S["layers"], S["heads"], causal=True)


@pytest.mark.parametrize("left_context", [0, 24])
@pytest.mark.parametrize("chunks", CHUNK_MIXES, ids=["mix70", "mix300"])
@pytest.mark.parametrize("hidden,heads", [(128, 2), (192, 2), (256, 2)], ids=["hd64", "hd96", "hd128"])
def test_streaming_equals_offline_causal_in_fp64(hidden, heads, chunks, left_context):
    """Carried LSTM (h, c) + cached roped K / V reproduce the offline causal Transformer: the causal graph is exactly streamable."""
    T = sum(chunks)
    sd = TR.random_state_dict(21, hidden, 2 * hidden, 2)
    x = torch.randn(2, T, hidden, generator=torch.Generator().manual_seed(22)).double()
    y_off = TR.forward(sd, x, 2, heads, True, left_context)
    y_st = TR.stream(sd, x, chunks, 2, heads, left_context)
    e = TR.rel_err(y_st, y_off)
    print(f"streamed vs offline, fp64: {e:.2e}")
    assert e < 1e-12
    assert float(y_off.abs().max()) > 0.5  # activations O(1): the comparison is not one of zeros


def test_golden_holds_the_reference_modules_outputs():
    """tests/golden/transformer_cache_small.npz against the restatement (always) and against a regeneration from the reference module (where
    the reference exists)."""
    g = np.load(TR.GOLDEN)
    seed = int(g["seed"])
    sd, x = TR.golden_inputs(seed)
    assert np.array_equal(g["x"], x.numpy())
    xd = x.double()
    truth = {"offline_noncausal": TR.forward(sd, xd, S["layers"], S["heads"]),
             "offline_causal": TR.forward(sd, xd, S["layers"], S["heads"], True)}
    state, ys, t = TR.new_state(S["layers"]), [], 0
    for n in TR.GOLDEN_CHUNKS:
        ys.append(TR.forward_cached(sd, xd[:, t:t + n], state, S["layers"], S["heads"]))
        t += n
    truth["cached_noncausal"] = torch.cat(ys, 1)
    for name, y64 in truth.items():
        e = TR.rel_err(torch.from_numpy(g[name]), y64)
        print(f"golden {name}: module fp32 vs fp64 restatement {e:.2e}")
        assert g[name].shape == (S["B"], S["T"], S["hidden"]) and e < 1e-5
    if ref_shim.reference_available():
        again = TR.reference_golden(seed)
        assert set(again) == set(g.files)
        for name in g.files:
            assert np.array_equal(again[name], g[name]), name
