"""UniSE(tail="trim") on the HIP components (the small models of tests/test_unise_driver_gpu.py plus a small BiCodec): the last segment of
an utterance runs at its own length through the front-end, the LM and the detokenizer, every row as that segment
alone, bit for bit; tail="wrap" is the unchanged default."""
import functools

import pytest
import torch

from oracle import bicodec_ref as BR
from tests.test_unise_driver_gpu import _components

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _drivers(device):
    import unified_audio_amd as qa
    from unified_audio_amd import synth
    from unified_audio_amd import unise as U

    fx, lm = _components(device)
    bspec = BR.BiCodecSpec(latent_dim=64, codebook_size=128, codebook_dim=8, spk_latent_dim=32, token_num=32, vocos_dim=32, vocos_inter=64,
                           vocos_layers=2, gen_channels=512, rates=(8, 5, 4, 2), kernel_sizes=(16, 11, 8, 4))
    bic = qa.BiCodec(qa.BiCodecSpec(**{f: getattr(bspec, f) for f in bspec.__dataclass_fields__}), device=device)
    bic.load_state_dict(synth.bicodec_state_dict(5, bspec))
    tok = qa.BiCodecTokenizer(model=bic)
    return U.UniSE(lm, fx, tokenizer=tok), U.UniSE(lm, fx, tokenizer=tok, tail="wrap"), U.UniSE(lm, fx, tokenizer=tok, tail="trim")


def _utterances(device, lengths, seed):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(1, n, generator=g) * 0.1).to(device) for n in lengths]


def test_a_trimmed_tail_equals_the_two_pieces_run_alone(qa_lib, gpu_device):
    """'tse' (no peak normalisation ties the pieces together): 80000 + 24320 samples under tail="trim" are the first 80000 samples through
    the unchanged driver followed by the last 24320 samples through tail="trim", each run alone."""
    default, _, trim = _drivers(gpu_device)
    src, = _utterances(gpu_device, [80000 + 24320], 11)
    enr, = _utterances(gpu_device, [32000], 12)
    whole, = trim.enhance("tse", [src], [enr])
    head, = default.enhance("tse", [src[:, :80000]], [enr])
    tail, = trim.enhance("tse", [src[:, 80000:]], [enr])
    assert whole.shape == (104320,) and head.shape == (80000,) and tail.shape == (24320,)
    assert torch.isfinite(whole).all()
    assert torch.equal(whole[:80000], head), "the full segment differs from the same 5 s through the unchanged driver"
    assert torch.equal(whole[80000:], tail), "the trimmed tail differs from the same samples alone"
    (g, s), = trim.enhance_tokens("tse", [src], [enr])
    assert s.shape == (2, 250) and int(s[0].min()) >= 0 and int(s[1, :76].min()) >= 0 and bool((s[1, 76:] == -1).all())


@pytest.mark.parametrize("mode", ["se", "tse"])
def test_a_batch_of_utterances_equals_each_alone_at_its_own_length(qa_lib, gpu_device, mode):
    """0.4 s (the min_tail wrap), 2 s, 5 s and 7.3 s in one call, also in micro-batches that split the utterances, and pipelined."""
    _, _, trim = _drivers(gpu_device)
    lengths = [6400, 32000, 80000, 116800]
    srcs = _utterances(gpu_device, lengths, 13)
    enrs = _utterances(gpu_device, [32000, 48000, 32000, 32000], 14) if mode == "tse" else None
    out = trim.enhance(mode, srcs, enrs)
    assert [tuple(o.shape) for o in out] == [(n,) for n in lengths]
    for i, src in enumerate(srcs):
        alone, = trim.enhance(mode, [src], None if enrs is None else [enrs[i]])
        assert torch.equal(out[i], alone), f"utterance {i} ({lengths[i]} samples) differs from itself alone"
    from unified_audio_amd import unise as U

    small = U.UniSE(trim.dnn, trim.semantic_model, detokenize=trim.detokenize, tail="trim", max_segments=2)
    assert all(torch.equal(a, b) for a, b in zip(small.enhance(mode, srcs, enrs), out)), "micro-batches of two segments changed the result"
    piped = trim.enhance_pipelined(mode, srcs, enrs, segments_per_batch=3)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(piped, out)), "the pipelined driver differs"


def test_wrap_is_the_unchanged_default(qa_lib, gpu_device):
    default, wrap, trim = _drivers(gpu_device)
    srcs = _utterances(gpu_device, [32000, 116800], 15)
    a, b = default.enhance("se", srcs), wrap.enhance("se", srcs)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    ta, tb = default.enhance_tokens("se", srcs), wrap.enhance_tokens("se", srcs)
    assert all(torch.equal(x[1], y[1]) and x[1].shape[1] == 250 and int(x[1].min()) >= 0 for x, y in zip(ta, tb))
    # and trim really is another computation on a short utterance: 100 tokens where wrap pays for 250
    (_, s), = trim.enhance_tokens("se", srcs[:1])
    assert bool((s[0, 100:] == -1).all()) and int(s[0, :100].min()) >= 0
