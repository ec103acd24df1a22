"""BiCodec with per-clip lengths, the part that needs no device.

    1  zero-padding into one batch is not the per-clip answer: the CPU oracle on a 20-token clip padded to 37 with arbitrary tokens
       against the clip alone (waveform), and on a short clip whose features come from a padded front-end call (semantic tokens)
    2  the seeds of tests/test_bicodec_ragged_gpu.py: the oracle in fp32 already agrees with the oracle in fp64 inside the audit cap,
       so the cap is a condition the device run can meet
    3  BiCodecTokenizer.token_frames is the front-end's floor rule
    4  the argument checks that run before any library call
"""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import bicodec_ref as BR
from oracle import ssl_ref as SR
from tests import bicodec_ragged_cases as K
from tests import bicodec_tokenize_ref as T
from tests.util import audit_codes, rel_err


# ------------------------------------------------------------------------------------------------ 1
def test_padding_a_token_clip_changes_its_waveform():
    """Row 1 of the small case holds 37 valid tokens; its first 20 are the clip.  Detokenizing all 37 and keeping the clip's samples is
    what a zero-copy padded batch computes."""
    c = K.detok_case("small")
    spec, n = c["spec"], K.TOKEN_LENGTHS[1]
    with torch.no_grad():
        padded = K.detokenize64(T.cast(c["sd"]), c["sem"][1:2], c["glob"][1:2], spec)[0, 0, :n * spec.hop]
    err = rel_err(padded, c["alone"][1]["wav"])
    print(f"BICODEC-RAGGED padded detokenize: {n} of {K.TOKEN_LENGTHS[0]} tokens, relative RMS {err:.3e}")
    assert err > K.STAGE_TOL
    assert err > 1e-2  # not a rounding matter: the k7 / dilated-k7 receptive field covers hundreds of samples of a 320-sample-per-token clip


def _padded_front_end_flips(b):
    """semantic tokens of clip b from features of the rectangular front-end call on the zero-padded, row-normalised batch row against
    those of the clip alone: the share that changes"""
    c = K.tokenizer_case()
    n, nb = K.SAMPLE_LENGTHS[b], K.FRAMES[b]
    row = torch.zeros(1, max(K.SAMPLE_LENGTHS), dtype=torch.float64)
    row[0, :n] = c["wav"][b, :n].double()
    sd64, ssl64 = T.cast(c["sd"]), T.cast(c["ssl_sd"])
    layers = c["espec"].vocos_layers
    with torch.no_grad():
        f_pad = SR.extract_features(ssl64, T.wav_normalize(row), K.XLSR_SMALL)[:, :nb]
        f_one = SR.extract_features(ssl64, T.wav_normalize(row[:, :n]), K.XLSR_SMALL)
    assert f_one.shape[1] == nb
    # the encoder sees the clip's own frames in both cases: what differs is the front-end alone
    t_pad = T.get_semantic_tokens(sd64, f_pad, layers)
    t_one = T.get_semantic_tokens(sd64, f_one, layers)
    return float((t_pad != t_one).double().mean()), rel_err(f_pad, f_one)


def test_padding_in_the_front_end_changes_semantic_tokens():
    share, ferr = _padded_front_end_flips(1)
    print(f"BICODEC-RAGGED padded front-end: clip of {K.SAMPLE_LENGTHS[1]} samples in a row of {max(K.SAMPLE_LENGTHS)}: "
          f"features {ferr:.3e} relative RMS, {share:.3f} of {K.FRAMES[1]} semantic tokens change")
    assert ferr > K.STAGE_TOL
    assert share > K.FLIP_CAP


# ------------------------------------------------------------------------------------------------ 2
def test_seeds_keep_the_fp32_oracle_inside_the_audit_cap():
    c = K.semantic_case()
    cb = T.normalized_codebook(c["sd"]).float().numpy()[None]
    sd32 = T.cast(c["sd"], torch.float32)
    for b, n in enumerate(K.TOKEN_LENGTHS):
        got = T.get_semantic_tokens(sd32, c["feat"][b:b + 1, :n].float(), c["espec"].vocos_layers)
        flips = audit_codes(c["alone"][b]["latent"].float().numpy(), cb, got.reshape(-1, 1).numpy(), c["alone"][b]["tokens"].reshape(-1, 1).numpy())
        assert flips <= K.FLIP_CAP, (b, flips)


def test_published_width_seed_keeps_the_fp32_oracle_inside_the_audit_cap():
    c = K.published_case()
    cb = T.normalized_codebook(c["sd"]).float().numpy()[None]
    sd32 = K.cast_used(c["sd"], ("encoder.", "quantizer."), torch.float32)
    for b, n in enumerate(K.PUBLISHED_LENGTHS):
        got = T.get_semantic_tokens(sd32, c["feat"][b:b + 1, :n].float(), c["espec"].vocos_layers)
        flips = audit_codes(c["alone"][b]["latent"].float().numpy(), cb, got.reshape(-1, 1).numpy(), c["alone"][b]["tokens"].reshape(-1, 1).numpy())
        assert flips <= K.FLIP_CAP, (b, flips)


def test_seeds_keep_the_fp32_detokenize_inside_the_stage_bound():
    for name in K.DSPECS:
        c = K.detok_case(name)
        for b, n in enumerate(K.TOKEN_LENGTHS):
            got = BR.detokenize(c["sd"], c["sem"][b:b + 1, :n], c["glob"][b:b + 1], c["spec"])[0, 0]
            assert rel_err(got, c["alone"][b]["wav"].float()) < K.STAGE_TOL, (name, b)


def test_seeds_keep_the_global_tokens_off_the_fsq_boundaries():
    """the FSQ audit of tests/test_bicodec_tokenize_gpu.py accepts a differing digit only within 1e-3 of a rounding boundary; with 4
    tokens per clip a single accepted flip would already exceed the cap, so the seed keeps every bounded value clear of one"""
    c = K.tokenizer_case()
    for b in range(len(K.SAMPLE_LENGTHS)):
        bd = c["alone"][b]["bounded"].reshape(-1, len(c["espec"].fsq_levels)).double().numpy()
        margin = np.abs(np.abs(bd - np.floor(bd)) - 0.5)
        assert margin.min() > 1e-3, (b, margin.min())


# ------------------------------------------------------------------------------------------------ 3
def test_token_frames_is_the_floor_rule(qa_lib):
    import unified_audio_amd as qa

    assert [K.frames_rule(n) for n in K.SAMPLE_LENGTHS] == list(K.FRAMES)
    assert [K.frames_rule(n) for n in (400, 719, 720, 16000)] == [1, 1, 2, 49]

    class Frames:  # token_frames asks the front-end, clip by clip
        def frames(self, n):
            return K.frames_rule(n)

    tok = qa.BiCodecTokenizer.__new__(qa.BiCodecTokenizer)
    torch.nn.Module.__init__(tok)
    tok._feature_extractor = Frames()
    assert tok.token_frames(K.SAMPLE_LENGTHS) == list(K.FRAMES)
    assert tok.token_frames(torch.tensor([400, 720])) == [1, 2]


# ------------------------------------------------------------------------------------------------ 4
def test_length_checks_name_the_row(qa_lib):
    import unified_audio_amd as qa
    from unified_audio_amd.bicodec import clip_lengths

    lens, arr = clip_lengths(torch.tensor([37, 1]), 2, 1, 37, "x")
    assert lens == [37, 1] and isinstance(arr, C.c_int64 * 2) and list(arr) == [37, 1]
    for bad, row in (([37, 0], 1), ([38, 5], 0), ([3, -2], 1)):
        with pytest.raises(qa.QuarkAudioError) as e:
            clip_lengths(bad, 2, 1, 37, "BiCodec.detokenize")
        assert e.value.status == -1 and f"lengths[{row}] = {bad[row]} is outside 1 .. T = 37" in str(e.value), str(e.value)
    for bad in ([37], [37, 1, 1]):
        with pytest.raises(qa.QuarkAudioError) as e:
            clip_lengths(bad, 2, 1, 37, "BiCodec.detokenize")
        assert e.value.status == -1 and f"{len(bad)} entries" in str(e.value)
    with pytest.raises(qa.QuarkAudioError) as e:
        clip_lengths([400, 399], 2, 400, 11577, "BiCodecTokenizer")
    assert "lengths[1] = 399 is outside 400 .. T = 11577" in str(e.value)


def test_host_side_argument_checks_need_no_device(qa_lib):
    """the C entry points refuse a null vector before they touch a device; BiCodec.tokenize wants both vectors or none"""
    import unified_audio_amd as qa

    x = (C.c_float * 8)()
    lens = (C.c_int64 * 1)(8)
    assert qa_lib.qa_wav_normalize_ragged(x, 1, 8, None, x, 1e-7, None) == -1
    bad = (C.c_int64 * 1)(9)
    assert qa_lib.qa_wav_normalize_ragged(x, 1, 8, bad, x, 1e-7, None) == -1
    assert b"lengths[0] = 9 is outside 1 .. T = 8" in qa_lib.qa_last_error()
    assert qa_lib.qa_wav_normalize_ragged(x, 1, 8, lens, x, -1.0, None) == -1
    assert qa_lib.qa_bicodec_detokenize_ragged(None, None, None, 1, 1, lens, None, None) == -1
    assert qa_lib.qa_bicodec_tokenize_ragged(None, None, 1, 1, lens, None, 8, lens, 0, None, None, None) == -1
    m = qa.BiCodec(qa.BiCodecSpec(**K.fields(K.DSPECS["small"])))
    with pytest.raises(qa.QuarkAudioError, match="together|no tokenizer"):
        m.tokenize({"feat": torch.zeros(1, 4, 1024), "ref_wav": torch.zeros(1, 4000)}, lengths=[4000])
