"""Per-clip lengths in one H-Codec 2.0 encode / decode call (Codec.encode_ragged / decode_ragged on a `version == 20` model,
qa_hcodec_encode_ragged / _decode_ragged, qa_resample_ragged): row b of a per-clip call is the rectangular call on
that clip alone at its own length.  Shapes and seeds: tests/hcodec20_ragged_cases.py.

    1  every row against oracle/hcodec20_ref.py on the clip alone; -1 / exact zeros behind it
    2  NaN behind every length, junk against -1 in the codes: the same bits
    3  a row does not know its neighbours, and equals the rectangular B = 1 call
    4  equal lengths are the rectangular call: same bits, same launches, no masked attention
    5  refusals come before any launch
    6  full width (d = 1536 persistent recurrence, 24 heads, n_fft 1920, 16 codebooks)
    7  the resampler with lengths
    8  the tokenizer: feats= given, and through an SSLFeatureExtractor in ONE front-end call
"""
import ctypes as C

import pytest
import torch

from oracle import hcodec_ref as R
from oracle import resample_ref as RR
from oracle import ssl_ref as S
from oracle import synth
from tests import hcodec20_ragged_cases as K
from tests.test_hcodec_ragged_gpu import _att_launches
from tests.util import audit_codes_bnq, rel_err

pytestmark = pytest.mark.gpu

HOP, FPC, JUNK, FRAMES, N = K.HOP, K.FPC, K.JUNK, K.FRAMES, K.N
STAGE_TOL = 5e-5  # tests/test_hcodec_gpu.py


def _codec(case, device, causal=False, **kw):
    import unified_audio_amd as qa

    return qa.Codec(None, None, None, spec=K.product_spec(case["spec"], causal), device=device, **kw).load_state_dict(case["sd"])


def _run(codec, case, frames, device):
    """The per-clip encode on clean inputs, the decode of the ORACLE's codes with junk behind them, and the decode of the call's own."""
    q, n = case["spec"].num_quantizers, max(frames)
    ac, sc = codec.encode_ragged(case["wav"].to(device), case["feat"].to(device), frames)
    ac_pad = torch.full((len(frames), q, n), JUNK, dtype=torch.int64)
    sc_pad = ac_pad.clone()
    for b, f in enumerate(frames):
        ac_pad[b, :, :f], sc_pad[b, :, :f] = case["alone"][b]["ac"][0], case["alone"][b]["sc"][0]
    w = codec.decode_ragged(ac_pad.to(device), sc_pad.to(device), lengths=frames)  # check_codes is on: the junk must not count
    w_own = codec.decode_ragged(ac, sc, lengths=frames)
    torch.cuda.synchronize()
    return dict(codec=codec, ac=ac, sc=sc, w=w, w_own=w_own, ac_pad=ac_pad, sc_pad=sc_pad)


@pytest.fixture(scope="module")
def small(qa_lib, gpu_device):
    case = K.small_case()
    return dict(case, **_run(_codec(case, gpu_device), case, FRAMES, gpu_device))


def _check_rows(run, frames, wav_tol):
    sd, q = run["sd"], run["spec"].num_quantizers
    cb_a, cb_s = R.rvq_codebooks(sd, "quantizer", q), R.rvq_codebooks(sd, "semantic_quantizer", q)
    ac, sc, w = run["ac"].cpu(), run["sc"].cpu(), run["w"].cpu()
    n = max(frames)
    assert ac.shape == sc.shape == (len(frames), q, n) and w.shape == (len(frames), HOP * n)
    for b, f in enumerate(frames):
        o = run["alone"][b]
        flips = (audit_codes_bnq(o["emb"], cb_a, ac[b:b + 1, :, :f], o["ac"], max_flip_frac=1.0),
                 audit_codes_bnq(o["sem"], cb_s, sc[b:b + 1, :, :f], o["sc"], max_flip_frac=1.0))
        err = rel_err(w[b, :HOP * f], o["wav"][0])
        print(f"clip {b}: {f} code frames, near-tie flips {flips}, decode rel. RMS error {err:.3e} (bound {wav_tol:.0e})")
        assert (ac[b, :, f:] == -1).all() and (sc[b, :, f:] == -1).all()
        assert err < wav_tol, (b, f, err)
        assert torch.equal(w[b, HOP * f:], torch.zeros(HOP * (n - f)))


def test_ragged_rows_match_the_oracle_clip_by_clip(small):
    """1. Codes: the near-tie audit with the project's CODE_TIE_TOL on the oracle's own RVQ inputs, max_flip_frac=1.0 as section 25 has it
    for clips of 1 .. 70 vectors; -1 behind the clip.  Decode of the ORACLE's codes with 10 ** 9 behind them: relative RMS < 1e-4, exact
    zeros behind the clip.  Zero padding through the oracle misses that bound by more than 1000 x (tests/test_hcodec20_ragged_cpu.py)."""
    _check_rows(small, FRAMES, 1e-4)


def _nan_behind(case, frames):
    wav, feat = case["wav"].clone(), case["feat"].clone()
    for b, f in enumerate(frames):
        wav[b, HOP * f:] = float("nan")
        feat[b, :, FPC * f:] = float("nan")
    return wav, feat


def test_padding_is_never_read(small, gpu_device):
    """2. NaN in wav and feat behind every clip's length: the same codes and, from them, the same waveform, bit for bit; and -1 in the
    codes behind a clip's end where run 1 had 10 ** 9."""
    codec = small["codec"]
    wav, feat = _nan_behind(small, FRAMES)
    ac, sc = codec.encode_ragged(wav.to(gpu_device), feat.to(gpu_device), FRAMES)
    assert torch.equal(ac, small["ac"]) and torch.equal(sc, small["sc"])
    assert torch.equal(codec.decode_ragged(ac, sc, lengths=FRAMES), small["w_own"])
    ac_pad, sc_pad = small["ac_pad"].clone(), small["sc_pad"].clone()
    for b, f in enumerate(FRAMES):
        ac_pad[b, :, f:], sc_pad[b, :, f:] = -1, -1
    assert torch.equal(codec.decode_ragged(ac_pad.to(gpu_device), sc_pad.to(gpu_device), lengths=FRAMES), small["w"])


def _batch(clips, n, sem_in, device):
    """clips: (wav [3840 f], feat [sem_in, 4 f]) per row -> wav [B, 3840 n], feat [B, sem_in, 4 n] with NaN behind every clip, the lengths"""
    wav = torch.full((len(clips), HOP * n), float("nan"))
    feat = torch.full((len(clips), sem_in, FPC * n), float("nan"))
    for b, (w, f) in enumerate(clips):
        wav[b, :w.numel()], feat[b, :, :f.shape[1]] = w, f
    return wav.to(device), feat.to(device), [w.numel() // HOP for w, _ in clips]


def _row_invariance(codec, case, f, batches, device):
    """The clip of f code frames gives the same bits as a row of every batch of `batches` ((clips, n, row) each), two identical calls
    agree, and the rectangular B = 1 call on the clip alone gives the same bits, encode and decode (2.0 has no fused stage 0)."""
    q, ks = case["spec"].num_quantizers, case["spec"].codebook_size
    outs = []
    for clips, n, row in batches:
        wav, feat, fr = _batch(clips, n, case["spec"].sem_in, device)
        ac, sc = codec.encode_ragged(wav, feat, fr)
        ac2, sc2 = codec.encode_ragged(wav, feat, fr)
        assert torch.equal(ac, ac2) and torch.equal(sc, sc2)
        assert all((ac[b, :, g:] == -1).all() and (sc[b, :, g:] == -1).all() for b, g in enumerate(fr))
        outs.append((ac[row, :, :f].clone(), sc[row, :, :f].clone(), row, n, fr))
    for a, s, _, _, _ in outs[1:]:
        assert torch.equal(a, outs[0][0]) and torch.equal(s, outs[0][1])
    a0, s0 = outs[0][0], outs[0][1]
    waves = []
    for _, _, row, n, fr in outs:
        ac = torch.full((len(fr), q, n), JUNK, dtype=torch.int64, device=device)
        sc = ac.clone()
        for b, g in enumerate(fr):  # the neighbours decode some other valid codes
            ac[b, :, :g], sc[b, :, :g] = (b + torch.arange(g, device=device)) % ks, (2 * b + torch.arange(g, device=device)) % ks
        ac[row, :, :f], sc[row, :, :f] = a0, s0
        w = codec.decode_ragged(ac, sc, lengths=fr)
        assert torch.equal(w, codec.decode_ragged(ac, sc, lengths=fr))
        assert all(torch.equal(w[b, HOP * g:], torch.zeros(HOP * (n - g), device=device)) for b, g in enumerate(fr))
        waves.append(w[row, :HOP * f].clone())
    assert all(torch.equal(w, waves[0]) for w in waves[1:])
    return a0, s0, waves[0]


def _clip(seed, f, sem_in):
    return synth.synth_wav_fullband(seed, 1, HOP * f)[0], synth.synth_feat(seed + 50, 1, FPC * f, sem_in)[0]


def test_a_row_does_not_know_its_neighbours(small, gpu_device):
    """3. The clip of 9 code frames as row 1 of [35, 9, 1], as row 2 of [17, 17, 9] inside 20 frames, and as a batch of one inside 12."""
    codec = small["codec"]
    x35, y9, z1, u17, v17 = _clip(1, 35, 64), _clip(2, 9, 64), _clip(3, 1, 64), _clip(4, 17, 64), _clip(5, 17, 64)
    a9, s9, w9 = _row_invariance(codec, small, 9, (([x35, y9, z1], 35, 1), ([u17, v17, y9], 20, 2), ([y9], 12, 0)), gpu_device)
    ra, rs = codec.encode(y9[0].to(gpu_device)[None], y9[1].to(gpu_device)[None])
    assert torch.equal(ra[0], a9) and torch.equal(rs[0], s9)
    assert torch.equal(codec.decode(a9[None], s9[None])[0], w9)


def test_equal_lengths_are_the_rectangular_call(small, qa_lib, gpu_device):
    """4. lengths = [N] * B: the outputs of encode / decode, bit for bit, through as many attention launches as the rectangular calls
    issue, none of them masked; [N, N - 1, N] masks every one."""
    codec, o = small["codec"], small["spec"]
    B, n = 3, 9
    layers = o.enc_transformer_layers + o.dec_transformer_layers
    wav = synth.synth_wav_fullband(31, B, HOP * n).to(gpu_device)
    feat = synth.synth_feat(32, B, FPC * n, 64).to(gpu_device)
    a0, m0 = _att_launches(qa_lib)
    ac, sc = codec.encode(wav, feat)
    w = codec.decode(ac, sc)
    a1, m1 = _att_launches(qa_lib)
    ac2, sc2 = codec.encode_ragged(wav, feat, [n] * B)
    w2 = codec.decode_ragged(ac, sc, lengths=torch.tensor([n] * B))
    a2, m2 = _att_launches(qa_lib)
    assert torch.equal(ac, ac2) and torch.equal(sc, sc2) and torch.equal(w, w2)
    assert (ac2 >= 0).all() and (sc2 >= 0).all()
    assert a1 - a0 == a2 - a1 == layers and m0 == m1 == m2
    ac3, sc3 = codec.encode_ragged(wav, feat, [n, n - 1, n])
    codec.decode_ragged(ac3, sc3, lengths=[n, n - 1, n])
    a3, m3 = _att_launches(qa_lib)
    assert a3 - a2 == layers and m3 - m2 == layers


def test_refusals_and_checks_come_before_any_launch(small, qa_lib, gpu_device):
    """5. Bad lengths are QA_ERR_INVALID and name the row; a causal 2.0 model is QA_ERR_UNSUPPORTED through the _ragged doors;
    encode(lengths=) / decode(lengths=) on a 2.0 model stay refused with -4 and now name the _ragged methods; nothing is launched by a
    refused call; a live entry out of range still raises IndexError."""
    import unified_audio_amd as qa

    codec, q = small["codec"], small["spec"].num_quantizers
    n = 3
    wav = synth.synth_wav_fullband(41, 2, HOP * n).to(gpu_device)
    feat = synth.synth_feat(42, 2, FPC * n, 64).to(gpu_device)
    codes = torch.zeros((2, q, n), dtype=torch.int64, device=gpu_device)
    before = _att_launches(qa_lib)
    for bad in (0, n + 1, -3):
        for call in (lambda fr: codec.encode_ragged(wav, feat, fr), lambda fr: codec.decode_ragged(codes, codes, lengths=fr)):
            with pytest.raises(qa.QuarkAudioError) as e:
                call([n, bad])
            assert e.value.status == -1 and f"frames[1] = {bad}" in str(e.value), str(e.value)
    for call in (lambda: codec.encode_ragged(wav, feat, [n]), lambda: codec.decode_ragged(codes, codes, lengths=[n, n, n])):
        with pytest.raises(qa.QuarkAudioError) as e:
            call()
        assert e.value.status == -1
    for call in (lambda: codec.encode(wav, feat, lengths=[n, 1]), lambda: codec.decode(codes, codes, lengths=[n, 1])):
        with pytest.raises(qa.QuarkAudioError) as e:
            call()
        assert e.value.status == -4 and "2.0" in str(e.value), str(e.value)
        assert "encode_ragged" in str(e.value) and "decode_ragged" in str(e.value)
    causal = _codec(small, gpu_device, causal=True)
    for call in (lambda: causal.encode_ragged(wav, feat, [n, 1]), lambda: causal.decode_ragged(codes, codes, lengths=[n, 1])):
        with pytest.raises(qa.QuarkAudioError) as e:
            call()
        assert e.value.status == -4 and "causal" in str(e.value), str(e.value)
    assert _att_launches(qa_lib) == before  # the refused calls launched nothing
    assert causal.encode(wav, feat)[0].shape == (2, q, n)  # and without lengths the causal model runs as before
    with pytest.raises(IndexError):  # a live entry out of range still counts
        codec.decode_ragged(torch.full_like(codes, 64), codes, lengths=[n, 2])


# ------------------------------------------------------------------------------------------------ 6
@pytest.fixture(scope="module")
def wide(qa_lib, gpu_device):
    case = K.wide_case()
    return dict(case, **_run(_codec(case, gpu_device), case, K.WIDE_FRAMES, gpu_device))


def test_full_width_rows_match_the_oracle(wide):
    """Full H-Codec 2.0 widths with two ConvNeXt blocks per stack, clips of 8 / 3 / 1 code frames: the bounds of
    tests/test_hcodec_gpu.py::test_hcodec20_full_width_parity - 2 * STAGE_TOL for the waveform, the near-tie audit for the codes."""
    _check_rows(wide, K.WIDE_FRAMES, 2 * STAGE_TOL)


def test_full_width_row_does_not_know_its_neighbours(wide, gpu_device):
    """The clip of 3 code frames as row 1 of [8, 3, 1], as row 0 of [3, 5] and alone inside 4 frames - and against the rectangular
    B = 1 call, bit for bit: the d = 1536 recurrence (lstm_persistent_kernel) puts the batch on the M rows of its MFMA tiles and splits
    K over the waves in a fixed order, so a row's bits do not depend on B."""
    codec, si = wide["codec"], wide["spec"].sem_in
    x8, y3, z1, v5 = _clip(11, 8, si), _clip(12, 3, si), _clip(13, 1, si), _clip(14, 5, si)
    a3, s3, w3 = _row_invariance(codec, wide, 3, (([x8, y3, z1], 8, 1), ([y3, v5], 5, 0), ([y3], 4, 0)), gpu_device)
    ra, rs = codec.encode(y3[0].to(gpu_device)[None], y3[1].to(gpu_device)[None])
    assert torch.equal(ra[0], a3) and torch.equal(rs[0], s3)
    assert torch.equal(codec.decode(a3[None], s3[None])[0], w3)


# ------------------------------------------------------------------------------------------------ 7
@pytest.mark.parametrize("orig", [48000, 44100])
def test_resample_with_lengths(qa_lib, gpu_device, orig):
    """Rows of T / 3847 / 41 / 1 samples, NaN behind every length: the valid outputs against the oracle on the clip alone (the bound of
    test_resample_matches_the_torchaudio_restatement), exact zeros behind them, bit-equal to qa_resample on the clip alone."""
    from unified_audio_amd import _lib

    T = 3840 * 3 if orig == 48000 else 4410 * 2 + 13
    lens = [T, 3847, 41, 1]
    g = torch.Generator().manual_seed(orig)
    wav = torch.randn(len(lens), T, generator=g)
    for b, n in enumerate(lens):
        wav[b, n:] = float("nan")
    x = wav.to(gpu_device)
    n_out = qa_lib.qa_resample_length(T, orig, 16000)
    out = torch.full((len(lens), n_out), float("nan"), device=gpu_device)
    arr = (C.c_int64 * len(lens))(*lens)
    _lib.check(qa_lib.qa_resample_ragged(x.data_ptr(), len(lens), T, arr, orig, 16000, out.data_ptr(), None))
    torch.cuda.synchronize()
    for b, n in enumerate(lens):
        want = RR.resample(wav[b:b + 1, :n], orig, 16000)
        m = want.shape[-1]
        assert m == qa_lib.qa_resample_length(n, orig, 16000)
        err = float((out[b, :m].cpu() - want[0]).abs().max())
        print(f"{orig} Hz, {n} samples -> {m}: max abs error {err:.3e}")
        assert err < 2e-6 * float(want.abs().max()) + 1e-6
        assert torch.equal(out[b, m:], torch.zeros(n_out - m, device=gpu_device))
        alone = torch.full((1, m), float("nan"), device=gpu_device)
        clip = x[b:b + 1, :n].contiguous()
        _lib.check(qa_lib.qa_resample(clip.data_ptr(), 1, n, orig, 16000, alone.data_ptr(), None))
        assert torch.equal(alone[0], out[b, :m])
    for bad in (0, T + 1):
        arr = (C.c_int64 * len(lens))(T, bad, 1, 1)
        assert qa_lib.qa_resample_ragged(x.data_ptr(), len(lens), T, arr, orig, 16000, out.data_ptr(), None) == -1
        assert f"lengths[1] = {bad}".encode() in qa_lib.qa_last_error()


# ------------------------------------------------------------------------------------------------ 8
LENS = [3840 * 5 + 7, 3840 + 1]  # samples, no hop multiples: 6 and 2 code frames


def _tok_wav():
    w = torch.full((2, LENS[0]), float("nan"))
    w[0], w[1, :LENS[1]] = synth.synth_wav_fullband(1, 1, LENS[0])[0], synth.synth_wav_fullband(2, 1, LENS[1])[0]
    return w


def _check_tokens(tok, w, ac, sc, alone, q, device):
    assert ac.shape == sc.shape == (2, q, 6) and (ac[1, :, 2:] == -1).all() and (sc[1, :, 2:] == -1).all()
    assert (ac[1, :, :2] >= 0).all() and (ac[0] >= 0).all() and (sc[0] >= 0).all()
    for b, f in enumerate((6, 2)):
        a1, s1 = alone(b)
        assert torch.equal(a1[0], ac[b, :, :f]) and torch.equal(s1[0], sc[b, :, :f])
    out = tok.detokenize(ac, sc, lengths=tok.code_frames(LENS))
    assert out.shape == (2, HOP * 6) and torch.equal(out[1, HOP * 2:], torch.zeros(HOP * 4, device=device))
    assert bool(out[1, :HOP * 2].abs().sum() > 0) and bool(torch.isfinite(out).all())


def test_tokenizer_with_features_given(small, gpu_device):
    """tokenize(wav, feats=, lengths=samples) on a 2.0 model: shapes, -1 behind, every clip torch.equal to the rectangular tokenizer on
    the clip alone, detokenize(..., lengths=) zeros behind."""
    import unified_audio_amd as qa

    tok = qa.HCodecTokenizer(model=small["codec"])
    assert tok.sampling_rate == 48000 and tok.hop_length == HOP and tok.code_frames(LENS) == [6, 2]
    w = _tok_wav()
    feats = synth.synth_feat(2, 2, FPC * 6, 64).transpose(1, 2)
    feats[1, FPC * 2:] = float("nan")
    ac, sc = tok.tokenize(w, feats=feats, lengths=LENS)
    f = (6, 2)
    _check_tokens(tok, w, ac, sc, lambda b: tok.tokenize(w[b:b + 1, :LENS[b]], feats=feats[b:b + 1, :FPC * f[b]]),
                  small["spec"].num_quantizers, gpu_device)


def test_tokenizer_makes_one_front_end_call(small, gpu_device):
    """The same through a reduced HuBERT-style SSLFeatureExtractor (tests/test_ssl_ragged_gpu.py builds it so): the 48 kHz lengths go
    through the resampler, the 16 kHz lengths to the extractor, in ONE call; NaN behind every clip; equal to the clip alone."""
    import unified_audio_amd as qa

    calls = []

    class Spy(qa.SSLFeatureExtractor):
        def __call__(self, wavs, lengths=None):
            calls.append((tuple(wavs.shape), None if lengths is None else list(lengths)))
            return super().__call__(wavs, lengths=lengths)

    sspec = S.SSLSpec(conv_dim=(64,) * 7, hidden_size=64, num_hidden_layers=2, num_attention_heads=2, intermediate_size=128,
                      num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=1)
    fx = Spy(qa.SSLSpec(**{f: getattr(sspec, f) for f in sspec.__dataclass_fields__}), device=gpu_device)
    fx.load_state_dict(S.synth_state_dict(9, sspec))
    tok = qa.HCodecTokenizer(model=small["codec"], feature_extractor=fx)
    w = _tok_wav()
    ac, sc = tok.tokenize(w, lengths=LENS)
    assert calls == [((2, 1280 * 6), [1280 * 6, 1280 * 2])], calls
    _check_tokens(tok, w, ac, sc, lambda b: tok.tokenize(w[b:b + 1, :LENS[b]]), small["spec"].num_quantizers, gpu_device)
