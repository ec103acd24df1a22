"""BiCodec with per-clip lengths in one tokenize / detokenize call: row b of a call with lengths is the clip alone
at its own length - against the fp64 CPU oracle on that clip, and bit for bit against the rectangular B = 1 call on that clip.

Shapes, seeds and the oracle's answers: tests/bicodec_ragged_cases.py (shared with the CPU file, which asserts that the seeds keep the
fp32 oracle inside the bounds used here).

    1  every row against the oracle on the clip alone: detokenize (taps and waveform, zeros behind), semantic tokens (audit, -1 behind),
       global tokens (FSQ audit on get_ref_clip(clip))
    2  NaN / junk behind every clip's end changes nothing
    3  a row == the rectangular B = 1 call on the trimmed clip == itself at another row, among other neighbours, inside a longer T
    4  lengths = [full] * B is the rectangular call, on all five entry points
    5  bad lengths are refused before any launch, naming the row; the handle is unharmed
    6  BiCodecTokenizer: one normalisation, one front-end call, one codec call; the round trip
    7  the published widths with a short backbone, B = 2, lengths (50, 23)
"""
from __future__ import annotations

import ctypes as C
import functools

import pytest
import torch

from tests import bicodec_ragged_cases as K
from tests import bicodec_tokenize_ref as T
from tests.test_bicodec_tokenize_gpu import _audit_fsq
from tests.util import audit_codes, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TAPS = ("z_q", "prenet.down", "prenet.backbone", "prenet.out")


# ------------------------------------------------------------------------------------------------ shared, built once, never modified
@functools.lru_cache(maxsize=None)
def _detok(name):
    import unified_audio_amd as qa

    c = K.detok_case(name)
    m = qa.BiCodec(qa.BiCodecSpec(**K.fields(c["spec"])), device=DEV).load_state_dict(c["sd"])
    sem, glob = c["sem"].to(DEV), c["glob"].to(DEV)
    m.enable_taps()
    wav = m.detokenize(sem, glob, lengths=K.TOKEN_LENGTHS)
    names = TAPS + tuple(f"gen.block{i}" for i in range(len(c["spec"].rates)))
    taps = {k: m.tap(k).clone() for k in names}
    m.enable_taps(False)
    torch.cuda.synchronize()
    return dict(c, m=m, sem_d=sem, glob_d=glob, wav=wav, taps=taps)


@functools.lru_cache(maxsize=None)
def _semantic():
    import unified_audio_amd as qa

    c = K.semantic_case()
    m = qa.BiCodec(c["dspec"], device=DEV, encoder_spec=c["espec"]).load_state_dict(c["sd"])
    feat = c["feat"].to(DEV)
    tok = m.get_semantic_tokens({"feat": feat}, lengths=K.TOKEN_LENGTHS)
    torch.cuda.synchronize()
    return dict(c, m=m, feat_d=feat, tok=tok)


@functools.lru_cache(maxsize=None)
def _tokenizer():
    import unified_audio_amd as qa

    c = K.tokenizer_case()
    calls = []

    class Spy(qa.SSLFeatureExtractor):
        def __call__(self, wavs, lengths=None):
            calls.append((tuple(wavs.shape), None if lengths is None else list(lengths)))
            return super().__call__(wavs, lengths=lengths)

    fx = Spy(K.xlsr_qa_spec(), device=DEV).load_state_dict(c["ssl_sd"])
    m = qa.BiCodec(c["dspec"], device=DEV, encoder_spec=c["espec"]).load_state_dict(c["sd"])
    tok = qa.BiCodecTokenizer(model=m, feature_extractor=fx)
    tok.config = {"sample_rate": K.REF_LEN, "ref_segment_duration": 1, "latent_hop_length": 320}  # get_ref_clip's length
    assert tok.ref_segment_length == K.REF_LEN
    wav = c["wav"].to(DEV)
    glob, sem = tok.tokenize(wav, lengths=K.SAMPLE_LENGTHS)
    torch.cuda.synchronize()
    first_calls = list(calls)
    return dict(c, m=m, fx=fx, tok=tok, wav_d=wav, glob=glob, sem=sem, calls=calls, first_calls=first_calls)


def _zeros(t):
    return torch.equal(t, torch.zeros_like(t))


# ------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("name", sorted(K.DSPECS))
def test_detokenize_rows_match_the_oracle_on_the_clip_alone(qa_lib, gpu_device, name):
    s = _detok(name)
    spec, B, Tm = s["spec"], len(K.TOKEN_LENGTHS), max(K.TOKEN_LENGTHS)
    assert s["wav"].shape == (B, 1, Tm * spec.hop) and s["wav"].dtype == torch.float32
    bad = []
    for b, n in enumerate(K.TOKEN_LENGTHS):
        ref = s["alone"][b]
        report = {}
        for k, v in s["taps"].items():
            rate = v.numel() // (B * Tm * ref["taps"][k].shape[1])  # frames per token at this stage
            rows = v.reshape(B, Tm * rate, -1)[b].cpu()
            assert torch.isfinite(rows).all(), (b, k)  # the rows behind a clip's end stay finite at every stage
            report[k] = rel_err(rows[:n * rate], ref["taps"][k].float())
        got = s["wav"][b, 0].cpu()
        report["wav"] = rel_err(got[:n * spec.hop], ref["wav"].float())
        print(f"BICODEC-RAGGED {name} clip {b} ({n} tokens): " + " ".join(f"{k} {v:.2e}" for k, v in report.items()))
        bad += [f"clip {b} ({n} tokens) {k}: {v:.3e} (bound {K.STAGE_TOL})" for k, v in report.items() if not v < K.STAGE_TOL]
        if not _zeros(got[n * spec.hop:]):
            bad.append(f"clip {b}: the samples behind {n * spec.hop} are not exactly 0")
    assert not bad, "\n".join(bad)


def test_semantic_rows_match_the_oracle_on_the_clip_alone(qa_lib, gpu_device):
    s = _semantic()
    tok = s["tok"].cpu()
    assert tok.shape == (len(K.TOKEN_LENGTHS), max(K.TOKEN_LENGTHS)) and tok.dtype == torch.int64
    cb = T.normalized_codebook(s["sd"]).float().numpy()[None]
    for b, n in enumerate(K.TOKEN_LENGTHS):
        ref = s["alone"][b]
        flips = audit_codes(ref["latent"].float().numpy(), cb, tok[b, :n].reshape(-1, 1).numpy(), ref["tokens"].reshape(-1, 1).numpy())
        assert flips <= K.FLIP_CAP, (b, flips)
        assert bool((tok[b, n:] == -1).all()), b


def test_global_rows_match_the_oracle_on_the_reference_clip_of_the_clip_alone(qa_lib, gpu_device):
    s = _tokenizer()
    glob = s["glob"].cpu()
    assert glob.shape == (len(K.SAMPLE_LENGTHS), 1, s["espec"].token_num) and glob.dtype == torch.int32
    for b in range(len(K.SAMPLE_LENGTHS)):
        _audit_fsq(s["alone"][b]["bounded"], glob[b, 0], s["alone"][b]["glob"], s["espec"].fsq_levels)


# ------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("name", sorted(K.DSPECS))
def test_tokens_behind_a_clip_are_never_read(qa_lib, gpu_device, name):
    s = _detok(name)
    sem = s["sem_d"].clone()
    for b, n in enumerate(K.TOKEN_LENGTHS):
        sem[b, n:] = -1
        sem[b, n + 1::2] = s["spec"].codebook_size + 5
    assert torch.equal(s["m"].detokenize(sem, s["glob_d"], lengths=K.TOKEN_LENGTHS), s["wav"])


def test_features_and_samples_behind_a_clip_are_never_read(qa_lib, gpu_device):
    import unified_audio_amd as qa

    s = _semantic()
    feat = s["feat_d"].clone()
    for b, n in enumerate(K.TOKEN_LENGTHS):
        feat[b, n:] = float("nan")
    assert torch.equal(s["m"].get_semantic_tokens({"feat": feat}, lengths=K.TOKEN_LENGTHS), s["tok"])
    t = _tokenizer()
    wav = t["wav_d"].clone()
    for b, n in enumerate(K.SAMPLE_LENGTHS):
        wav[b, n:] = float("nan")
    glob, sem = t["tok"].tokenize(wav, lengths=K.SAMPLE_LENGTHS)
    assert torch.equal(glob, t["glob"]) and torch.equal(sem, t["sem"])
    assert torch.equal(qa.wav_normalize(wav, lengths=K.SAMPLE_LENGTHS), qa.wav_normalize(t["wav_d"], lengths=K.SAMPLE_LENGTHS))
    assert torch.equal(t["m"].get_global_tokens({"ref_wav": wav}, K.REF_LEN, lengths=K.SAMPLE_LENGTHS), t["glob"])


# ------------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize("name", sorted(K.DSPECS))
def test_a_detokenize_row_equals_itself_alone_bit_for_bit(qa_lib, gpu_device, name):
    s = _detok(name)
    m, sem, glob, hop = s["m"], s["sem_d"], s["glob_d"], s["spec"].hop
    B, Tm = sem.shape
    for b, n in enumerate(K.TOKEN_LENGTHS):
        alone = m.detokenize(sem[b:b + 1, :n].contiguous(), glob[b:b + 1])
        assert torch.equal(s["wav"][b, 0, :n * hop], alone[0, 0]), f"row {b} ({n} tokens) differs from the rectangular call on the clip alone"
    order = list(range(B))[::-1]  # another row, other neighbours, a longer T, other tokens behind
    wide = torch.full((B, Tm + 11), 3, dtype=torch.int64, device=sem.device)
    wide[:, :Tm] = sem[order]
    other = m.detokenize(wide, glob[order], lengths=[K.TOKEN_LENGTHS[i] for i in order])
    for row, b in enumerate(order):
        n = K.TOKEN_LENGTHS[b]
        assert torch.equal(other[row, 0, :n * hop], s["wav"][b, 0, :n * hop]), f"clip {b} at row {row} of a longer batch"
        assert _zeros(other[row, 0, n * hop:])
    pair = m.detokenize(sem[2:4, :K.TOKEN_LENGTHS[2]].contiguous(), glob[2:4], lengths=K.TOKEN_LENGTHS[2:4])
    for row, b in enumerate((2, 3)):
        n = K.TOKEN_LENGTHS[b]
        assert torch.equal(pair[row, 0, :n * hop], s["wav"][b, 0, :n * hop]), f"clip {b} in a batch of two"


def test_a_semantic_row_equals_itself_alone_bit_for_bit(qa_lib, gpu_device):
    s = _semantic()
    m, feat = s["m"], s["feat_d"]
    B, Nm, Cin = feat.shape
    for b, n in enumerate(K.TOKEN_LENGTHS):
        alone = m.get_semantic_tokens({"feat": feat[b:b + 1, :n].contiguous()})
        assert torch.equal(s["tok"][b, :n], alone[0]), b
    order = list(range(B))[::-1]
    wide = torch.full((B, Nm + 9, Cin), 0.5, device=feat.device)
    wide[:, :Nm] = feat[order]
    other = m.get_semantic_tokens({"feat": wide}, lengths=[K.TOKEN_LENGTHS[i] for i in order])
    for row, b in enumerate(order):
        n = K.TOKEN_LENGTHS[b]
        assert torch.equal(other[row, :n], s["tok"][b, :n]) and bool((other[row, n:] == -1).all()), (row, b)


def test_normalisation_and_global_rows_equal_themselves_alone_bit_for_bit(qa_lib, gpu_device):
    import unified_audio_amd as qa

    t = _tokenizer()
    m, wav = t["m"], t["wav_d"]
    B, Tm = wav.shape
    norm = qa.wav_normalize(wav, lengths=K.SAMPLE_LENGTHS)
    glob = m.get_global_tokens({"ref_wav": wav}, K.REF_LEN, lengths=K.SAMPLE_LENGTHS)
    assert torch.equal(glob, t["glob"])  # tokenize's global half is this call
    for b, n in enumerate(K.SAMPLE_LENGTHS):
        clip = wav[b:b + 1, :n].contiguous()
        assert torch.equal(norm[b, :n], qa.wav_normalize(clip)[0]) and _zeros(norm[b, n:]), b
        assert torch.equal(glob[b], m.get_global_tokens({"ref_wav": clip}, K.REF_LEN)[0]), b
        assert torch.equal(glob[b], m.get_global_tokens({"ref_wav": T.ref_clip(clip.cpu(), K.REF_LEN).to(DEV)})[0]), b
    order = list(range(B))[::-1]
    wide = torch.full((B, Tm + 333), 0.25, device=wav.device)
    wide[:, :Tm] = wav[order]
    lens = [K.SAMPLE_LENGTHS[i] for i in order]
    norm2 = qa.wav_normalize(wide, lengths=lens)
    glob2 = m.get_global_tokens({"ref_wav": wide}, K.REF_LEN, lengths=lens)
    for row, b in enumerate(order):
        n = K.SAMPLE_LENGTHS[b]
        assert torch.equal(norm2[row, :n], norm[b, :n]) and _zeros(norm2[row, n:]), (row, b)
        assert torch.equal(glob2[row], glob[b]), (row, b)


# ------------------------------------------------------------------------------------------------ 4
def test_equal_lengths_are_the_rectangular_call(qa_lib, gpu_device):
    import unified_audio_amd as qa

    s, e, t = _detok("small"), _semantic(), _tokenizer()
    B, Tm = s["sem_d"].shape
    assert torch.equal(s["m"].detokenize(s["sem_d"], s["glob_d"], lengths=[Tm] * B), s["m"].detokenize(s["sem_d"], s["glob_d"]))
    batch = {"feat": e["feat_d"]}
    assert torch.equal(e["m"].get_semantic_tokens(batch, lengths=[Tm] * B), e["m"].get_semantic_tokens(batch))
    wav, m = t["wav_d"], t["m"]
    Tw = wav.shape[1]
    assert torch.equal(qa.wav_normalize(wav, lengths=[Tw] * B), qa.wav_normalize(wav))
    for ref_len in (K.REF_LEN, 0):  # without a reference length only the rectangular call exists
        assert torch.equal(m.get_global_tokens({"ref_wav": wav}, ref_len, lengths=torch.tensor([Tw] * B)), m.get_global_tokens({"ref_wav": wav}, ref_len))
    feat = t["fx"](qa.wav_normalize(wav))
    full = {"feat": feat, "ref_wav": wav}
    a = m.tokenize(full, K.REF_LEN, lengths=[Tw] * B, frame_lengths=[feat.shape[1]] * B)
    b = m.tokenize(full, K.REF_LEN)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ------------------------------------------------------------------------------------------------ 5
def test_bad_lengths_are_refused_before_any_launch(qa_lib, gpu_device):
    import unified_audio_amd as qa

    s, e, t = _detok("small"), _semantic(), _tokenizer()
    m, sem, glob = s["m"], s["sem_d"], s["glob_d"]
    B, Tm = sem.shape
    before = m.detokenize(sem, glob)
    tok_before = e["m"].get_semantic_tokens({"feat": e["feat_d"]})
    calls = {
        "detokenize": lambda lens: m.detokenize(sem, glob, lengths=lens),
        "semantic": lambda lens: e["m"].get_semantic_tokens({"feat": e["feat_d"]}, lengths=lens),
    }
    for name, call in calls.items():
        for row, value in ((0, 0), (1, Tm + 1), (3, -5)):
            lens = [Tm] * B
            lens[row] = value
            with pytest.raises(qa.QuarkAudioError) as err:
                call(lens)
            assert err.value.status == -1 and f"lengths[{row}] = {value}" in str(err.value), (name, str(err.value))
        for lens in ([Tm] * (B - 1), [Tm] * (B + 1)):
            with pytest.raises(qa.QuarkAudioError) as err:
                call(lens)
            assert err.value.status == -1 and f"{len(lens)} entries" in str(err.value), (name, str(err.value))
    # the library's own check, for callers of the C-ABI: the same words, before anything is launched
    wav = torch.empty(B, 1, Tm * s["spec"].hop, device=DEV)
    for row, value in ((2, 0), (1, Tm + 1), (0, -1)):
        lens = [Tm] * B
        lens[row] = value
        st = qa_lib.qa_bicodec_detokenize_ragged(m._handle, sem.data_ptr(), glob.reshape(B, -1).contiguous().data_ptr(), B, Tm, (C.c_int64 * B)(*lens),
                                                 wav.data_ptr(), torch.cuda.current_stream().cuda_stream)
        msg = qa_lib.qa_last_error().decode()
        assert st == -1 and f"qa_bicodec_detokenize_ragged: lengths[{row}] = {value} is outside 1 .. T = {Tm}" in msg, msg
    # samples: 400 make the first frame
    Tw = t["wav_d"].shape[1]
    for row, value in ((3, 399), (0, Tw + 1), (2, 0)):
        lens = list(K.SAMPLE_LENGTHS)
        lens[row] = value
        n_calls = len(t["calls"])
        with pytest.raises(qa.QuarkAudioError) as err:
            t["tok"].tokenize(t["wav_d"], lengths=lens)
        assert err.value.status == -1 and f"lengths[{row}] = {value}" in str(err.value), str(err.value)
        assert len(t["calls"]) == n_calls  # refused in front of the front-end call
    with pytest.raises(qa.QuarkAudioError) as err:  # clips of different lengths have no common "rows as they are"
        t["m"].get_global_tokens({"ref_wav": t["wav_d"]}, 0, lengths=K.SAMPLE_LENGTHS)
    assert err.value.status == -1 and "ref_len" in str(err.value)
    # a live token out of range is still an IndexError; one behind a clip's end is not
    junk = sem.clone()
    junk[1, K.TOKEN_LENGTHS[1] - 1] = s["spec"].codebook_size
    with pytest.raises(IndexError):
        m.detokenize(junk, glob, lengths=K.TOKEN_LENGTHS)
    torch.cuda.synchronize()
    assert torch.equal(m.detokenize(sem, glob), before)
    assert torch.equal(e["m"].get_semantic_tokens({"feat": e["feat_d"]}), tok_before)
    assert torch.equal(m.detokenize(sem, glob, lengths=K.TOKEN_LENGTHS), s["wav"])


# ------------------------------------------------------------------------------------------------ 6
def test_the_tokenizer_makes_one_call_of_each_kind_and_equals_the_per_clip_loop(qa_lib, gpu_device):
    t = _tokenizer()
    tok, wav = t["tok"], t["wav_d"]
    B, Tw = wav.shape
    assert t["first_calls"] == [((B, Tw), list(K.SAMPLE_LENGTHS))], t["first_calls"]
    frames = tok.token_frames(K.SAMPLE_LENGTHS)
    assert frames == list(K.FRAMES)
    assert t["sem"].shape == (B, t["fx"].frames(Tw)) and t["sem"].dtype == torch.int64
    for b, n in enumerate(K.SAMPLE_LENGTHS):
        g1, s1 = tok.tokenize(wav[b:b + 1, :n].contiguous())
        assert s1.shape == (1, frames[b])
        assert torch.equal(t["sem"][b, :frames[b]], s1[0]) and bool((t["sem"][b, frames[b]:] == -1).all()), b
        assert torch.equal(t["glob"][b], g1[0]), b


def test_round_trip_with_lengths_equals_the_per_clip_round_trip(qa_lib, gpu_device):
    t = _tokenizer()
    tok, wav = t["tok"], t["wav_d"]
    hop = t["dspec"].hop
    frames = tok.token_frames(K.SAMPLE_LENGTHS)
    out = tok.detokenize(t["glob"], t["sem"], lengths=frames)
    assert out.shape == (len(frames), 1, t["sem"].shape[1] * hop)
    for b, n in enumerate(K.SAMPLE_LENGTHS):
        g1, s1 = tok.tokenize(wav[b:b + 1, :n].contiguous())
        one = tok.detokenize(g1, s1)
        assert torch.equal(out[b, 0, :frames[b] * hop], one[0, 0]) and _zeros(out[b, 0, frames[b] * hop:]), b


# ------------------------------------------------------------------------------------------------ 7
def test_published_widths_short_backbone(qa_lib, gpu_device):
    """Every kernel shape of the published configuration (tests/test_bicodec_gpu.py::test_published_widths_short_backbone: 1024-wide
    latents, 384 / 2048 Vocos, the 1536-channel generator at rates 8, 5, 4, 2) with a 2-layer backbone; lengths (50, 23)."""
    import unified_audio_amd as qa

    c = K.published_case()
    spec, espec, sd, sem, glob, lens = c["spec"], c["espec"], c["sd"], c["sem"], c["glob"], K.PUBLISHED_LENGTHS
    m = qa.BiCodec(qa.BiCodecSpec(**K.fields(spec)), device=DEV, encoder_spec=espec).load_state_dict(sd).enable_taps()
    got = m.detokenize(sem.to(DEV), glob.to(DEV), lengths=lens)
    names = TAPS + tuple(f"gen.block{i}" for i in range(len(spec.rates)))
    taps = {k: m.tap(k) for k in names}
    sd64 = T.cast(sd)
    bad = []
    for b, n in enumerate(lens):
        ot = {}
        with torch.no_grad():
            want = K.detokenize64(sd64, sem[b:b + 1, :n], glob[b:b + 1], spec, ot)[0, 0]
        ref = K.oracle_detok_taps(sd64, spec, ot)
        report = {}
        for k, v in taps.items():
            rate = v.numel() // (2 * max(lens) * ref[k].shape[1])
            report[k] = rel_err(v.reshape(2, max(lens) * rate, -1)[b, :n * rate].cpu(), ref[k].float())
        report["wav"] = rel_err(got[b, 0, :n * spec.hop].cpu(), want.float())
        print(f"BICODEC-RAGGED published widths clip {b} ({n} tokens): " + " ".join(f"{k} {v:.2e}" for k, v in report.items()))
        bad += [f"clip {b} {k}: {v:.3e}" for k, v in report.items() if not v < 2 * K.STAGE_TOL]
        assert _zeros(got[b, 0, n * spec.hop:])
        alone = m.detokenize(sem[b:b + 1, :n].to(DEV), glob[b:b + 1].to(DEV))
        assert torch.equal(got[b, 0, :n * spec.hop], alone[0, 0]), b
    assert not bad, "\n".join(bad)
    # the encoder at its published widths: rows against the oracle's audit and the clip alone
    feat = c["feat"]
    tok = m.get_semantic_tokens({"feat": feat.to(DEV)}, lengths=lens)
    cb = T.normalized_codebook(sd).float().numpy()[None]
    for b, n in enumerate(lens):
        ref = c["alone"][b]
        flips = audit_codes(ref["latent"].float().numpy(), cb, tok[b, :n].reshape(-1, 1).cpu().numpy(), ref["tokens"].reshape(-1, 1).numpy())
        assert flips <= K.FLIP_CAP and bool((tok[b, n:] == -1).all()), (b, flips)
        assert torch.equal(tok[b, :n], m.get_semantic_tokens({"feat": feat[b:b + 1, :n].to(DEV)})[0]), b
