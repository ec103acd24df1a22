"""SSL front-end with per-clip lengths in one call (qa_ssl_forward_ragged through SSLFeatureExtractor(wavs, lengths=...), DESIGN.md
section 27): row b of a ragged call is the clip wav[b, :lengths[b]] alone - against the CPU oracle on that clip, and bit for bit against
the rectangular call on that clip.

Small specs: the three of tests/test_ssl_gpu.py (GroupNorm + post-LN at hd 32, LayerNorm + stable-LN at hd 64, WavLM's gated bias).
Lengths in samples, longest first: 320 * 140 + 57 (140 frames: crosses the 128-query tile), 320 * 66 (66 frames: a 2-key tail in the
third 32-key tile), 320 * 34 + 123 (35 frames by the extractor's floor rule: a 3-key tail in the second tile), 200 (one frame: one
key, one positional-conv row; its 103 layer-0 frames end inside the second 64-frame conv0 chunk) and, added to those four, 320 * 34 (34
frames: the 2-key tail in the second tile).  None of 57, 123, 200 is a multiple of the layer-0 stride 5.

    1  every row against the oracle on the clip alone (the bounds of tests/test_ssl_gpu.py), exact zeros behind its frames
    2  NaN behind every clip's end changes nothing
    3  a row == the clip alone == itself at another row, among other neighbours, inside a longer T; both attention forms
    4  lengths = [T] * B is the rectangular call: same bits, same launches, no KMASK instance; a ragged call masks n_layers launches
    5  bad lengths are refused before any launch, naming row and value
    6  attention_kernel<HD, BIAS, KMASK> through qa_debug_attention_bias_kmask against a float64 masked-softmax truth
    7  the real widths (HuBERT-base, WavLM-base+, XLSR), 2 layers each
    8  the callers: HCodecTokenizer.tokenize(lengths=...) and UniSE._enroll_features make ONE front-end call
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import functools

import pytest
import torch

from oracle import ssl_ref as S
from tests.test_attention_gpu import (C_PARITY, E_FLOOR, OUT_HEAD, S_ULP, Case, _seed, launch, make_inputs, pack, scores)
from tests.util import check_guarded_out, guarded_out, rel_err, with_knob

pytestmark = pytest.mark.gpu

TOL = 5e-5  # tests/test_ssl_gpu.py: relative RMS on the uncompressed hidden-state average
CTOL = 1e-3  # ... and the compressed features in absolute terms, away from sign flips of tiny means

SMALL = dict(conv_dim=(64,) * 7, num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=2)
SPECS = {
    "group_post_ln": (S.SSLSpec(**SMALL, hidden_size=96, num_hidden_layers=3, num_attention_heads=3, intermediate_size=192), "hubert"),
    "layer_stable_ln": (S.SSLSpec(**SMALL, hidden_size=128, num_hidden_layers=3, num_attention_heads=2, intermediate_size=256, conv_bias=True,
                                  feat_extract_norm="layer", do_stable_layer_norm=True, select=(1, 3)), "wav2vec2"),
    "wavlm": (S.SSLSpec(**SMALL, hidden_size=96, num_hidden_layers=3, num_attention_heads=3, intermediate_size=192, num_buckets=16,
                        max_bucket_distance=10), "wavlm"),
}
LENGTHS = (320 * 140 + 57, 320 * 66, 320 * 34 + 123, 200, 320 * 34)
# 2 layers at the real widths: the 512-channel extractor, the k128 / 16-group positional convolution, hd 64
WIDE = {
    "hubert_base": (dataclasses.replace(S.SPEC_HUBERT_BASE, num_hidden_layers=2), "hubert"),
    "wavlm_base_plus": (dataclasses.replace(S.SPEC_WAVLM_BASE_PLUS, num_hidden_layers=2, compress_exponent=0.3), "wavlm"),
    "xlsr": (dataclasses.replace(S.SPEC_XLSR53, num_hidden_layers=2, select=(1, 2)), "wav2vec2"),
}
WIDE_LENGTHS = (16000, 9923)


def _extractor(ospec, sd, expo, device):
    import unified_audio_amd as qa

    kw = {f: getattr(ospec, f) for f in ospec.__dataclass_fields__}
    return qa.SSLFeatureExtractor(qa.SSLSpec(**{**kw, "compress_exponent": expo}), device=device).load_state_dict(sd)


@functools.lru_cache(maxsize=None)
def _setup(name, seed=3):
    """Per spec, once per session: weights, a [B, T] batch whose rows hold other (finite) samples behind every clip's end, the
    oracle's features of every clip ALONE, plain and compressed, and the two extractors.  Shared by the tests; never modified."""
    ospec, kind = (SPECS.get(name) or WIDE[name])
    lengths = LENGTHS if name in SPECS else WIDE_LENGTHS
    device = torch.device("cuda:0")
    sd = S.synth_state_dict(seed, ospec, kind)
    T = max(lengths)
    g = torch.Generator().manual_seed(seed + 10)
    wav = torch.randn(len(lengths), T, generator=g) * 0.2 + 0.05 * torch.sin(torch.arange(T) * 0.03)[None]
    expos = (0.0, ospec.compress_exponent)
    refs = {}
    with torch.no_grad():
        for expo in expos:
            spec = dataclasses.replace(ospec, compress_exponent=expo)
            refs[expo] = [S.extract_features(sd, wav[b:b + 1, :n], spec)[0] for b, n in enumerate(lengths)]
    fx = {expo: _extractor(ospec, sd, expo, device) for expo in expos}
    return dict(spec=ospec, lengths=list(lengths), wav=wav.to(device), refs=refs, fx=fx, expos=expos)


def _check_rows_against_oracle(s, got):
    """got[expo] [B, N, d] of a ragged call: per clip the two errors of tests/test_ssl_gpu.py, and exact zeros behind its frames."""
    plain, comp = s["expos"]
    fx = s["fx"][plain]
    bad = []
    for b, n in enumerate(s["lengths"]):
        nb = fx.frames(n)
        ref0, ref1 = s["refs"][plain][b], s["refs"][comp][b]
        assert ref0.shape == (nb, s["spec"].hidden_size)
        g0, g1 = got[plain][b].cpu(), got[comp][b].cpu()
        assert torch.isfinite(g0).all() and torch.isfinite(g1).all()
        err = rel_err(g0[:nb], ref0)
        far = ref0.abs() > 1e-3
        cerr = float((g1[:nb] - ref1)[far].abs().max())
        print(f"SSL-RAGGED clip {b}: {n} samples, {nb} frames: err {err:.3e} cerr {cerr:.3e}")
        if not (err < TOL and cerr < CTOL):
            bad.append(f"clip {b} ({n} samples): err {err:.3e} (bound {TOL}), cerr {cerr:.3e} (bound {CTOL})")
        for g_ in (g0, g1):
            if not torch.equal(g_[nb:], torch.zeros_like(g_[nb:])):
                bad.append(f"clip {b}: the rows behind frame {nb} are not exactly 0")
    assert not bad, "\n".join(bad)


@functools.lru_cache(maxsize=None)
def _run1(name):
    s = _setup(name)
    out = {expo: s["fx"][expo](s["wav"], lengths=s["lengths"]) for expo in s["expos"]}
    torch.cuda.synchronize()
    return out


# ------------------------------------------------------------------------------------------------ 1, 2
@pytest.mark.parametrize("name", sorted(SPECS))
def test_every_row_matches_the_oracle_on_the_clip_alone(qa_lib, gpu_device, name):
    s = _setup(name)
    got = _run1(name)
    T = max(s["lengths"])
    assert all(g.shape == (len(s["lengths"]), s["fx"][0.0].frames(T), s["spec"].hidden_size) for g in got.values())
    _check_rows_against_oracle(s, got)


@pytest.mark.parametrize("name", sorted(SPECS))
def test_what_lies_behind_a_clip_is_never_read(qa_lib, gpu_device, name):
    s = _setup(name)
    wav = s["wav"].clone()
    for b, n in enumerate(s["lengths"]):
        wav[b, n:] = float("nan")
    for expo in s["expos"]:
        got = s["fx"][expo](wav, lengths=s["lengths"])
        assert torch.equal(got, _run1(name)[expo]), expo


# ------------------------------------------------------------------------------------------------ 3
def _check_row_invariance(s, fx):
    wav, lengths = s["wav"], s["lengths"]
    B, T = wav.shape
    batch = fx(wav, lengths=lengths)
    frames = [fx.frames(n) for n in lengths]
    for b, n in enumerate(lengths):
        alone = fx(wav[b:b + 1, :n].contiguous())
        assert alone.shape[1] == frames[b]
        assert torch.equal(batch[b, :frames[b]], alone[0]), f"row {b} ({n} samples) differs from the clip alone"
    # the rows in reverse order (another row, other neighbours), inside a longer T, behind other samples
    order = list(range(B))[::-1]
    wide = torch.full((B, T + 997), 0.25, device=wav.device)
    wide[:, :T] = wav[order]
    other = fx(wide, lengths=[lengths[i] for i in order])
    assert other.shape[1] == fx.frames(T + 997)
    for row, b in enumerate(order):
        assert torch.equal(other[row, :frames[b]], batch[b, :frames[b]]), f"clip {b} at row {row} of a longer batch"
        assert not other[row, frames[b]:].any()
    # two clips alone together
    pair = fx(wav[2:4, :lengths[2]].contiguous(), lengths=lengths[2:4]) if B >= 4 else None
    if pair is not None:
        for row, b in enumerate((2, 3)):
            assert torch.equal(pair[row, :frames[b]], batch[b, :frames[b]]), f"clip {b} in a batch of two"


@pytest.mark.parametrize("math", (0, 1))
@pytest.mark.parametrize("name", sorted(SPECS))
def test_a_row_equals_itself_alone_bit_for_bit(qa_lib, gpu_device, name, math):
    s = _setup(name)
    with with_knob("QA_ATT_MATH", math):
        _check_row_invariance(s, s["fx"][0.0])


# ------------------------------------------------------------------------------------------------ 4
def _att_counts(lib):
    out = (C.c_int64 * 2)()
    assert lib.qa_debug_att_stats(out) == 0
    lib.qa_debug_att_kmask_launches.restype = C.c_longlong
    return int(out[0]) + int(out[1]), int(lib.qa_debug_att_kmask_launches())


@pytest.mark.parametrize("name", sorted(SPECS))
def test_equal_lengths_are_the_rectangular_call(qa_lib, gpu_device, name):
    s = _setup(name)
    fx, wav = s["fx"][s["expos"][1]], s["wav"]
    B, T = wav.shape
    n_layers = s["spec"].num_hidden_layers
    c0 = _att_counts(qa_lib)
    rect = fx(wav)
    c1 = _att_counts(qa_lib)
    full = fx(wav, lengths=[T] * B)
    c2 = _att_counts(qa_lib)
    assert torch.equal(full, rect)
    assert (c1[0] - c0[0], c1[1] - c0[1]) == (n_layers, 0)
    assert (c2[0] - c1[0], c2[1] - c1[1]) == (n_layers, 0), "a call whose clips fill their rows took a masked kernel"
    fx(wav, lengths=torch.tensor(s["lengths"]))
    c3 = _att_counts(qa_lib)
    assert (c3[0] - c2[0], c3[1] - c2[1]) == (n_layers, n_layers), "a ragged call masks every attention launch, and adds none"


# ------------------------------------------------------------------------------------------------ 5
def test_bad_lengths_are_refused_before_any_launch(qa_lib, gpu_device):
    import unified_audio_amd as qa

    s = _setup("group_post_ln")
    fx, wav = s["fx"][0.0], s["wav"][:2].contiguous()
    T = wav.shape[1]
    # the shortest input that yields one frame with the 10,3,3,3,3,2,2 / 5,2,2,2,2,2,2 extractor and 160 + 160 samples of padding
    assert fx.frames(80) == 1
    with pytest.raises(qa.QuarkAudioError):
        fx.frames(79)
    before = _att_counts(qa_lib)
    for row, value in ((0, 0), (1, T + 1), (1, 79), (0, -5)):
        lens = [T, T]
        lens[row] = value
        with pytest.raises(qa.QuarkAudioError) as e:
            fx(wav, lengths=lens)
        assert e.value.status == -1 and f"lengths[{row}] = {value}" in str(e.value), str(e.value)
    for lens in ([T], [T, T, T]):
        with pytest.raises(qa.QuarkAudioError) as e:
            fx(wav, lengths=lens)
        assert e.value.status == -1 and f"{len(lens)} entries" in str(e.value), str(e.value)
    torch.cuda.synchronize()
    assert _att_counts(qa_lib) == before
    assert fx(wav, lengths=[T, 80]).shape == (2, fx.frames(T), s["spec"].hidden_size)  # the handle still works; 80 samples are one frame


# ------------------------------------------------------------------------------------------------ 6
def _bias_kmask_launch(lib, c, p, valid):
    fn = lib.qa_debug_attention_bias_kmask
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_int,
                   C.c_longlong, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    ldo = c.d + 4
    buf, out = guarded_out(c.B * c.n_q, c.d, ldo, OUT_HEAD, torch.device("cuda"))
    st = fn(p.q, p.ldq, p.k, p.v, p.ldkv, out.data_ptr(), ldo, c.B, c.n_q, c.n_keys, p.kv_bstride, c.H, c.hd, c.hd ** -0.5, p.gate,
            p.relbias, c.R, valid.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert st == 0, lib.qa_last_error()
    torch.cuda.synchronize()
    check_guarded_out(buf, out, OUT_HEAD)
    return out.reshape(c.B, c.n_q, c.H, c.hd).clone()


def _masked_truth(c, x, valid, dtype):
    """softmax(scale Q K^T + gate * bias, keys outside `valid` [B, n_keys] at -inf) V in `dtype` -> ([B, n_q, H, hd], scores)."""
    s = scores(c, x, dtype, torch.arange(c.n_q)).masked_fill(~valid.view(c.B, 1, 1, c.n_keys), float("-inf"))
    p = torch.exp(s - s.amax(-1, keepdim=True))
    return ((p @ x["v"].transpose(1, 2).to(dtype)) / p.sum(-1, keepdim=True)).transpose(1, 2), s


BIAS_KMASK = {70: (70, 33, 1), 129: (129, 128, 31)}  # n -> valid keys per batch item


@pytest.mark.parametrize("n", sorted(BIAS_KMASK))
@pytest.mark.parametrize("hd", (32, 64))
def test_gated_bias_under_a_key_padding_mask(qa_lib, gpu_device, hd, n):
    """The masked keys' K / V rows hold ordinary numbers (the kernel reads them and multiplies by p = 0); the rows outside every buffer,
    the gate past its end and the rows around the bias table are NaN (tests/test_attention_gpu.pack)."""
    counts = BIAS_KMASK[n]
    c = Case("bias", B=len(counts), H=3, hd=hd, n_q=n, n_keys=n, R=20, buckets=64)
    x = make_inputs(c, "randn", _seed(c, "bias_kmask"))
    valid = torch.arange(n).view(1, -1) < torch.tensor(counts).view(-1, 1)
    p = pack(c, x, gpu_device)
    vbytes = valid.to(torch.uint8).contiguous().to(gpu_device)
    t64, s64 = _masked_truth(c, x, valid, torch.float64)
    t32, _ = _masked_truth(c, x, valid, torch.float32)
    scale = float(t64.abs().max())
    e_cpu = float((t32.double() - t64).abs().max()) / scale
    s_max = float(s64[torch.isfinite(s64)].abs().max())
    bound = C_PARITY * max(e_cpu, E_FLOOR, S_ULP * s_max)
    lib = qa_lib
    lib.qa_debug_att_kmask_launches.restype = C.c_longlong
    bad = []
    for math in (0, 1):
        with with_knob("QA_ATT_MATH", math):
            k0 = int(lib.qa_debug_att_kmask_launches())
            out = _bias_kmask_launch(lib, c, p, vbytes)
            assert int(lib.qa_debug_att_kmask_launches()) == k0 + 1
            e = float((out.cpu().double() - t64).abs().max()) / scale
            print(f"ATTN-BIAS-KMASK math{math} hd{hd} n{n}: e_hip {e:.3e} e_cpu32 {e_cpu:.3e} bound {bound:.3e} frac {e / bound:.3f}")
            if not e <= bound:
                bad.append(f"QA_ATT_MATH={math}: e_hip {e:.3e} > bound {bound:.3e} (e_cpu32 {e_cpu:.3e})")
            # an item with v valid keys == the existing bias launch on its first v rows alone
            for b, v in enumerate(counts):
                c1 = dataclasses.replace(c, B=1, n_q=v, n_keys=v)
                x1 = dict(q=x["q"][b:b + 1, :v].contiguous(), k=x["k"][b:b + 1, :v].contiguous(), v=x["v"][b:b + 1, :v].contiguous(),
                          gate=x["gate"][b:b + 1, :, :v].contiguous(), emb=x["emb"])
                alone = launch(lib, c1, pack(c1, x1, gpu_device))
                if not torch.equal(out[b, :v], alone[0]):
                    bad.append(f"QA_ATT_MATH={math}: item {b} ({v} valid keys of {n}) differs from the bias launch at n = {v}")
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------ 7
@pytest.mark.parametrize("name", sorted(WIDE))
def test_real_widths(qa_lib, gpu_device, name):
    s = _setup(name)
    _check_rows_against_oracle(s, _run1(name))
    for math in (0, 1):
        with with_knob("QA_ATT_MATH", math):
            _check_row_invariance(s, s["fx"][s["expos"][1]])


# ------------------------------------------------------------------------------------------------ 8
def test_tokenize_with_lengths_makes_one_front_end_call(qa_lib, gpu_device):
    import unified_audio_amd as qa
    from oracle import hcodec_ref as R
    from oracle import synth
    from tests.util import MINI

    calls = []

    class Spy(qa.SSLFeatureExtractor):
        def __call__(self, wavs, lengths=None):
            calls.append((tuple(wavs.shape), None if lengths is None else list(lengths)))
            return super().__call__(wavs, lengths=lengths)

    sspec = S.SSLSpec(conv_dim=(64,) * 7, hidden_size=64, num_hidden_layers=2, num_attention_heads=2, intermediate_size=128,
                      num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=1)
    fx = Spy(qa.SSLSpec(**{f: getattr(sspec, f) for f in sspec.__dataclass_fields__}), device=gpu_device)
    fx.load_state_dict(S.synth_state_dict(9, sspec))
    # a codec whose frame rates match the extractor (tests/test_ssl_gpu.py): hop 640 = 2 * prod(ratios)
    kw = dict(MINI, ratios=(8, 5, 4, 2), dimension=512, code_dim=512, enc_heads=8, hop=320, n_fft=1280)
    tok = qa.HCodecTokenizer(state_dict=synth.hcodec10_state_dict(13, R.HCodecSpec(**kw)), feature_extractor=fx, device=gpu_device,
                             spec=qa.HCodecSpec(**kw))
    lens = [640 * 12 - 100, 640 * 5 + 1, 640 * 9, 640 * 5 - 7]  # 12, 6, 9, 5 code frames
    frames = tok.code_frames(lens)
    assert frames == [12, 6, 9, 5]
    wav = synth.synth_wav(14, len(lens), max(lens)).to(gpu_device)
    ac, sc = tok.tokenize(wav, lengths=lens)
    assert calls == [((len(lens), 640 * 12), [640 * f for f in frames])], calls
    # the same codes from the features of every clip alone (each padded to its own hop multiple, as tokenize pads a clip)
    feats = torch.zeros(len(lens), 2 * 12, sspec.hidden_size, device=gpu_device)
    for b, n in enumerate(lens):
        feats[b, :2 * frames[b]] = fx(tok.pad_wav(wav[b:b + 1, :n]))[0]
    ac2, sc2 = tok.tokenize(wav, feats=feats, lengths=lens)
    assert torch.equal(ac, ac2) and torch.equal(sc, sc2)
    assert ac.shape[-1] == 12 and bool((ac[1, :, 6:] == -1).all()) and bool((ac[1, :, :6] >= 0).all())


def test_unise_enrollments_of_mixed_lengths_make_one_front_end_call(qa_lib, gpu_device):
    from unified_audio_amd import unise as U

    s = _setup("wavlm")
    fx = s["fx"][0.0]
    calls = []

    class Spy:
        frames = fx.frames

        def __call__(self, wavs, lengths=None):
            calls.append(tuple(wavs.shape))
            return fx(wavs, lengths=lengths)

    class NoLM:
        def generate(self, task_name, enroll_mel, enroll_feats, mix_mel, mix_feats, do_sample, enroll_lengths=None):
            raise AssertionError("not called")

    drv = U.UniSE(NoLM(), Spy())
    assert drv._ssl_ragged_ok
    g = torch.Generator().manual_seed(2)
    enrs = [(torch.randn(1, n, generator=g) * 0.1).to(gpu_device) for n in (8000, 12001, 8000, 20000, 200)]
    ef, n_enr, frames = drv._enroll_features(enrs)
    assert calls == [(5, 20000)] and n_enr == 20000
    calls.clear()
    drv._ssl_ragged_ok = False  # the loop over distinct lengths, as for a front-end without the keyword
    ef2, n2, frames2 = drv._enroll_features(enrs)
    assert sorted(calls) == [(1, 200), (1, 12001), (1, 20000), (2, 8000)]
    assert (n_enr, frames) == (n2, frames2) and frames == [fx.frames(e.size(-1)) for e in enrs]
    assert torch.equal(ef, ef2)
