"""Per-clip lengths in one H-Codec 1.5 encode / decode call (Codec.encode_ragged / decode_ragged, qa_hcodec_encode_adaptive_ragged /
_decode_adaptive_ragged): row b of a per-clip call is the rectangular call on that clip alone, as B = 1, at its own
length, with its own group count and no padded query token among its keys."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

from oracle import hcodec15_ref as R15
from oracle import hcodec_ref as R
from oracle import synth
from tests.util import MINI, audit_codes_bnq, rel_err, with_knob

pytestmark = pytest.mark.gpu

# The shapes of tests/test_hcodec_ragged_gpu.py: 140 decoder frames cross the 128-query attention tile, one code frame is the reflect
# short-input case and the single-group case.  On the CPU oracle the clips give 12 / 6 / 5 / 1 groups of 1 .. 8 frames, so the interleaved
# aggregator rows run from 82 keys (70 + 12) down to 2 (1 + 1), under one mask of 82 columns.
FRAMES = [70, 33, 17, 1]
N = 70
HOP = 640
THR = 0.7
INVALID, UNSUPPORTED = -1, -4


def _att_launches(qa_lib):
    """(attention launches so far, those of them that took a key-padding-mask instantiation)"""
    out = (C.c_int64 * 2)()
    assert qa_lib.qa_debug_att_stats(out) == 0
    fn = qa_lib.qa_debug_att_kmask_launches
    fn.restype, fn.argtypes = C.c_longlong, []
    return out[0] + out[1], int(fn())


def _token_lengths(sc, K):
    return torch.div(sc[:, 0], K, rounding_mode="floor") + 1


@pytest.fixture(scope="module")
def full(qa_lib, gpu_device):
    """SPEC_15 with one aggregator / bottleneck layer at threshold 0.7, the oracle on every clip ALONE at its own length (computed once, never
    modified), and the per-clip call's outputs on clean inputs (run 1)."""
    import unified_audio_amd as qa

    ospec = dataclasses.replace(R.SPEC_15, agg_layers=1, bt_layers=1, threshold=THR)
    sd = synth.hcodec10_state_dict(1234, ospec)
    fields = {f: getattr(ospec, f) for f in ospec.__dataclass_fields__}
    codec = qa.Codec(None, None, None, spec=qa.HCodecSpec(**fields), device=gpu_device).load_state_dict(sd)
    wav, feat = synth.synth_wav(7, 4, HOP * N), synth.synth_feat(9, 4, 2 * N, 1024)
    alone = []
    for b, f in enumerate(FRAMES):
        taps = {}
        o = R15.encode(sd, wav[b:b + 1, None, :HOP * f], feat[b:b + 1, :, :2 * f], ospec, taps)
        alone.append(dict(ac=o["acoustic_codes"], sc=o["semantic_codes"], emb=taps["enc.emb_agg"], sem=taps["enc.sem_agg"], sim=taps["enc.sim"],
                          wav=R15.decode(sd, o["acoustic_codes"], o["semantic_codes"], ospec)))
    codes = codec.encode_ragged(wav.to(gpu_device).unsqueeze(1), feat.to(gpu_device), FRAMES)
    ac, sc = codes["acoustic_codes"].clone(), codes["semantic_codes"].clone()
    w_own = codec.decode_ragged(ac, sc)
    # the oracle's codes, padded with junk length-0 entries: any value in [-K, 0) is a group of no frames
    K, q = ospec.codebook_size, ospec.num_quantizers
    G = max(o["sc"].shape[2] for o in alone)
    junk = -1 - (torch.arange(4 * q * G).view(4, q, G) * 7919) % K
    ac_pad, sc_pad = junk.clone(), junk.clone()
    for b, o in enumerate(alone):
        g = o["sc"].shape[2]
        ac_pad[b, :, :g], sc_pad[b, :, :g] = o["ac"][0], o["sc"][0]
    w = codec.decode_ragged(ac_pad.to(gpu_device), sc_pad.to(gpu_device))  # check_codes is on: length-0 entries are in range
    torch.cuda.synchronize()
    return dict(ospec=ospec, sd=sd, codec=codec, wav=wav, feat=feat, alone=alone, ac=ac, sc=sc, w=w, w_own=w_own, ac_pad=ac_pad, sc_pad=sc_pad)


def test_rows_match_the_oracle_clip_by_clip(full):
    """1. Every row against the oracle on that clip alone.  The inputs are guarded first: no similarity of any clip lies within 1e-3 of the
    threshold (the closest is 0.010), so the grouping - integer output of a threshold test - must equal the oracle's exactly.  Codes: the
    near-tie audit with the project's CODE_TIE_TOL on the oracle's own aggregated embeddings, max_flip_frac=1.0 as for the other
    minimum-length clips (1 .. 12 vectors: any flip must be an audited near-tie); entries behind the clip's groups are -1.  decode_ragged
    of the ORACLE's codes (junk length-0 entries behind them): relative RMS error < 1e-4 per clip, exactly zero behind the clip."""
    ospec, sd = full["ospec"], full["sd"]
    K, q = ospec.codebook_size, ospec.num_quantizers
    cb_a, cb_s = R.rvq_codebooks(sd, "quantizer", q), R.rvq_codebooks(sd, "semantic_quantizer", q)
    for b, o in enumerate(full["alone"]):
        if o["sim"].numel():
            margin = float((o["sim"] - THR).abs().min())
            print(f"clip {b}: min |sim - threshold| = {margin:.4f}")
            assert margin > 1e-3, (b, margin)
    ac, sc, w = full["ac"].cpu(), full["sc"].cpu(), full["w"].cpu()
    G = max(o["sc"].shape[2] for o in full["alone"])
    spf = 2 * ospec.hop  # samples per code frame
    assert ac.shape == sc.shape == (4, q, G) and w.shape == (4, spf * N), (ac.shape, w.shape)
    for b, f in enumerate(FRAMES):
        o = full["alone"][b]
        g = o["sc"].shape[2]
        want = _token_lengths(o["sc"], K)
        print(f"clip {b}: {f} code frames, {g} groups of {want[0].tolist()} frames")
        assert torch.equal(_token_lengths(sc[b:b + 1, :, :g], K), want) and torch.equal(_token_lengths(ac[b:b + 1, :, :g], K), want)
        assert (ac[b, :, g:] == -1).all() and (sc[b, :, g:] == -1).all()
        flips = (audit_codes_bnq(o["emb"], cb_a, ac[b:b + 1, :, :g] % K, o["ac"] % K, max_flip_frac=1.0),
                 audit_codes_bnq(o["sem"], cb_s, sc[b:b + 1, :, :g] % K, o["sc"] % K, max_flip_frac=1.0))
        err = rel_err(w[b, :spf * f], o["wav"][0])
        print(f"clip {b}: near-tie flips {flips}, decode rel. RMS error {err:.3e}")
        assert err < 1e-4, (b, f, err)
        assert torch.equal(w[b, spf * f:], torch.zeros(spf * (N - f)))
    assert full["codec"].adaptive_frames(full["sc"]) == FRAMES


def test_padding_is_never_read(full, gpu_device):
    """2. NaN in wav and feat behind every clip's length: the same codes and, from them, the same waveform, bit for bit; and what the code
    tensors hold in their length-0 entries does not matter either."""
    codec = full["codec"]
    wav, feat = full["wav"].clone(), full["feat"].clone()
    for b, f in enumerate(FRAMES):
        wav[b, HOP * f:] = float("nan")
        feat[b, :, 2 * f:] = float("nan")
    codes = codec.encode_ragged(wav.to(gpu_device).unsqueeze(1), feat.to(gpu_device), FRAMES)
    assert torch.equal(codes["acoustic_codes"], full["ac"]) and torch.equal(codes["semantic_codes"], full["sc"])
    assert torch.equal(codec.decode_ragged(**codes), full["w_own"])
    ac_pad, sc_pad = full["ac_pad"].clone(), full["sc_pad"].clone()
    ac_pad[ac_pad < 0], sc_pad[sc_pad < 0] = -1, -1
    assert torch.equal(codec.decode_ragged(ac_pad.to(gpu_device), sc_pad.to(gpu_device)), full["w"])


# ---- MINI as an H-Codec 1.5 (tests/test_agg_last_rows_gpu.py): hop 16, 2 feature / decoder frames per code frame, 2 aggregator layers

def _mini15(device, **kw):
    import unified_audio_amd as qa

    spec = dataclasses.replace(qa.HCodecSpec(**MINI), adaptive=True, agg_layers=2, bt_layers=1, agg_heads=2, bt_heads=2, agg_ff=128, bt_ff=128,
                               max_tokens_per_group=32, **kw)
    sd = synth.hcodec10_state_dict(7, spec)
    return spec, sd, qa.Codec(None, None, None, spec=spec, device=device).load_state_dict(sd)


@pytest.fixture(scope="module")
def mini(qa_lib, gpu_device):
    return _mini15(gpu_device)


def _const(seed, pieces, frames, dim=64):
    """[dim, frames]: `pieces` constant stretches of (almost) equal length, each an independent normal vector"""
    rng = np.random.default_rng(seed)
    out = np.zeros((dim, frames), np.float32)
    edges = np.linspace(0, frames, pieces + 1).round().astype(int)
    for i in range(pieces):
        out[:, edges[i]:edges[i + 1]] = rng.standard_normal((dim, 1))
    return torch.from_numpy(out)


def _clip(seed, f, pieces=None):
    """(wav [16 f], feat [64, 2 f]).  On the CPU oracle at threshold 0.7: (1, 9) -> 4 groups, (4, 9) -> 3, (8, 4, 1) -> 2 (1 + 3 frames),
    (12, 9, 5) -> 9, (13, 9, 1) -> 1, every similarity at least 0.005 away from the threshold."""
    feat = synth.synth_feat(seed + 50, 1, 2 * f, 64)[0] if pieces is None else _const(seed + 50, pieces, 2 * f)
    return synth.synth_wav(seed, 1, 16 * f)[0], feat


def _batch(clips, n, device):
    """wav [B, 1, 16 n], feat [B, 64, 2 n] with NaN behind every clip, and the lengths"""
    wav = torch.full((len(clips), 16 * n), float("nan"))
    feat = torch.full((len(clips), 64, 2 * n), float("nan"))
    for b, (w, f) in enumerate(clips):
        wav[b, :w.numel()], feat[b, :, :f.shape[1]] = w, f
    return wav.to(device).unsqueeze(1), feat.to(device), [w.numel() // 16 for w, _ in clips]


def _alone(codec, clip, device):
    """the rectangular B = 1 calls on one clip: encode on the unfused stage 0 that a per-clip call takes (the fused
    kernel sums conv0 in another order), decode as it is"""
    with with_knob("QA_SEANET_FUSED", 0):
        c = codec.encode(clip[0].to(device)[None, None], clip[1].to(device)[None], threshold=THR)
    return c["acoustic_codes"], c["semantic_codes"], codec.decode(c["acoustic_codes"], c["semantic_codes"])


@pytest.mark.parametrize("last_rows", [1, 0], ids=["readout-layer", "full-last-layer"])
def test_a_row_does_not_know_its_neighbours(mini, gpu_device, knob, last_rows):
    """3. The clip of 4 code frames (2 groups) gives the same bits as row 1 of [9, 4, 1], as row 2 of [9, 9, 4] inside 12 frames, and as a
    batch of one inside 9 frames - next to clips of 4, 3 and 1 groups, so the batch's G is 4 where it has neighbours - and the same bits
    as the rectangular B = 1 calls on the clip alone.  With QA_AGG_LAST_ROWS 1 (the read-out layer under the mask: compact queries) and 0."""
    spec, sd, codec = mini
    knob("QA_AGG_LAST_ROWS", last_rows)
    K = spec.codebook_size
    x9, y4, z1, v9 = _clip(1, 9), _clip(8, 4, 1), _clip(3, 1), _clip(4, 9)
    a4, s4, w4 = _alone(codec, y4, gpu_device)
    g4 = a4.shape[2]
    assert _token_lengths(s4, K).tolist() == [[1, 3]], _token_lengths(s4, K)
    for clips, n, row, want_G in (([x9, y4, z1], 9, 1, 4), ([x9, v9, y4], 12, 2, 4), ([y4], 9, 0, 2)):
        wav, feat, fr = _batch(clips, n, gpu_device)
        c = codec.encode_ragged(wav, feat, fr, threshold=THR)
        c2 = codec.encode_ragged(wav, feat, fr, threshold=THR)
        ac, sc = c["acoustic_codes"], c["semantic_codes"]
        assert torch.equal(ac, c2["acoustic_codes"]) and torch.equal(sc, c2["semantic_codes"])
        assert ac.shape[2] == want_G and codec.adaptive_frames(sc) == fr, (ac.shape, codec.adaptive_frames(sc), fr)
        assert torch.equal(ac[row, :, :g4], a4[0]) and torch.equal(sc[row, :, :g4], s4[0]), (n, row)
        assert (ac[row, :, g4:] == -1).all() and (sc[row, :, g4:] == -1).all()
        w = codec.decode_ragged(ac, sc)
        assert w.shape == (len(fr), 16 * max(fr)) and torch.equal(w, codec.decode_ragged(ac, sc))
        assert all(torch.equal(w[b, 16 * f:], torch.zeros(16 * (max(fr) - f), device=gpu_device)) for b, f in enumerate(fr))
        assert torch.equal(w[row, :16 * 4], w4[0]), (n, row)


def test_equal_lengths(mini, qa_lib, gpu_device):
    """4. B = 1 with lengths = [N] is the rectangular call, bit for bit.  Four clips of 9 frames with 4 / 3 / 9 / 1 groups: every row of the
    per-clip call equals its clip alone, which the rectangular batch need not (printed: in how many code entries it differs).  A call with
    lengths takes the masked path also when every length is N; a rectangular 1.5 call launches no masked attention."""
    spec, sd, codec = mini
    K = spec.codebook_size
    clips = [_clip(1, 9), _clip(4, 9), _clip(12, 9, 5), _clip(13, 9, 1)]
    wav, feat, fr = _batch(clips, 9, gpu_device)
    a0, m0 = _att_launches(qa_lib)
    with with_knob("QA_SEANET_FUSED", 0):
        rect = codec.encode(wav, feat, threshold=THR)
    w_rect = codec.decode(**rect)
    a1, m1 = _att_launches(qa_lib)
    assert a1 > a0 and m1 == m0  # the rectangular calls: attention launches, none of them masked
    c = codec.encode_ragged(wav, feat, fr, threshold=THR)
    w = codec.decode_ragged(**c)
    a2, m2 = _att_launches(qa_lib)
    assert a2 - a1 == a1 - a0 == m2 - m1  # as many launches, every one masked
    nseg = (_token_lengths(c["semantic_codes"], K) > 0).sum(dim=1).tolist()
    assert nseg == [4, 3, 9, 1] and c["semantic_codes"].shape[2] == 9, nseg
    for b, clip in enumerate(clips):
        a1c, s1c, w1c = _alone(codec, clip, gpu_device)
        g = nseg[b]
        assert a1c.shape[2] == g
        assert torch.equal(c["acoustic_codes"][b, :, :g], a1c[0]) and torch.equal(c["semantic_codes"][b, :, :g], s1c[0]), b
        assert (c["acoustic_codes"][b, :, g:] == -1).all() and torch.equal(w[b], w1c[0]), b
        d = int((rect["acoustic_codes"][b, :, :g] % K != a1c[0] % K).sum()), float((w_rect[b] - w1c[0]).abs().max())
        print(f"row {b}: {g} groups; the rectangular batch differs from the clip alone in {d[0]} of {a1c[0].numel()} acoustic codes, "
              f"max |wav difference| {d[1]:.2e}")
        # B = 1, lengths = [N]: the rectangular call itself
        x1, f1 = clip[0].to(gpu_device)[None, None], clip[1].to(gpu_device)[None]
        c1 = codec.encode_ragged(x1, f1, [9], threshold=THR)
        assert torch.equal(c1["acoustic_codes"], a1c) and torch.equal(c1["semantic_codes"], s1c)
        assert torch.equal(codec.decode_ragged(**c1), w1c)


class _Raw:
    """the per-clip entry points through ctypes, on buffers of this object; frames: a Python list"""

    def __init__(self, codec, qa_lib, B, n, device):
        self.codec, self.lib, self.B, self.n = codec, qa_lib, B, n
        q = codec.spec.num_quantizers
        self.wav = torch.zeros((B, 16 * n), device=device)
        self.feat = torch.zeros((B, 64, 2 * n), device=device)
        self.codes = torch.zeros((B, q, n), dtype=torch.int64, device=device)
        self.out = torch.zeros((B, 16 * n), device=device)
        self.g = C.c_int64(0)

    def encode(self, frames):
        fr = (C.c_int64 * len(frames))(*frames)
        sb, sc, st = self.feat.stride()
        st_ = self.lib.qa_hcodec_encode_adaptive_ragged(self.codec._handle, self.wav.data_ptr(), self.B, self.wav.shape[1], fr, self.feat.data_ptr(),
                                                        sb, sc, st, self.feat.shape[2], self.codes.data_ptr(), self.codes.data_ptr(),
                                                        C.byref(self.g), THR, None)
        return st_, self.lib.qa_last_error().decode()

    def decode(self, frames):
        fr = (C.c_int64 * len(frames))(*frames)
        st_ = self.lib.qa_hcodec_decode_adaptive_ragged(self.codec._handle, self.codes.data_ptr(), self.codes.data_ptr(), self.B, self.n, self.n, fr,
                                                        self.out.data_ptr(), None)
        return st_, self.lib.qa_last_error().decode()


def test_refusals_and_checks_come_before_any_launch(mini, qa_lib, gpu_device):
    """5. Bad lengths are QA_ERR_INVALID, name the entry point, the row and its value, and launch nothing; causal aggregators, a causal
    bottleneck and spec.causal are QA_ERR_UNSUPPORTED; a 1.0 handle is refused by the family check (QA_ERR_INVALID, as on the other adaptive
    entry points); a row whose codes hold no frame is QA_ERR_INVALID naming the row; the 1.0 methods keep refusing a 1.5 model."""
    import unified_audio_amd as qa

    spec, sd, codec = mini
    n = 6
    raw = _Raw(codec, qa_lib, 2, n, gpu_device)
    torch.cuda.synchronize()
    before = _att_launches(qa_lib)
    for bad in (0, n + 1, -3):
        for fn, call in (("qa_hcodec_encode_adaptive_ragged", raw.encode), ("qa_hcodec_decode_adaptive_ragged", raw.decode)):
            st, msg = call([n, bad])
            assert st == INVALID and msg.startswith(fn + ":") and f"frames[1] = {bad}" in msg, (fn, st, msg)
        with pytest.raises(qa.QuarkAudioError) as e:
            codec.encode_ragged(raw.wav.unsqueeze(1), raw.feat, [n, bad])
        assert e.value.status == INVALID and f"frames[1] = {bad}" in str(e.value), str(e.value)
    with pytest.raises(qa.QuarkAudioError) as e:
        codec.encode_ragged(raw.wav.unsqueeze(1), raw.feat, [n])  # wrong count
    assert e.value.status == INVALID
    # a row with no frames: its codes are all length-0 entries
    codes = torch.zeros((2, spec.num_quantizers, 3), dtype=torch.int64, device=gpu_device)
    codes[1] = -1
    with pytest.raises(qa.QuarkAudioError) as e:
        codec.decode_ragged(codes, codes)
    assert e.value.status == INVALID and "frames[1] = 0" in str(e.value), str(e.value)
    # the 1.0 calls on this model: refused as before, and the message now names the per-clip methods
    for call in (lambda: codec.encode(raw.wav.unsqueeze(1), raw.feat, lengths=[n, 1]), lambda: codec.decode(raw.codes, raw.codes, lengths=[n, 1])):
        with pytest.raises(qa.QuarkAudioError) as e:
            call()
        assert e.value.status == UNSUPPORTED and "1.5" in str(e.value) and "encode_ragged" in str(e.value), str(e.value)
    for kw, word in ((dict(agg_causal=True), "causal aggregators"), (dict(bt_causal=True), "causal bottleneck"), (dict(causal=True), "spec.causal")):
        _, _, cc = _mini15(gpu_device, **kw)
        r = _Raw(cc, qa_lib, 2, n, gpu_device)
        for fn, call in (("qa_hcodec_encode_adaptive_ragged", r.encode), ("qa_hcodec_decode_adaptive_ragged", r.decode)):
            st, msg = call([n, 2])
            assert st == UNSUPPORTED and msg.startswith(fn + ":") and word in msg, (kw, fn, st, msg)
    c10 = qa.Codec(None, None, None, spec=qa.HCodecSpec(**MINI), device=gpu_device).load_state_dict(synth.hcodec10_state_dict(21, qa.HCodecSpec(**MINI)))
    r = _Raw(c10, qa_lib, 2, n, gpu_device)
    for fn, call in (("qa_hcodec_encode_adaptive_ragged", r.encode), ("qa_hcodec_decode_adaptive_ragged", r.decode)):
        st, msg = call([n, 2])
        assert st == INVALID and msg.startswith(fn + ":") and "is not an H-Codec 1.5 model" in msg, (fn, st, msg)
    torch.cuda.synchronize()
    assert _att_launches(qa_lib) == before  # none of the refused calls launched an attention
    assert bool((raw.out == 0).all()) and raw.g.value == 0  # ... or wrote an output


def test_tokenizer_routes_lengths_to_the_per_clip_calls(mini, gpu_device):
    """6. tokenize(wav, feats=..., lengths=samples) then detokenize(**codes, ragged=True) equal the Codec calls; sample lengths round up to
    whole hops, and each clip is the clip alone through the rectangular tokenizer (unfused stage 0, as above)."""
    import unified_audio_amd as qa

    spec, sd, codec = mini
    tok = qa.HCodecTokenizer(model=codec, device=gpu_device)
    lens = [16 * 9 + 5, 16 * 3 + 1]
    assert tok.code_frames(lens) == [10, 4]
    w = torch.full((2, lens[0]), float("nan"))
    w[0], w[1, :lens[1]] = synth.synth_wav(1, 1, lens[0])[0], synth.synth_wav(8, 1, lens[1])[0]
    feats = torch.stack([synth.synth_feat(51, 1, 20, 64)[0], torch.cat([_const(58, 1, 8), torch.full((64, 12), float("nan"))], dim=1)]).transpose(1, 2)
    codes = tok.tokenize(w, feats=feats, lengths=lens, threshold=THR)
    assert set(codes) == {"acoustic_codes", "semantic_codes"} and codec.adaptive_frames(codes["semantic_codes"]) == [10, 4]
    # the Codec call on the same clips, each zero-padded to its own hop multiple
    wp = torch.full((2, 160), float("nan"))
    wp[0, :lens[0]], wp[1, :lens[1]] = w[0], w[1, :lens[1]]
    wp[0, lens[0]:160], wp[1, lens[1]:64] = 0.0, 0.0
    want = codec.encode_ragged(wp.to(gpu_device).unsqueeze(1), feats.transpose(1, 2).to(gpu_device), [10, 4], threshold=THR)
    assert all(torch.equal(codes[k], want[k]) for k in want)
    out = tok.detokenize(**codes, ragged=True)
    assert out.shape == (2, 160) and torch.equal(out, codec.decode_ragged(**codes))
    assert torch.equal(out[1, 64:], torch.zeros(96, device=gpu_device)) and bool(out[1, :64].abs().sum() > 0) and bool(torch.isfinite(out).all())
    with with_knob("QA_SEANET_FUSED", 0):
        one = tok.tokenize(w[1:2, :lens[1]], feats=feats[1:2, :8], threshold=THR)
    g = one["semantic_codes"].shape[2]
    assert torch.equal(one["acoustic_codes"][0], codes["acoustic_codes"][1, :, :g]) and (codes["acoustic_codes"][1, :, g:] == -1).all()
    assert torch.equal(tok.detokenize(**one)[0], out[1, :64])
