"""Pre-split weight images (QA_GEMM_PRESPLIT, csrc/split_planes.h): a weight store builds the three bf16 planes of all its weights
once, at load, and conv_gemm's split-6 launches copy them into LDS instead of splitting the weight tile in the K loop.

The split is elementwise and deterministic and the LDS image is the same, so everything here is BIT FOR BIT, no tolerance:
(a) whole models - H-Codec 1.0 / 1.5 / 2.0 encode + decode, BiCodec detokenize, an SSL extractor - give torch.equal outputs with
    QA_GEMM_PRESPLIT = 1 and 0, under the cost model's choice AND with the 128-column tiles forced (QA_GEMM_CFG 2, 3): only those
    read an image, the cost model picks narrower ones at these small shapes, and the profiler hook confirms that 128-column
    launches ran against the store's image; on one model also with every tile forced (QA_GEMM_CFG 0 .. 4), with the table form
    (QA_GEMM_LINEAR = 0) and under the fp32 chain (QA_GEMM_MATH = 0), which ignores the image;
(b) every legal (tile, path, geometry) instantiation of tests/test_conv_gemm_gpu.py, its weight given an image through
    qa_weight_planes / qa_weight_planes_attach: the same bits with the image used, ignored and detached; a zeroed image shows
    that the 128-column tiles (and only they) really read it;
(c) the LM keeps the fp32 chain: no image is built for it and generate is unchanged;
(d) the image itself equals the numpy emulation of the split (tests/test_split_rne_cpu.py) for subnormals, +-inf, NaN and values
    that round to bf16 inf.
"""
import dataclasses

import numpy as np
import pytest
import torch

from oracle import hcodec_ref as R
from oracle import llm_ref as LR
from oracle import ssl_ref as S
from oracle import synth as osynth
from tests import test_conv_gemm_gpu as G
from tests.test_bicodec_tokenize_gpu import SMALL as BICODEC_SMALL
from tests.test_bicodec_tokenize_gpu import _dspec, _full_sd
from tests.test_llm_gpu import SMALL as LM_SMALL
from tests.test_split_rne_cpu import split
from tests.util import MINI
from unified_audio_amd import synth

pytestmark = pytest.mark.gpu


def _plane_bytes(lib):
    return int(lib.qa_weight_planes_bytes())


def _same_with_and_without(knob, run, label=""):
    """run() -> list of tensors: equal with the images used (1) and ignored (0)."""
    knob("QA_GEMM_PRESPLIT", 1)
    a = [t.clone() for t in run()]
    knob("QA_GEMM_PRESPLIT", 0)
    b = [t.clone() for t in run()]
    knob("QA_GEMM_PRESPLIT", 1)
    torch.cuda.synchronize()
    assert len(a) == len(b)
    for i, (u, v) in enumerate(zip(a, b)):
        assert u.shape == v.shape and torch.equal(u, v), f"{label}: output {i} differs between QA_GEMM_PRESPLIT = 1 and 0"
    return a


def _loaded(lib, load):
    """load() -> model; the load must have attached a plane image."""
    before = _plane_bytes(lib)
    m = load()
    assert _plane_bytes(lib) > before, "the load attached no plane image"
    return m


def _hcodec10(lib, dev):
    import unified_audio_amd as qa

    ospec = R.HCodecSpec(**MINI)
    sd = osynth.hcodec10_state_dict(5, ospec)
    codec = _loaded(lib, lambda: qa.Codec(None, None, None, spec=qa.HCodecSpec(**MINI), device=dev).load_state_dict(sd))
    T = 16 * 64 * 3
    wav = osynth.synth_wav(6, 3, T).to(dev).unsqueeze(1)
    feat = osynth.synth_feat(7, 3, T // 8, 64).to(dev)

    def run():
        ac, sc = codec.encode(wav, feat)
        return [ac, sc, codec.decode(ac, sc)]

    return run


def _hcodec15(lib, dev):
    import unified_audio_amd as qa

    ospec = dataclasses.replace(R.SPEC_15, agg_layers=1, bt_layers=1, threshold=0.6)
    sd = osynth.hcodec10_state_dict(17, ospec)
    kw = {f: getattr(ospec, f) for f in ospec.__dataclass_fields__}
    codec = _loaded(lib, lambda: qa.Codec(None, None, None, spec=qa.HCodecSpec(**kw), device=dev).load_state_dict(sd))
    wav = osynth.synth_wav(3, 2, 640 * 40).to(dev).unsqueeze(1)
    feat = osynth.synth_feat(4, 2, 80, ospec.sem_in).to(dev)

    def run():
        codes = codec.encode(wav, feat)
        return [codes["acoustic_codes"], codes["semantic_codes"], codec.decode(codes["acoustic_codes"], codes["semantic_codes"])]

    return run


def _hcodec20(lib, dev):
    import unified_audio_amd as qa
    from oracle import hcodec20_ref as R20

    o = R20.HCodec20Spec(enc_dim=256, enc_inter=512, enc_convnext_layers=2, enc_transformer_layers=1, dimension=128, sem_in=64,
                         sem_ch=128, codebook_size=64, num_quantizers=5, dec_dim=256, dec_inter=512, dec_convnext_layers=2,
                         dec_transformer_layers=1)
    sd = osynth.hcodec20_state_dict(51, o)
    pspec = qa.HCodecSpec(version=20, enc_dim=o.enc_dim, enc_inter=o.enc_inter, enc_convnext_layers=o.enc_convnext_layers,
                          enc_layers=o.enc_transformer_layers, frame_stride=o.stride, tr_inter_cap=o.tr_inter_cap, dimension=o.dimension,
                          code_dim=o.dimension, sem_in=o.sem_in, sem_ch=o.sem_ch, sem_strides=o.sem_strides,
                          codebook_size=o.codebook_size, num_quantizers=o.num_quantizers, dec_dim=o.dec_dim, dec_inter=o.dec_inter,
                          dec_heads=o.dec_dim // 64, dec_layers=o.dec_transformer_layers, convnext_layers=o.dec_convnext_layers,
                          n_fft=o.n_fft, hop=o.hop, gn_groups=o.gn_groups, causal=o.causal)
    codec = _loaded(lib, lambda: qa.Codec(None, None, None, spec=pspec, device=dev).load_state_dict(sd))
    T = 3840 * 6
    wav = osynth.synth_wav_fullband(52, 2, T).to(dev)
    feat = osynth.synth_feat(53, 2, T // o.hop, o.sem_in).to(dev)

    def run():
        ac, sc = codec.encode(wav, feat)
        return [ac, sc, codec.decode(ac, sc)]

    return run


def _bicodec(lib, dev):
    import unified_audio_amd as qa

    espec = qa.BiCodecEncoderSpec(**BICODEC_SMALL)
    sd = _full_sd(espec, 41)
    m = _loaded(lib, lambda: qa.BiCodec(_dspec(espec), device=dev, encoder_spec=espec).load_state_dict(sd))
    sem, glob = synth.bicodec_tokens(42, 2, 40, _dspec(espec))
    sem, glob = sem.to(dev), glob.to(dev)
    return lambda: [m.detokenize(sem, glob)]


def _ssl(lib, dev):
    import unified_audio_amd as qa

    ospec = S.SSLSpec(conv_dim=(64,) * 7, hidden_size=96, num_hidden_layers=2, num_attention_heads=3, intermediate_size=192,
                      num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=2)
    sd = S.synth_state_dict(3, ospec, "hubert")
    kw = {f.name: getattr(ospec, f.name) for f in dataclasses.fields(ospec)}
    fx = _loaded(lib, lambda: qa.SSLFeatureExtractor(qa.SSLSpec(**kw), device=dev).load_state_dict(sd))
    wav = torch.randn(2, 8000, generator=torch.Generator().manual_seed(4)).to(dev)
    return lambda: [fx(wav)]


MODELS = {"hcodec10": _hcodec10, "hcodec15": _hcodec15, "hcodec20": _hcodec20, "bicodec_detokenize": _bicodec, "ssl": _ssl}


WIDE = (2, 3, 5)  # QA_GEMM_CFG of the 128-column tiles (128 x 128, 64 x 128, 256 x 128): the ones that read an image


def _ab_on_wide_tiles(lib, knob, run, label, cfgs=(-1, 2, 3), extra=None):
    """run() under the cost model's choice and with each 128-column tile forced: QA_GEMM_PRESPLIT = 1 and 0 give the same bits, every
    forced setting gives the bits of the first, and under each forced tile the profiler saw launches of a 128-column tile - at the
    small shapes of these tests the cost model alone picks narrower tiles, which never read an image."""
    base = None
    for cfg in cfgs:
        G._pin_defaults(lib, knob)
        for k, v in (extra or {}).items():
            knob(k, v)
        knob("QA_GEMM_CFG", cfg)
        knob("QA_GEMM_PRESPLIT", 1)
        _, launches = G._profiled(lib, run)
        wide = sum(launches[c] for c in WIDE)
        print(f"{label} QA_GEMM_CFG={cfg}: launches per tile {launches}")
        if cfg in WIDE:
            assert wide > 0, f"{label}: no launch took a 128-column tile under QA_GEMM_CFG = {cfg}: {launches}"
        out = _same_with_and_without(knob, run, f"{label} cfg {cfg}")
        if base is None:
            base = out
        for u, v in zip(out, base):
            assert torch.equal(u, v), f"{label}: QA_GEMM_CFG = {cfg} differs from the first setting"
    return base


# (a)
@pytest.mark.parametrize("model", list(MODELS))
def test_model_outputs_do_not_depend_on_the_plane_image(qa_lib, gpu_device, knob, model):
    run = MODELS[model](qa_lib, gpu_device)  # _loaded: the store attached an image
    out = _ab_on_wide_tiles(qa_lib, knob, run, model)
    assert all(torch.isfinite(t).all() for t in out if t.is_floating_point())


def test_every_tile_and_the_table_form_read_the_same_planes(qa_lib, gpu_device, knob):
    run = _hcodec15(qa_lib, gpu_device)
    base = _ab_on_wide_tiles(qa_lib, knob, run, "hcodec15", cfgs=(-1, 0, 1, 2, 3, 4))
    for extra in ({"QA_GEMM_LINEAR": 0}, {"QA_GEMM_BK16": 0}, {"QA_GEMM_BK16_MIN_TILES": 0}, {"QA_GEMM_LINEAR": 0, "QA_GEMM_BK16_MIN_TILES": 0}):
        out = _ab_on_wide_tiles(qa_lib, knob, run, f"hcodec15 {extra}", cfgs=(2, 3), extra=extra)
        for u, v in zip(out, base):
            assert torch.equal(u, v), f"{extra} differs from the default knobs"


def test_fp32_chain_ignores_the_plane_image(qa_lib, gpu_device, knob):
    run = _hcodec10(qa_lib, gpu_device)
    _ab_on_wide_tiles(qa_lib, knob, run, "fp32 chain", extra={"QA_GEMM_MATH": 0})


def test_a_store_loaded_without_planes_computes_the_same(qa_lib, gpu_device, knob):
    import unified_audio_amd as qa

    G._pin_defaults(qa_lib, knob)
    knob("QA_GEMM_CFG", 2)  # 128 x 128: the store that has an image reads it
    ospec = R.HCodecSpec(**MINI)
    sd = osynth.hcodec10_state_dict(5, ospec)
    T = 16 * 64 * 3
    wav = osynth.synth_wav(6, 3, T).to(gpu_device).unsqueeze(1)
    feat = osynth.synth_feat(7, 3, T // 8, 64).to(gpu_device)
    outs = []
    for pre in (1, 0):
        knob("QA_GEMM_PRESPLIT", pre)
        before = _plane_bytes(qa_lib)
        codec = qa.Codec(None, None, None, spec=qa.HCodecSpec(**MINI), device=gpu_device).load_state_dict(sd)
        assert (_plane_bytes(qa_lib) > before) == bool(pre)
        knob("QA_GEMM_PRESPLIT", 1)  # at launch: use an image where there is one

        def run():
            ac, sc = codec.encode(wav, feat)
            return [ac.clone(), sc.clone(), codec.decode(ac, sc).clone()]

        out, launches = G._profiled(qa_lib, run)
        assert launches[2] > 0, launches
        outs.append(out)
        del codec
    for u, v in zip(*outs):
        assert torch.equal(u, v)


# (b)
def _image(lib, w):
    """Device image (uint8, 6 bytes per weight) of a device float tensor, built by the library's kernel."""
    from unified_audio_amd import _lib

    assert w.is_contiguous() and w.numel() % 8 == 0
    planes = torch.zeros(w.numel() * 6, dtype=torch.uint8, device=w.device)
    _lib.check(lib.qa_weight_planes(w.data_ptr(), w.numel(), planes.data_ptr(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return planes


@pytest.mark.parametrize("tile,path,geo", G.PARITY, ids=[f"cfg{t}-{p}-{g}" for t, p, g in G.PARITY])
def test_every_instantiation_gives_the_same_bits_from_an_image(qa_lib, gpu_device, knob, tile, path, geo):
    from unified_audio_amd import _lib

    G._pin_defaults(qa_lib, knob)
    prob, _ = G._small(geo, path, gpu_device)
    knob("QA_GEMM_CFG", tile)
    for k, v in G.PATHS[path][0].items():
        knob(k, v)
    knob("QA_GEMM_PRESPLIT", 1)
    plain = prob.run(qa_lib).clone()  # no image attached: the in-loop split
    planes = _image(qa_lib, prob.wd)
    before = _plane_bytes(qa_lib)
    _lib.check(qa_lib.qa_weight_planes_attach(prob.wd.data_ptr(), prob.wd.numel(), planes.data_ptr()))
    try:
        assert _plane_bytes(qa_lib) == before + planes.numel()
        used = prob.run(qa_lib).clone()
        knob("QA_GEMM_PRESPLIT", 0)
        ignored = prob.run(qa_lib).clone()
        knob("QA_GEMM_PRESPLIT", 1)
        # poison the image: a launch that really reads it now gives other numbers - the attached path is the one that ran
        planes.fill_(0)
        poisoned = prob.run(qa_lib).clone()
        torch.cuda.synchronize()
    finally:
        _lib.check(qa_lib.qa_weight_planes_detach(prob.wd.data_ptr()))
    assert _plane_bytes(qa_lib) == before
    detached = prob.run(qa_lib)
    assert torch.equal(used, plain), "the pre-split path differs from the in-loop split"
    assert torch.equal(ignored, plain) and torch.equal(detached, plain)
    cfg, _ = G._launched(tile, path, prob.c)
    if G.TILES[cfg][1] == 128:  # the 128-column tiles read the image; narrower ones keep the in-loop split
        assert not torch.equal(poisoned, plain), "the launch did not read the attached image"
    else:
        assert torch.equal(poisoned, plain), "a tile narrower than 128 columns read the image"


@pytest.mark.parametrize("tile", [2, 3])
def test_row_slices_of_an_imaged_weight_find_their_planes(qa_lib, gpu_device, knob, tile):
    """The image address follows from the float's offset alone: a launch on rows [r0, r1) of an attached weight reads the planes of
    those rows.  Forced 128-column tiles (the ones that read an image); slices that start inside the attached range, with N = 100 and
    N = 1 (rows past N clamped to row N - 1 of the slice) and one that spans two column tiles; a zeroed image shows that every one
    of these launches really read it."""
    from tests.util import conv1d_cl
    from unified_audio_amd import _lib

    G._pin_defaults(qa_lib, knob)
    g = torch.Generator().manual_seed(77)
    x = torch.randn(1, 700, 96, generator=g).to(gpu_device)
    w = (torch.randn(300, 1, 96, generator=g) * 0.1).to(gpu_device)
    b = torch.randn(300, generator=g).to(gpu_device)
    slices = ((0, 300), (37, 137), (37, 165), (100, 300), (200, 300), (299, 300))
    knob("QA_GEMM_CFG", tile)
    knob("QA_GEMM_PRESPLIT", 1)
    full, launches = G._profiled(qa_lib, lambda: conv1d_cl(qa_lib, x, w, b).clone())  # no image attached yet: the in-loop split
    assert launches == [int(i == tile) for i in range(6)], launches
    planes = _image(qa_lib, w)
    _lib.check(qa_lib.qa_weight_planes_attach(w.data_ptr(), w.numel(), planes.data_ptr()))
    try:
        for r0, r1 in slices:
            y, launches = G._profiled(qa_lib, lambda: conv1d_cl(qa_lib, x, w[r0:r1], b[r0:r1]))
            assert launches == [int(i == tile) for i in range(6)], launches
            assert torch.equal(y, full[..., r0:r1]), f"rows {r0}:{r1} from the image differ from the in-loop split"
        planes.fill_(0)
        for r0, r1 in slices:
            y = conv1d_cl(qa_lib, x, w[r0:r1], b[r0:r1])
            assert not torch.equal(y, full[..., r0:r1]), f"rows {r0}:{r1}: the launch did not read the attached image"
        torch.cuda.synchronize()
    finally:
        _lib.check(qa_lib.qa_weight_planes_detach(w.data_ptr()))
    # a weight that reaches past the attached range has no planes: in-loop split, right bits (the zeroed image would show)
    w2 = torch.cat([w.flatten(), w.flatten()[:96 * 4]]).contiguous()
    _lib.check(qa_lib.qa_weight_planes_attach(w2.data_ptr(), 96 * 300, planes.data_ptr()))  # the first 300 rows only
    try:
        past = w2[96 * 200:96 * 304].view(104, 1, 96)  # rows 200 .. 303: four of them outside the attached range
        y = conv1d_cl(qa_lib, x, past, b[:104])
        want = conv1d_cl(qa_lib, x, past.clone(), b[:104])
        inside = conv1d_cl(qa_lib, x, w2[96 * 200:96 * 300].view(100, 1, 96), b[:100])
        torch.cuda.synchronize()
    finally:
        _lib.check(qa_lib.qa_weight_planes_detach(w2.data_ptr()))
    assert torch.equal(y, want), "a weight that reaches past the attached range read the image"
    assert not torch.equal(inside, want[..., :100]), "rows inside the attached range did not read the (zeroed) image"


# (c)
def test_lm_builds_no_image_and_generates_the_same(qa_lib, gpu_device, knob):
    import unified_audio_amd as qa

    spec = LM_SMALL
    sd = LR.lm_state_dict(21, spec)
    cfg = dict(global_size=spec.global_size, semantic_size=spec.semantic_size, hidden_size=spec.hidden, num_layers=spec.n_layers,
               num_attention_heads=spec.n_heads)
    before = _plane_bytes(qa_lib)
    lm = qa.LLM_SFT(num_tasks=spec.num_tasks, feats_dim=spec.feats_dim, llm_base_config=cfg, device=gpu_device).load_state_dict(sd)
    assert _plane_bytes(qa_lib) == before, "the LM's store built a plane image although its launches keep the fp32 chain"
    mix = LR.synth_feats(1, 2, 40, spec.feats_dim).to(gpu_device)
    mel = torch.zeros(2, 4, 80)
    _same_with_and_without(knob, lambda: list(lm.generate("se", None, None, mel, mix, global_length=3, do_sample=False)), "lm.generate")


# (d)
def _special_values():
    rng = np.random.default_rng(9)
    v = np.concatenate([
        rng.standard_normal(4096).astype(np.float32),
        (rng.standard_normal(4096) * np.exp2(rng.integers(-120, 120, 4096))).astype(np.float32),
        rng.integers(1, 1 << 23, 1024, dtype=np.uint32).view(np.float32),                    # subnormals
        rng.integers(0x7F7F8000, 0x7F800000, 64, dtype=np.uint32).view(np.float32),           # finite, round to bf16 inf
        np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 3.3895314e38, 2.0 ** -126, 2.0 ** -149], np.float32),
    ])
    v = np.concatenate([v, -v])
    rng.shuffle(v)
    return v[:len(v) // 8 * 8].copy()


def test_the_image_equals_the_numpy_split(qa_lib, gpu_device):
    x = _special_values()
    n = len(x)
    img = _image(qa_lib, torch.from_numpy(x).to(gpu_device)).cpu().numpy()
    assert img.size == 6 * n
    got = img.view(np.uint16).reshape(n // 8, 3, 8)  # [group][plane][float in group]: csrc/split_planes.h
    for p, want in enumerate(split(x)):
        want_bits = (want.view(np.uint32) >> 16).astype(np.uint16).reshape(n // 8, 8)
        nan = np.isnan(want).reshape(n // 8, 8)
        g = got[:, p, :]
        assert np.array_equal(g[~nan], want_bits[~nan]), f"plane {p} differs from the numpy split"
        # NaN: any NaN pattern of bf16
        assert np.all((g[nan] & 0x7F80) == 0x7F80) and np.all((g[nan] & 0x007F) != 0), f"plane {p}: a NaN did not stay NaN"
    # the byte offsets the layout function gives are where the values sit
    for idx, plane in ((0, 0), (5, 1), (8, 2), (n - 1, 0), (n - 1, 2)):
        off = qa_lib.qa_weight_plane_offset(idx, plane)
        assert img[off:off + 2].view(np.uint16)[0] == got[idx // 8, plane, idx % 8]
