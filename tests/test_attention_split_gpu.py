"""The two arithmetic forms of attention_kernel (csrc/attention.hip: one kernel body, the SPLIT template parameter selects the AttForm;
knob QA_ATT_MATH): 1 = split-6 (three bf16 planes per operand, six v_mfma_f32_32x32x16_bf16 per 16-wide k group), 0 = the fp32 chain
(v_mfma_f32_32x32x2_f32).  The parity matrix, the memory contract and the invariances of both forms are in tests/test_attention_gpu.py.

(a) both forms on the callers' geometries against the float64 truth of tests/test_attention_gpu.py, under that file's bound
    C_PARITY * max(e_cpu32, E_FLOOR, S_ULP * s_max) - the bound comes from the host's own fp32 evaluation and the number format, and both
    forms must meet it.  The ratio e_split / e_chain is printed per case and per mode (test_split_ratio_report, pytest -s); it is a
    record, not a gate: split-6 keeps every bf16 x bf16 product exact and drops only terms of the size of one fp32 rounding, so the
    expectation from conv_gemm is a ratio of at most about 1.
(b) who takes which form: a UniSE LM handle and a codec handle in one process, counted by qa_debug_att_stats - the LM's prefill takes
    the fp32 chain whatever the knob says (its decode kernels are fp32), the codec follows the knob.
(c) every plane of every operand is read: zeroing the h, m or l plane (QA_ATT_DEBUG bits 32 / 64 / 128) of Q, K, V or P alone (bits
    256 / 512 / 1024 / 2048) changes the split-6 output, by about 1, 2^-8 and 2^-16 relative; the fp32 chain ignores the bits.  The
    probability split without finite tests (split4_unit) gives the planes of split4_rne on [0, 1], compared on the device
    (qa_debug_att_split_unit) over every exponent down to the subnormals.
(d) a query with no visible key gives exactly 0 in both forms (ring mode, a chunk as long as the ring).
(e) the key-padding mask (the KMASK instantiations of the Conformer condition encoder, through qa_debug_attention_kmask): both forms
    against fp64 under the same bound, every head dim, ragged lengths on the tile edges, an item whose keys are all padding (exact 0),
    padded keys hold finite data: they are read and multiplied by p = 0, as in the reference.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import zlib

import pytest
import torch

from tests.test_attention_gpu import (AT_SIZE, C_PARITY, E_FLOOR, OUT_HEAD, S_ULP, Case, _seed, check_parity, launch, make_inputs, pack,
                                      reference_mask)
from tests.util import check_guarded_out, guarded_out, with_knob

pytestmark = pytest.mark.gpu

GEOMETRIES = dict(AT_SIZE)
GEOMETRIES.update({
    "hcodec15_aggregator": Case("self", B=32, H=8, hd=64, n_q=283, n_keys=283),   # 64 launches per H-Codec 1.5 step
    "hcodec15_encoder": Case("self", B=32, H=8, hd=64, n_q=500, n_keys=500),
    "hcodec10_decoder": Case("self", B=32, H=8, hd=96, n_q=500, n_keys=500),
    "small_hd32": Case("self", B=3, H=5, hd=32, n_q=283, n_keys=283),
    "window_hd96": Case("window", B=3, H=5, hd=96, n_q=283, n_keys=283, context=34),
})
RATIOS = []  # (mode, name, e_chain, e_split)


def _stats(lib):
    out = (C.c_int64 * 2)()
    assert lib.qa_debug_att_stats(out) == 0, lib.qa_last_error()
    return int(out[0]), int(out[1])


@pytest.mark.parametrize("name", sorted(GEOMETRIES))
def test_both_forms_meet_the_fp64_bound(qa_lib, gpu_device, name):
    c = GEOMETRIES[name]
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    edges = {0, 1, 31, 32, 33, 127, 128, 129, c.n_q - 1}
    rows = sorted({r for r in edges if r < c.n_q} | set(torch.randint(0, c.n_q, (24,), generator=g).tolist()))
    x = make_inputs(c, "randn", _seed(c, "randn"))
    e, bad = {}, []
    for math in (0, 1):
        with with_knob("QA_ATT_MATH", math):
            before = _stats(qa_lib)
            e_hip, e_cpu, bound, msg = check_parity(qa_lib, c, "randn", rows=rows, x=x)
            after = _stats(qa_lib)
        assert after[math] == before[math] + 1 and after[1 - math] == before[1 - math], "the knob did not select the kernel form"
        e[math] = e_hip
        if msg:
            bad.append(f"QA_ATT_MATH={math}: {msg}")
    RATIOS.append((c.mode, name, e[0], e[1]))
    print(f"ATTN-SPLIT {name} ({c.mode} hd{c.hd}): e_chain {e[0]:.3e} e_split {e[1]:.3e} ratio {e[1] / max(e[0], 1e-300):.3f}")
    assert not bad, "\n".join(bad)


def test_lm_takes_the_fp32_chain_and_the_codec_follows_the_knob(qa_lib, gpu_device):
    import unified_audio_amd as qa
    from oracle import llm_ref as L
    from oracle import hcodec_ref as R
    from oracle import synth

    spec = L.LMSpec(hidden=256, n_layers=2, n_heads=4, global_size=96, semantic_size=160, feats_dim=64, num_tasks=3)
    sd = L.lm_state_dict(21, spec)
    cfg = dict(global_size=spec.global_size, semantic_size=spec.semantic_size, hidden_size=spec.hidden, num_layers=spec.n_layers,
               num_attention_heads=spec.n_heads)
    lm = qa.LLM_SFT(num_tasks=spec.num_tasks, feats_dim=spec.feats_dim, llm_base_config=cfg, device=gpu_device)
    lm.load_state_dict({"dnn." + k: v for k, v in sd.items()})
    mini = dict(n_filters=32, ratios=(2, 4), dimension=128, enc_heads=2, enc_layers=1, sem_in=64, sem_ch=64, sem_strides=(2, 1),
                code_dim=128, codebook_size=64, num_quantizers=3, dec_dim=128, dec_inter=256, dec_heads=4, dec_layers=1,
                convnext_layers=2, n_fft=32, hop=8, gn_groups=32)
    csd = synth.hcodec10_state_dict(5, R.HCodecSpec(**mini))
    codec = qa.Codec(None, None, None, spec=qa.HCodecSpec(**mini), device=gpu_device).load_state_dict(csd)
    wav = synth.synth_wav(6, 2, 16 * 64).to(gpu_device).unsqueeze(1)
    feat = synth.synth_feat(7, 2, 16 * 64 // 8, 64).to(gpu_device)
    mix = L.synth_feats(1, 3, 9, spec.feats_dim).to(gpu_device)
    mel = torch.zeros(3, 12, 80)

    for math in (1, 0):
        with with_knob("QA_ATT_MATH", math):
            s0 = _stats(qa_lib)
            lm.generate("se", None, None, mel, mix, global_length=5, do_sample=False)
            torch.cuda.synchronize()
            s1 = _stats(qa_lib)
            codec.encode(wav, feat)
            torch.cuda.synchronize()
            s2 = _stats(qa_lib)
        assert s1[0] > s0[0] and s1[1] == s0[1], f"QA_ATT_MATH={math}: LM launches (fp32, split) {s0} -> {s1}"
        codec_form = 1 if math else 0
        assert s2[codec_form] > s1[codec_form] and s2[1 - codec_form] == s1[1 - codec_form], \
            f"QA_ATT_MATH={math}: codec launches (fp32, split) {s1} -> {s2}"


OPERANDS = {"Q": 256, "K": 512, "V": 1024, "P": 2048}


@pytest.mark.parametrize("hd", (32, 64, 96, 128))
def test_every_plane_of_every_operand_is_read(qa_lib, gpu_device, hd):
    from unified_audio_amd import _lib

    c = Case("self", B=2, H=3, hd=hd, n_q=129, n_keys=129)
    p = pack(c, make_inputs(c, "randn", _seed(c, "planes")), gpu_device)
    # relative size of what a plane of ONE operand carries: h the value itself, m <= 2^-8, l <= 2^-16 of it.  The windows are wide
    # (averaging over keys and d shrinks the change); the lower ends sit above the 2^-24 of an fp32 rounding only for h and m, so the
    # l plane is required to change the bits at all and to stay below 2^-13.
    windows = {32: (0.05, 4.0), 64: (2.0 ** -16, 2.0 ** -5), 128: (0.0, 2.0 ** -13)}
    with with_knob("QA_ATT_MATH", 1), with_knob("QA_ATT_DEBUG", 0):
        ref = launch(qa_lib, c, p)
        scale = float(ref.abs().max())
        for op, sel in list(OPERANDS.items()) + [("all", 0)]:
            for bit, (lo, hi) in windows.items():
                _lib.set_knob("QA_ATT_DEBUG", bit | sel)
                out = launch(qa_lib, c, p)
                d = float((out - ref).abs().max()) / scale
                print(f"ATTN-PLANE hd{hd} {op} bit {bit}: max |delta| / max |o| = {d:.3e}")
                assert not torch.equal(out, ref), f"{op} plane bit {bit}: the output did not change"
                assert lo <= d < hi, f"{op} plane bit {bit}: change {d:.3e} outside [{lo:.1e}, {hi:.1e})"
        _lib.set_knob("QA_ATT_DEBUG", 0)
        assert torch.equal(launch(qa_lib, c, p), ref)
    with with_knob("QA_ATT_MATH", 0), with_knob("QA_ATT_DEBUG", 0):
        ref0 = launch(qa_lib, c, p)
        _lib.set_knob("QA_ATT_DEBUG", 32 | 64 | 128)
        assert torch.equal(launch(qa_lib, c, p), ref0), "the fp32 chain has no planes"


def test_probability_split_equals_split4_rne_on_the_unit_interval(qa_lib, gpu_device):
    fn = qa_lib.qa_debug_att_split_unit
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p]
    g = torch.Generator().manual_seed(11)
    # every binade of (0, 1] down to the subnormals with random mantissas, the bf16 rounding ties, 0, 1 and what exp2 returns
    expo = torch.arange(-149, 1, dtype=torch.float64)
    mant = 1.0 + torch.rand(len(expo), 512, generator=g, dtype=torch.float64)
    binades = (mant * torch.exp2(expo).view(-1, 1)).clamp(max=1.0).float().reshape(-1)
    ties = (torch.arange(128, 256, dtype=torch.float64).view(-1, 1) / 256 + torch.tensor([2.0 ** -9, 2.0 ** -9 + 2.0 ** -24, 2.0 ** -17])).float()
    probs = torch.exp2(-40.0 * torch.rand(1 << 16, generator=g))
    x = torch.cat([binades, ties.reshape(-1), probs, torch.tensor([0.0, 1.0, 2.0 ** -126, 2.0 ** -149])])
    x = torch.cat([x, torch.zeros((-len(x)) % 4)]).to(gpu_device)
    assert float(x.min()) >= 0.0 and float(x.max()) <= 1.0
    bad = torch.zeros(1, dtype=torch.int64, device=gpu_device)
    assert fn(x.data_ptr(), x.numel(), bad.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0, qa_lib.qa_last_error()
    torch.cuda.synchronize()
    assert int(bad.item()) == 0, f"{int(bad.item())} of {x.numel() // 4} groups split differently"


# ------------------------------------------------------------------------------------------------ (e) key-padding mask
def _kmask_launch(lib, c, qkv, valid):
    fn = lib.qa_debug_attention_kmask
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_int,
                   C.c_longlong, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p]
    d, ldo = c.d, c.d + 4
    buf, out = guarded_out(c.B * c.n_q, d, ldo, OUT_HEAD, torch.device("cuda"))
    st = fn(qkv.data_ptr(), 3 * d, qkv.data_ptr() + 4 * d, qkv.data_ptr() + 8 * d, 3 * d, out.data_ptr(), ldo, c.B, c.n_q, c.n_keys,
            c.n_keys * 3 * d, c.H, c.hd, c.hd ** -0.5, valid.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert st == 0, lib.qa_last_error()
    torch.cuda.synchronize()
    check_guarded_out(buf, out, OUT_HEAD)
    return out.reshape(c.B, c.n_q, c.H, c.hd).clone()


def _kmask_truth(c, x, valid, dtype):
    q, k, v = (x[n].transpose(1, 2).to(dtype) for n in ("q", "k", "v"))
    s = (q * c.hd ** -0.5) @ k.transpose(-1, -2)
    s = s.masked_fill(~valid.view(c.B, 1, 1, c.n_keys), float("-inf"))
    m = s.amax(-1, keepdim=True)
    p = torch.exp(s - torch.where(torch.isfinite(m), m, torch.zeros_like(m)))
    l = p.sum(-1, keepdim=True)
    return ((p @ v) / torch.where(l > 0, l, torch.ones_like(l))).transpose(1, 2), s


KMASK_LENGTHS = {  # n -> valid keys per batch item: tile edges, a lone key, a hole in the middle (item 3), nothing (item 4)
    33: (33, 1, 32, 31, 0),
    283: (283, 129, 250, 64, 0),
}


@pytest.mark.parametrize("n", sorted(KMASK_LENGTHS))
@pytest.mark.parametrize("hd", (32, 64, 96, 128))
def test_key_padding_mask_both_forms_meet_the_fp64_bound(qa_lib, gpu_device, hd, n):
    lens = KMASK_LENGTHS[n]
    c = Case("self", B=len(lens), H=3, hd=hd, n_q=n, n_keys=n)
    x = make_inputs(c, "randn", _seed(c, "kmask"))
    valid = torch.arange(n).view(1, -1) < torch.tensor(lens).view(-1, 1)
    valid[3, lens[3] // 2] = False  # a padded key between valid ones
    qkv = torch.cat([x[k].reshape(c.B, n, c.d) for k in ("q", "k", "v")], dim=-1).contiguous().to(gpu_device)
    vbytes = valid.to(torch.uint8).contiguous().to(gpu_device)
    t64, s64 = _kmask_truth(c, x, valid, torch.float64)
    t32, _ = _kmask_truth(c, x, valid, torch.float32)
    scale = float(t64.abs().max())
    e_cpu = float((t32.double() - t64).abs().max()) / scale
    s_max = float(s64[torch.isfinite(s64)].abs().max())
    bound = C_PARITY * max(e_cpu, E_FLOOR, S_ULP * s_max)
    e, bad = {}, []
    for math in (0, 1):
        with with_knob("QA_ATT_MATH", math):
            before = _stats(qa_lib)
            out = _kmask_launch(qa_lib, c, qkv, vbytes).cpu()
            after = _stats(qa_lib)
        assert after[math] == before[math] + 1, "the knob did not select the kernel form"
        e[math] = float((out.double() - t64).abs().max()) / scale
        if not torch.equal(out[4], torch.zeros_like(out[4])):
            bad.append(f"QA_ATT_MATH={math}: an item whose keys are all padding is not exactly 0")
        if not e[math] <= bound:
            bad.append(f"QA_ATT_MATH={math}: e_hip {e[math]:.3e} > bound {bound:.3e} (e_cpu32 {e_cpu:.3e})")
    RATIOS.append(("kmask", f"kmask_hd{hd}_n{n}", e[0], e[1]))
    print(f"ATTN-SPLIT kmask hd{hd} n{n}: e_chain {e[0]:.3e} e_split {e[1]:.3e} bound {bound:.3e} ratio {e[1] / max(e[0], 1e-300):.3f}")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("math", (0, 1))
@pytest.mark.parametrize("hd", (32, 64, 96, 128))
def test_all_masked_rows_are_exactly_zero(qa_lib, gpu_device, hd, math):
    c = Case("ring", B=2, H=3, hd=hd, n_q=37, n_keys=37, ring_end=37 * 4 + 20, context=37)  # query 0 sees nothing
    blind = ~reference_mask(c, torch.arange(c.n_q)).any(-1)
    assert blind.any() and not blind.all()
    p = pack(c, make_inputs(c, "randn", _seed(c, "blind")), gpu_device)
    with with_knob("QA_ATT_MATH", math):
        out = launch(qa_lib, c, p).cpu()
    assert torch.equal(out[:, blind], torch.zeros_like(out[:, blind]))
    assert bool(torch.isfinite(out).all()) and float(out[:, ~blind].abs().max()) > 0


def test_split_ratio_report():
    by = {}
    for mode, name, e0, e1 in RATIOS:
        by.setdefault(mode, []).append((e0, e1))
    for mode, v in sorted(by.items()):
        e0 = max(a for a, _ in v)
        e1 = max(b for _, b in v)
        print(f"ATTN-SPLIT-SUMMARY {mode}: {len(v)} cases, max e_chain {e0:.2e}, max e_split {e1:.2e}, ratio {e1 / max(e0, 1e-300):.3f}")
