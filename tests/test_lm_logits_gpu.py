"""The UniSE AR-LM decode step at its LOGITS (qa_lm_enable_taps / qa_lm_tap), not only at its tokens.

(a) fp64 parity, teacher-forced: the oracle re-runs the HIP token stream in float64 (the truth) and in float32 (the yardstick);
    the HIP logits of every (sequence, step) must be within a small multiple of the fp32 oracle's own distance from the truth,
    over the shapes the dispatch code branches on (row groups, tile widths, head dims, fused / unfused MLP, key splits 1 .. 4).
(b) the picked token is the FIRST maximum of the tapped logits (exact ties included); sampled runs meet the same logits bound.
(c) bit-exact invariance: a row's logits do not depend on the batch it is in, the prefetch planes, the row split, the chain count,
    graph replay or the taps themselves (include/quarkaudio.h: "No knob changes results beyond fp32 summation order"; INTEGRATION.md:
    max_segments "changes speed and memory, never a sample").
"""
import pytest
import torch

from oracle import llm_ref as L
from tests.test_llm_gpu import SMALL, _model

pytestmark = pytest.mark.gpu

HD32 = L.LMSpec(hidden=256, n_layers=2, n_heads=8, global_size=1000, semantic_size=1004, feats_dim=64, num_tasks=3)  # head tiles 8 / 4
H512 = L.LMSpec(hidden=512, n_layers=2, n_heads=8, global_size=256, semantic_size=512, feats_dim=64, num_tasks=3)
H1024 = L.LMSpec(hidden=1024, n_layers=2, n_heads=8, global_size=256, semantic_size=384, feats_dim=64, num_tasks=3)

# e = max |l - l64| / rms(l64) over the active slice of one (sequence, step); the HIP bound is C_PARITY * max(e_cpu32, E_FLOOR).
# Measured on MI355X (max over all steps of a case, e_hip / e_cpu32): small b1 1.02e-6 / 1.26e-6, b12 1.37e-6 / 1.78e-6,
# b24 1.41e-6 / 2.17e-6, b48 1.46e-6 / 2.15e-6, b65 1.29e-6 / 2.24e-6, hd32 1.60e-6 / 2.62e-6, unise b5 4.21e-6 / 3.57e-6,
# unise b33 5.05e-6 / 4.14e-6, h512 unfused 1.63e-6 / 2.40e-6, h1024 2.15e-6 / 2.28e-6, long 3.48e-6 / 3.37e-6, long graph
# 4.57e-6 / 4.25e-6, sampled 1.55e-6 / 2.07e-6: the kernel is as close to the truth as the fp32 oracle (ratio <= 1.22).  Bounds of
# 5e-6 .. 1.7e-5; one MLP K-slice partial scaled by 1 + 2^-10 gives 4.4e-4 .. 6.2e-4 (and passes every token-level test).
C_PARITY = 4.0
E_FLOOR = 1e-6


def _inputs(spec, task, B, Nm, Ne, seed):
    mix = L.synth_feats(seed, B, Nm, spec.feats_dim)
    enr = L.synth_feats(seed + 1, B, Ne, spec.feats_dim) if task != "se" else None
    return enr, mix


def _run(lm, spec, dev, task, enr, mix, S, G, **kw):
    """HIP generate with taps on: (gids, sids, logits.global [B, G+1, gs], logits.semantic [B, S, ss]) on the host."""
    B = mix.shape[0]
    mel = torch.zeros(B, S, 80)
    lm.enable_taps(True)
    kw.setdefault("do_sample", False)
    g, s = lm.generate(task, None if enr is None else mel, None if enr is None else enr.to(dev), mel, mix.to(dev), global_length=G, **kw)
    lg = lm.tap("logits.global").view(B, G + 1, spec.global_size)
    ls = lm.tap("logits.semantic").view(B, S, spec.semantic_size)
    torch.cuda.synchronize()
    return g.cpu(), s.cpu(), lg.cpu(), ls.cpu()


def _step_err(hip, truth):
    """[B, T, W] x [B, T, W] -> max over (sequence, step) of max |hip - truth| / rms(truth)."""
    truth = truth.double()
    rms = truth.pow(2).mean(-1).sqrt()
    return float(((hip.double() - truth).abs().amax(-1) / rms).max())


def _oracle_logits(sd, spec, task, enr, mix, S, G, gids, sids, dtype):
    """Teacher-forced oracle on the HIP stream (like test_llm_gpu._audit): the slice logits of every step, [B, G+1, gs], [B, S, ss]."""
    B = mix.shape[0]
    # the discarded (G+1)-th global token is never fed back (the semantic phase restarts from its own first id): any id will do
    forced = torch.cat([gids + spec.global_offset, torch.full((B, 1), spec.global_offset), sids + spec.semantic_offset], dim=1)
    out = []
    L.generate(sd, task, enr, mix, S, G, spec, forced=forced, logits_out=out, dtype=dtype)
    go, so = spec.global_offset, spec.semantic_offset
    lg = torch.stack([x[:, go:go + spec.global_size] for x in out[:G + 1]], dim=1)
    ls = torch.stack([x[:, so:so + spec.semantic_size] for x in out[G + 1:]], dim=1)
    return lg, ls


def _first_argmax(x):
    """Index of the FIRST maximum along the last axis (the pick's tie rule), independent of torch.argmax's tie behaviour."""
    m = x.amax(-1, keepdim=True)
    idx = torch.arange(x.shape[-1]).expand_as(x)
    return torch.where(x == m, idx, x.shape[-1]).amin(-1)


def _check_picks(gids, sids, lg, ls, G):
    assert torch.equal(gids, _first_argmax(lg[:, :G])), "a global token is not the first maximum of its step's tapped logits"
    assert torch.equal(sids, _first_argmax(ls)), "a semantic token is not the first maximum of its step's tapped logits"


def _parity(sd, spec, task, enr, mix, S, G, gids, sids, lg, ls, label):
    lg64, ls64 = _oracle_logits(sd, spec, task, enr, mix, S, G, gids, sids, torch.float64)
    lg32, ls32 = _oracle_logits(sd, spec, task, enr, mix, S, G, gids, sids, torch.float32)
    e_hip = max(_step_err(lg, lg64), _step_err(ls, ls64))
    e_cpu = max(_step_err(lg32, lg64), _step_err(ls32, ls64))
    bound = C_PARITY * max(e_cpu, E_FLOOR)
    print(f"logits parity {label}: e_hip {e_hip:.3e} e_cpu32 {e_cpu:.3e} bound {bound:.3e}")
    assert e_hip <= bound, f"{label}: HIP logits {e_hip:.3e} from the fp64 truth, bound {bound:.3e} (fp32 oracle {e_cpu:.3e})"
    return e_hip, e_cpu


# (spec, weight seed, task, B, n_mix, n_enroll, S, G, knobs): every branch of the decode step's dispatch
PARITY_CASES = {
    # hidden 256 / 4 heads (hd 64): o_proj without the 8-row kernel (K share of one 32-wide chunk), fused MLP NB = 1, head tile 4
    "small_b1_se": (SMALL, 21, "se", 1, 9, 0, 12, 5, {}),
    "small_b12_tse": (SMALL, 22, "tse", 12, 9, 7, 12, 5, {}),     # 9 .. 16 rows: the 8-row split of the qkv / MLP launches
    "small_b24_se": (SMALL, 23, "se", 24, 7, 0, 10, 4, {}),       # 17 .. 32: 16-row groups, two row tiles
    "small_b48_tse": (SMALL, 24, "tse", 48, 6, 5, 10, 4, {}),     # 33 .. 64: 32-row groups (fused MLP: 16 below hidden 512)
    "small_b65_se": (SMALL, 25, "se", 65, 6, 0, 10, 4, {}),       # > 64: two chains replaying captured steps
    # hd 32 (lm_attn_kernel<32>), head tile 8 (global 1000) and 4 (semantic 1004: not a multiple of 8)
    "hd32_tiles8_4_tse": (HD32, 26, "tse", 9, 8, 6, 10, 4, {}),
    # the UniSE shape: 12 x 512, R8 o_proj (width 4 / 8 / 16 by batch), fused MLP NB = 2, head tile 16
    "unise_b5_se": (L.SPEC_UNISE, 33, "se", 5, 20, 0, 10, 6, {}),
    "unise_b33_tse": (L.SPEC_UNISE, 34, "tse", 33, 12, 8, 8, 4, {}),
    # hidden 512 with the fused MLP off at create: gate/up + down GEMVs (down K = 2048, NB = 8)
    "h512_unfused_b20_se": (H512, 27, "se", 20, 10, 0, 10, 4, {"QA_LM_MLP_FUSED": 0}),
    # hidden 1024 / hd 128: no fused MLP at this width, lm_attn_kernel<128>, o_proj NB = 4
    "h1024_b6_tse": (H1024, 28, "tse", 6, 8, 5, 8, 4, {}),
    # decode from ~200 to ~1110 keys: the attention's key split runs 1 -> 4 (cap 1152: 18 tiles per split), host-driven and replayed
    "small_long_se": (SMALL, 29, "se", 3, 200, 0, 900, 8, {}),
    "small_long_graph_tse": (SMALL, 30, "tse", 2, 150, 50, 900, 8, {"QA_LM_GRAPH": 1}),
}


@pytest.mark.parametrize("case", list(PARITY_CASES))
def test_decode_logits_match_fp64_oracle_teacher_forced(qa_lib, gpu_device, knob, case):
    spec, seed, task, B, Nm, Ne, S, G, knobs = PARITY_CASES[case]
    for k, v in knobs.items():
        knob(k, v)
    sd, lm = _model(spec, seed, gpu_device)  # after the knobs: QA_LM_MLP_FUSED is read at create
    enr, mix = _inputs(spec, task, B, Nm, Ne, seed + 100)
    gids, sids, lg, ls = _run(lm, spec, gpu_device, task, enr, mix, S, G)
    assert torch.isfinite(lg).all() and torch.isfinite(ls).all()
    _check_picks(gids, sids, lg, ls, G)
    _parity(sd, spec, task, enr, mix, S, G, gids, sids, lg, ls, case)


def test_pick_takes_the_first_of_exactly_tied_maxima_across_tiles(qa_lib, gpu_device):
    """Duplicated output_head rows give bit-identical logits (each column's K order is the same): ties inside a head tile (shuffle
    merge of the GM_HEAD epilogue) and across tiles (lm_pick_kernel, including a lane that walks several tiles at 256 tiles of the
    UniSE semantic slice) must resolve to the lowest index, like torch.argmax on the reference's logits."""
    for spec, pairs in ((SMALL, ((7, 90), (20, 21), (2, 150))), (L.SPEC_UNISE, ((5, 4000), (100, 101), (64, 8000)))):
        sd = L.lm_state_dict(41, spec)
        w = sd["output_head.weight"].clone()
        go, so = spec.global_offset, spec.semantic_offset
        (g1, g2), (g3, g4), (s1, s2) = pairs
        for a, b in ((go + g1, go + g2), (go + g3, go + g4), (so + s1, so + s2)):
            w[a] = 4.0 * w[a]  # large rows: they win most steps
            w[b] = w[a]
        sd["output_head.weight"] = w
        import unified_audio_amd as qa

        cfg = dict(global_size=spec.global_size, semantic_size=spec.semantic_size, hidden_size=spec.hidden,
                   num_layers=spec.n_layers, num_attention_heads=spec.n_heads)
        lm = qa.LLM_SFT(num_tasks=spec.num_tasks, feats_dim=spec.feats_dim, llm_base_config=cfg, device=gpu_device).load_state_dict(sd)
        enr, mix = _inputs(spec, "se", 40, 6, 0, 7)
        S, G = 12, 6
        gids, sids, lg, ls = _run(lm, spec, gpu_device, "se", enr, mix, S, G)
        _check_picks(gids, sids, lg, ls, G)
        ties = int((lg[:, :G, g1] == lg[:, :G, g2]).logical_and(gids == g1).sum()) + int((ls[..., s1] == ls[..., s2]).logical_and(sids == s1).sum())
        assert ties > 0, "no exact tie was decided: the case does not test the tie rule"
        assert not (gids == g2).any() and not (gids == g4).any() and not (sids == s2).any()


def test_sampled_decode_logits_match_fp64_oracle(qa_lib, gpu_device):
    """generate_sampled computes the same logits as the greedy path (the sampler reads the head's stored slice): teacher-forced on
    the sampled stream they meet the same fp64 bound."""
    spec = SMALL
    sd, lm = _model(spec, 31, gpu_device)
    enr, mix = _inputs(spec, "tse", 12, 8, 6, 131)
    torch.manual_seed(5)
    gids, sids, lg, ls = _run(lm, spec, gpu_device, "tse", enr, mix, 14, 6, do_sample=True)
    assert int(gids.min()) >= 0 and int(gids.max()) < spec.global_size and int(sids.max()) < spec.semantic_size
    # a sampled token survives the filters: its logit is finite and within the top-50 of its step (top_k default)
    rank_g = (lg[:, :6] > lg[:, :6].gather(-1, gids[..., None])).sum(-1)
    rank_s = (ls > ls.gather(-1, sids[..., None])).sum(-1)
    assert int(rank_g.max()) < 50 and int(rank_s.max()) < 50
    _parity(sd, spec, "tse", enr, mix, 14, 6, gids, sids, lg, ls, "sampled_small_b12_tse")


# ------------------------------------------------------------------------------------------- (c) bit-exact invariance

BATCHES = (1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 47, 48, 63, 64, 65)


@pytest.mark.parametrize("spec_name", ["small", "unise"])
@pytest.mark.parametrize("cache", ["short", "long"])
def test_logits_are_bit_identical_for_every_batch_size(qa_lib, gpu_device, spec_name, cache):
    """The first B rows of one fixed 66-sequence batch (two captured chains of 33) for every B across the row-group (8 / 16 / 32), o_proj
    tile-width (4 / 8 / 16) and chain (> 64) boundaries - including ADVICE r05's B = 32 against 33 at hidden 256 - give bit-identical
    logits.  `long`: the cache crosses 256 keys during the decode, so host-driven steps (B <= 64) and replayed steps (B = 65, 66)
    both run more than one key split."""
    spec = SMALL if spec_name == "small" else L.SPEC_UNISE
    _, lm = _model(spec, 43, gpu_device)
    Nm, S, G = (6, 10, 4) if cache == "short" else (240, 24, 4)  # long: prompt 242, keys 242 .. 270 (cap 320)
    enr, mix = _inputs(spec, "tse", 66, Nm, 5, 17)
    _, _, lg, ls = _run(lm, spec, gpu_device, "tse", enr, mix, S, G)
    bad = []
    for B in BATCHES:
        _, _, lgb, lsb = _run(lm, spec, gpu_device, "tse", enr[:B], mix[:B], S, G)
        if not (torch.equal(lgb, lg[:B]) and torch.equal(lsb, ls[:B])):
            bad.append(B)
    assert not bad, f"batch sizes whose logits differ from the same rows of the 66-sequence batch: {bad}"


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("B", [16, 40])
def test_prefetch_planes_do_not_change_a_bit(qa_lib, gpu_device, knob, B):
    """QA_LM_PF planes only touch weights the next launch streams (lm_decode.h PfArgs: a hint that cannot change a result)."""
    spec = L.SPEC_UNISE
    _, lm = _model(spec, 44, gpu_device)
    enr, mix = _inputs(spec, "se", B, 20, 0, 18)
    ref = _run(lm, spec, gpu_device, "se", enr, mix, 10, 4)
    for pf in (0, 1, 2, 4, 8, 15):
        knob("QA_LM_PF", pf)
        assert _same(_run(lm, spec, gpu_device, "se", enr, mix, 10, 4), ref), pf


@pytest.mark.parametrize("B", [9, 16])
def test_row_split_does_not_change_a_bit(qa_lib, gpu_device, knob, B):
    """QA_LM_ROWSPLIT (8-row groups of the qkv / fused-MLP launches at 9 .. 16 sequences) is a schedule, not a result; the captured
    step's graph is keyed by it, so a replayed step follows the knob too."""
    spec = L.SPEC_UNISE
    _, lm = _model(spec, 45, gpu_device)
    enr, mix = _inputs(spec, "tse", B, 12, 6, 19)
    ref = _run(lm, spec, gpu_device, "tse", enr, mix, 8, 4)
    for graph in (0, 1):
        knob("QA_LM_GRAPH", graph)
        for rs in (0, 1, 2, 3):
            knob("QA_LM_ROWSPLIT", rs)
            assert _same(_run(lm, spec, gpu_device, "tse", enr, mix, 8, 4), ref), (graph, rs)


@pytest.mark.parametrize("spec_name", ["small", "unise"])
def test_chains_and_graph_replay_do_not_change_a_bit(qa_lib, gpu_device, knob, spec_name):
    """QA_LM_CHAINS 1 / 2 / 4 against the default, QA_LM_GRAPH 1 against 0, with a cache that crosses 256 keys (small spec: also 512)."""
    spec = SMALL if spec_name == "small" else L.SPEC_UNISE
    _, lm = _model(spec, 46, gpu_device)
    B, Nm, S, G = (40, 200, 350, 4) if spec_name == "small" else (24, 230, 40, 4)
    enr, mix = _inputs(spec, "se", B, Nm, 0, 20)
    ref = _run(lm, spec, gpu_device, "se", enr, mix, S, G)
    for chains in (1, 2, 4):
        knob("QA_LM_CHAINS", chains)
        assert _same(_run(lm, spec, gpu_device, "se", enr, mix, S, G), ref), chains
    knob("QA_LM_CHAINS", 0)
    knob("QA_LM_GRAPH", 1)
    assert _same(_run(lm, spec, gpu_device, "se", enr, mix, S, G), ref), "graph replay"


def test_taps_change_no_token_and_repeat_bit_exactly(qa_lib, gpu_device):
    """Taps are a test hook: tokens with taps on equal tokens with taps off (greedy and sampled, one chain and two), two identical
    calls give identical logits, a tap of a call made with taps off is refused, and taps under a caller's stream capture are refused."""
    import unified_audio_amd as qa

    spec = SMALL
    _, lm = _model(spec, 47, gpu_device)
    for B in (12, 70):
        enr, mix = _inputs(spec, "tse", B, 8, 5, 21)
        mel = torch.zeros(B, 9, 80)
        args = ("tse", mel, enr.to(gpu_device), mel, mix.to(gpu_device))
        for kw in (dict(do_sample=False), dict(do_sample=True)):
            lm.enable_taps(False)
            torch.manual_seed(3)
            off = lm.generate(*args, global_length=4, **kw)
            with pytest.raises(qa.QuarkAudioError, match="no intermediate"):
                lm.tap("logits.global")
            lm.enable_taps(True)
            torch.manual_seed(3)
            on = lm.generate(*args, global_length=4, **kw)
            t1 = (lm.tap("logits.global"), lm.tap("logits.semantic"))
            torch.manual_seed(3)
            on2 = lm.generate(*args, global_length=4, **kw)
            t2 = (lm.tap("logits.global"), lm.tap("logits.semantic"))
            torch.cuda.synchronize()
            assert _same(off, on) and _same(on, on2), (B, kw)
            assert _same(t1, t2), (B, kw)
            assert t1[0].numel() == B * 5 * spec.global_size and t1[1].numel() == B * 9 * spec.semantic_size
    with pytest.raises(qa.QuarkAudioError, match="no intermediate"):
        lm.tap("logits.nothing")
    # a caller's stream capture: refused with the reason (taps allocate and synchronise)
    lm.enable_taps(True)
    mix = L.synth_feats(3, 4, 6, spec.feats_dim).to(gpu_device)
    mel = torch.zeros(4, 5, 80)
    side = torch.cuda.Stream(gpu_device)
    side.wait_stream(torch.cuda.current_stream(gpu_device))
    g = torch.cuda.CUDAGraph()
    with pytest.raises(qa.QuarkAudioError, match="stream capture"):
        with torch.cuda.graph(g, stream=side):
            lm.generate("se", None, None, mel, mix, global_length=3, do_sample=False)
    lm.enable_taps(False)
    torch.cuda.synchronize()
