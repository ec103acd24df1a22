"""tests/agg_ref.py is what tests/test_agg_kernels_gpu.py takes for the truth: here every restatement is pinned to the project's oracle
(oracle/hcodec15_ref.py), and every align case of the GPU module is shown to be decided - its closest similarity at least
agg_ref.MIN_MARGIN from the threshold, the oracle's float32 and float64 groupings equal - so the GPU module compares integers exactly
and skips nothing.  The one case that sits ON its threshold does so exactly, in both precisions, by construction."""
import dataclasses

import pytest
import torch

from oracle import hcodec15_ref as R15
from tests import agg_ref as A

F64, I64 = torch.float64, torch.int64


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _oracle_groups(h, thr, mt):
    """similarity_alignment on h [1, n, D] -> (seg [n], start [nseg], len [nseg]), start / len from the alignment matrix."""
    seg, nseg, _ = R15.similarity_alignment(h, thr, mt)
    am = R15.alignment_matrix(seg)[0]  # [G, n]
    assert am.shape[0] == int(nseg[0])
    return seg[0], am.argmax(1), am.sum(1).long()


# ------------------------------------------------------------------------------------------------ the cases, and align_ref on them
@pytest.mark.parametrize("case", A.ALIGN_CASES, ids=[c["id"] for c in A.ALIGN_CASES])
def test_align_cases_are_decided_and_align_ref_is_the_oracle(case):
    h = A.align_input(case)
    B, T, _ = h.shape
    thr, mt, lens = case["thr"], case["mt"], case["lens"]
    if case["kind"] == "tie":
        for dt in (torch.float32, F64):
            assert A.cosine_sims(h[0], dt).tolist() == [1.0] and thr == 1.0, "the tie case must sit on its threshold exactly"
            assert torch.nn.functional.cosine_similarity(h[:, :-1].to(dt), h[:, 1:].to(dt), dim=2).tolist() == [[1.0]]
    else:
        m = A.margin(case)
        assert m >= A.MIN_MARGIN, f"closest similarity {m:.3e} from the threshold"
        assert m == float("inf") or abs(A.margin(case, torch.float32) - m) < 1e-5  # inf: no frame pair (T = 1)
    seg, start, ln, nseg, gmax = A.align_ref(h, thr, mt, lens)
    assert gmax == int(nseg.max())
    for b in range(B):
        n = A.clip_len(lens, b, T)
        s32, st32, l32 = _oracle_groups(h[b:b + 1, :n], thr, mt)
        s64, st64, l64 = _oracle_groups(h[b:b + 1, :n].double(), thr, mt)
        assert torch.equal(s32, s64) and torch.equal(st32, st64) and torch.equal(l32, l64), "float32 and float64 groupings differ"
        G = int(nseg[b])
        assert G == len(st64)
        assert torch.equal(seg[b, :n], s64) and torch.equal(start[b, :G], st64) and torch.equal(ln[b, :G], l64)
        assert (seg[b, n:] == A.UNWRITTEN).all() and (start[b, G:] == T).all() and (ln[b, G:] == 0).all()
        assert int(ln[b].sum()) == n and int(ln[b].max()) <= mt
        if lens is not None:  # the clip in the batch is the clip alone at T = lens[b]
            a = A.align_ref(h[b:b + 1, :n], thr, mt)
            assert torch.equal(a[0][0], seg[b, :n]) and torch.equal(a[1][0, :G], start[b, :G]) and torch.equal(a[2][0, :G], ln[b, :G])
            assert int(a[3][0]) == G


def test_align_cases_reach_the_branches():
    """What the whole-codec tests reach only by luck: a run cut by the cap, a group of exactly max_tokens that ends on the last frame, a
    remainder group of one frame, nseg == T, and the boundary pair around a zero frame."""
    seen = set()
    for case in A.ALIGN_CASES:
        h = A.align_input(case)
        B, T, _ = h.shape
        seg, start, ln, nseg, _ = A.align_ref(h, case["thr"], case["mt"], case["lens"])
        for b in range(B):
            n, G = A.clip_len(case["lens"], b, T), int(nseg[b])
            sims = A.cosine_sims(h[b, :n]).tolist()
            for g in range(1, G):
                if sims[int(start[b, g]) - 1] > case["thr"]:
                    seen.add("cap split")
                    if case["mt"] == 8:
                        seen.add("cap of 8")
            if case["mt"] > 1 and int(ln[b, G - 1]) == case["mt"]:
                seen.add("full group at the end")
            if case["mt"] > 1 and G > 1 and int(ln[b, G - 1]) == 1 and sims[n - 2] > case["thr"]:
                seen.add("remainder of one")
            if G == n and n > 1:
                seen.add("nseg == T")
            if case["kind"] == "same" and b == 1 and n > 21:
                z = int(seg[b, 20])
                assert int(start[b, z]) == 20 and int(ln[b, z]) == 1 and int(start[b, z + 1]) == 21 and int(seg[b, 19]) == z - 1
                seen.add("zero frame")
    assert seen == {"cap split", "cap of 8", "full group at the end", "remainder of one", "nseg == T", "zero frame"}, seen


# ------------------------------------------------------------------------------------------------ aggregator input / read-out
def _oracle_inter(feats, align, nseg, qemb):
    """The interleave of query_token_aggregator (its lines up to `inter`), restated: feats [B, D, T], align [B, G, T] -> [B, T + G, D]."""
    b, d, t = feats.shape
    g = align.shape[1]
    group_mask = torch.arange(g)[None, :] < nseg[:, None]
    last = (align * torch.arange(t)).max(dim=2).values
    frame_len = last.masked_fill(~group_mask, -1).max(dim=1).values + 1
    frame_mask = torch.arange(t)[None, :] < frame_len[:, None]
    last_cnt = last.clone()
    last_cnt[~group_mask] = t + 1
    n_before = (last_cnt.unsqueeze(2) < torch.arange(t)).sum(dim=1)
    queries = (torch.einsum("bgt,bdt->bgd", align, feats) / align.sum(dim=2).clamp(min=1).unsqueeze(-1)).transpose(1, 2)
    src = torch.cat([feats, queries + qemb.view(1, d, 1)], dim=2)
    dest = torch.cat([torch.arange(t) + n_before, last + torch.arange(g) + 1], dim=1).to(torch.long)
    perm = dest.masked_fill(~torch.cat([frame_mask, group_mask], dim=1), t + g).argsort(dim=1, stable=True)
    return torch.gather(src, 2, perm.unsqueeze(1).expand(-1, d, -1)).transpose(1, 2)


RECT = [c for c in A.AGG_CASES if c["lens"] is None and c["shape"][2] != 1024]


@pytest.mark.parametrize("extra", [0, 3])
@pytest.mark.parametrize("case", RECT, ids=[c["id"] for c in RECT])
def test_agg_build_and_gather_ref_are_the_oracle(case, extra):
    h = A.align_input(case)
    B, T, D = h.shape
    g = _gen(3)
    feats, qemb = torch.randn(B, T, D, generator=g, dtype=F64), torch.randn(D, generator=g, dtype=F64)
    seg, start, ln, nseg, gmax = A.align_ref(h, case["thr"], case["mt"])
    G = gmax + extra
    align = torch.cat([R15.alignment_matrix(seg).double(), torch.zeros(B, extra, T, dtype=F64)], dim=1)
    built = A.agg_build_ref(feats, seg, start, ln, nseg, qemb, G)
    assert not torch.isnan(built).any(), "the rectangular form fills every position"
    want = _oracle_inter(feats.transpose(1, 2), align, nseg, qemb)
    torch.testing.assert_close(built, want, rtol=1e-13, atol=1e-13)
    frames = torch.ones(B, T + G, dtype=torch.bool)  # frame rows and padded-group rows are copies
    for b in range(B):
        for k in range(int(nseg[b])):
            frames[b, int(start[b, k]) + int(ln[b, k]) + k] = False
    assert torch.equal(built[frames], want[frames])
    spec = dataclasses.replace(R15.SPEC_15, agg_layers=0, agg_heads=1)
    out = R15.query_token_aggregator({"a.query_embedding": qemb.view(1, D, 1)}, "a", feats.transpose(1, 2), align, nseg, spec)
    torch.testing.assert_close(A.agg_gather_ref(built, start, ln, nseg, G), out.transpose(1, 2), rtol=1e-13, atol=1e-13)


RAGGED = [c for c in A.AGG_CASES if c["lens"] is not None and c["shape"][2] != 1024]


@pytest.mark.parametrize("case", RAGGED, ids=[c["id"] for c in RAGGED])
def test_per_clip_agg_refs_are_the_clip_alone(case):
    h = A.align_input(case)
    B, T, D = h.shape
    g = _gen(4)
    feats, qemb = torch.randn(B, T, D, generator=g, dtype=F64), torch.randn(D, generator=g, dtype=F64)
    seg, start, ln, nseg, gmax = A.align_ref(h, case["thr"], case["mt"], case["lens"])
    G = gmax + 2
    built = A.agg_build_ref(feats, seg, start, ln, nseg, qemb, G, case["lens"])
    mask = A.agg_key_mask_ref(B, T, G, case["lens"], nseg)
    for b in range(B):
        n, k = case["lens"][b], int(nseg[b])
        a = A.align_ref(h[b:b + 1, :n], case["thr"], case["mt"])
        alone = A.agg_build_ref(feats[b:b + 1, :n], a[0], a[1], a[2], a[3], qemb, k)
        assert torch.equal(built[b, :n + k], alone[0]) and not built[b, n + k:].any()
        assert mask[b].tolist() == [1] * (n + k) + [0] * (T + G - n - k)
        assert torch.equal(A.agg_gather_ref(built, start, ln, nseg, G)[b, :k], A.agg_gather_ref(alone, a[1], a[2], a[3], k)[0])


# ------------------------------------------------------------------------------------------------ length-injected codes
@pytest.mark.parametrize("K", [3, 1024])
@pytest.mark.parametrize("Q", [1, 4])
def test_code_refs_are_the_oracle(K, Q):
    B, G = 3, 37
    idx, ln = A.random_codes(5 + K + Q, B, Q, G, K)
    tl = ln.unsqueeze(1)
    want = (tl - 1) * K + idx.transpose(1, 2)  # encode's `inject`
    codes = A.codes_inject_ref(idx, ln, K, 0)
    assert torch.equal(codes, want)
    minus1 = A.codes_inject_ref(idx, ln, K, 1)
    pad = (ln == 0).unsqueeze(1).expand(-1, Q, -1)
    assert torch.equal(minus1[~pad], want[~pad]) and (minus1[pad] == -1).all() and pad.any()
    for c in (codes, minus1, torch.cat([codes, torch.full((B, Q, 1), -K - 1)], dim=2)):
        plain, lengths = R15.extract_lengths(c, K)
        assert torch.equal(A.token_lengths_ref(c, K), lengths)
        totals, tmax = A.adaptive_frames_ref(c, K)
        assert torch.equal(totals, lengths.clamp_min(0).sum(1)) and tmax == int(totals.max())
    assert torch.equal(A.token_lengths_ref(codes, K), ln) and torch.equal(A.token_lengths_ref(minus1, K), ln)
    assert A.token_lengths_ref(torch.full((1, Q, 1), -K - 1), K).tolist() == [[-1]]
    # de-aggregation: the acoustic stream repeats by the SEMANTIC stream's lengths
    other = A.codes_inject_ref(torch.randint(K, (B, G, Q), generator=_gen(9)), ln, K, 1)
    own = ln.clone()  # groups this stream dropped and the other kept: negative codes that are repeated, as Python's code % K
    own[:, 0] = 0
    own[1, G // 2] = 0
    dropped = [A.codes_inject_ref(idx, own, K, p) for p in (0, 1)]
    dropped[0][2, :, 1] = -K - 1
    for c in (codes, minus1, *dropped):
        plain, _ = R15.extract_lengths(c, K)
        assert c is codes or c is minus1 or bool((c[:, :, 0] < 0).all())
        _, lengths = R15.extract_lengths(other, K)
        o = R15.deaggregate_indices(plain, lengths).transpose(1, 2)  # [B, max total, Q]
        tmax = o.shape[1]
        assert tmax == int(ln.sum(1).max())
        for T in (tmax, tmax + 5, tmax - 7):
            want = torch.zeros(B, T, Q, dtype=I64)
            want[:, :min(T, tmax)] = o[:, :T]
            assert torch.equal(A.deaggregate_ref(c, other, T, K), want)
        cap = [0, int(ln[1].sum()) - 3, tmax]
        capped = A.deaggregate_ref(c, other, tmax, K, cap)
        for b in range(B):  # the item alone, cut to T = cap[b]; index 0 behind
            assert torch.equal(capped[b, :cap[b]], A.deaggregate_ref(c[b:b + 1], other[b:b + 1], cap[b], K)[0]) and not capped[b, cap[b]:].any()


# ------------------------------------------------------------------------------------------------ layout, mask, ring
def test_layout_mask_and_ring_refs():
    g = _gen(11)
    B, N, Q = 3, 7, 4
    src = torch.randint(50, (B, N, Q), generator=g)
    lens = [7, 3, 1]
    live = torch.arange(N)[None, :] < torch.tensor(lens)[:, None]
    assert torch.equal(A.codes_bqn_ref(src, 0), src.permute(0, 2, 1))
    assert torch.equal(A.codes_bqn_ref(src, 0, lens), torch.where(live[:, None, :], src.permute(0, 2, 1), -1))
    assert torch.equal(A.codes_bqn_ref(src.permute(0, 2, 1).contiguous(), 1, lens), torch.where(live[:, :, None], src, -1))
    for mul in (1, 2):
        assert torch.equal(A.len_mask_ref(B, N, lens, mul).bool(), torch.arange(N)[None, :] < mul * torch.tensor(lens)[:, None])
    for cap, T, pos0 in ((5, 3, 4), (5, 5, 37), (32, 1, 10 ** 6 + 3)):
        d = 8
        k, v = torch.randn(B, T, d, generator=g), torch.randn(B, T, d, generator=g)
        kc, vc = torch.randn(B, cap, d, generator=g), torch.randn(B, cap, d, generator=g)
        st = R15.MimiStreamState(B, 1, 1, d, cap)  # RingKVCache.complete with the running offset at pos0
        st.cache[0][0].copy_(kc.unsqueeze(1))
        st.cache[0][1].copy_(vc.unsqueeze(1))
        st.offset = pos0
        ko, vo, _ = st.complete(0, k.unsqueeze(1), v.unsqueeze(1))
        got = A.ring_append_ref(k, v, kc, vc, pos0)
        assert torch.equal(got[0], ko[:, 0]) and torch.equal(got[1], vo[:, 0])
