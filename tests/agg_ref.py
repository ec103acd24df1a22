"""TEST INFRASTRUCTURE ONLY - plain restatements of the second half of csrc/ew.hip: the H-Codec 1.5 adaptive-frame-rate kernels (align,
agg_*, codes_inject, adaptive_frames, token_lengths, deaggregate), the code layout (codes_to / from_bqn), the length mask and the ring
cache append.  One function per kernel, loops over float64 / int64 on the CPU, in the library's own layouts.  tests/test_agg_ref_cpu.py
pins them to oracle/hcodec15_ref.py; tests/test_agg_kernels_gpu.py holds the kernels against them.

Per-clip lengths: `lens` (B frame counts) makes clip b the clip run alone at T = lens[b] (the rule of ew_ref.per_clip).  What a kernel
leaves unwritten is UNWRITTEN in the integer references - the tests fill their integer outputs with the same value, so one torch.equal
checks both what is written and what is not.

The second part builds the align inputs: frames whose consecutive cosine similarities are CHOSEN (chosen_frames), so that no case sits
near its threshold and integer output is compared exactly, with nothing skipped."""
from __future__ import annotations

import functools
import math

import torch

F64 = torch.float64
I64 = torch.int64
UNWRITTEN = -0x7777  # the fill of every integer output buffer of the tests: never a valid group index, start, length or code


def clip_len(lens, b, T):
    """Frames of clip b: the kernels clamp lens[b] to [1, T]."""
    return T if lens is None else min(max(int(lens[b]), 1), T)


# ------------------------------------------------------------------------------------------------ align
def cosine_sims(x, dtype=F64):
    """x [n, D] -> [n - 1]: (x_t / max(|x_t|, 1e-8)) . (x_t+1 / max(|x_t+1|, 1e-8))."""
    x = x.to(dtype)
    u = x / x.pow(2).sum(1).sqrt().clamp_min(1e-8)[:, None]
    return (u[:-1] * u[1:]).sum(1)


def align_ref(h, thr, max_tokens, lens=None):
    """h [B, T, D] -> (seg [B, T], start [B, T], len [B, T], nseg [B], gmax).  A new run starts at frame 0 and wherever sim <= thr; a run
    is cut into groups of max_tokens frames.  start / len behind nseg[b] are T / 0; seg behind lens[b] is UNWRITTEN."""
    B, T, _ = h.shape
    seg = torch.full((B, T), UNWRITTEN, dtype=I64)
    start = torch.full((B, T), T, dtype=I64)
    ln = torch.zeros((B, T), dtype=I64)
    nseg = torch.zeros(B, dtype=I64)
    for b in range(B):
        n = clip_len(lens, b, T)
        sim = cosine_sims(h[b, :n]).tolist()
        g, run = -1, 0
        for t in range(n):
            run = 0 if t == 0 or sim[t - 1] <= thr else run + 1
            if run % max_tokens == 0:
                g += 1
                start[b, g] = t
            seg[b, t] = g
            ln[b, g] += 1
        nseg[b] = g + 1
    return seg, start, ln, nseg, int(nseg.max())


# ------------------------------------------------------------------------------------------------ aggregator input / read-out
def agg_build_ref(feats, seg, start, ln, nseg, qemb, G, lens=None, dtype=F64):
    """feats [B, T, D], qemb [D] -> [B, T + G, D]: frame t at t + seg[t], the query of group g (mean of its frames + qemb) behind the
    group's last frame at start + len + g, padded groups (g >= nseg[b]) at T + g with the bare qemb.  With lens the row holds
    lens[b] + nseg[b] positions, as for the clip alone, and exact zeros behind.  dtype float32: torch's own mean + embedding."""
    B, T, D = feats.shape
    x, q = feats.to(dtype), qemb.to(dtype)
    out = torch.full((B, T + G, D), float("nan"), dtype=dtype) if lens is None else torch.zeros(B, T + G, D, dtype=dtype)
    for b in range(B):
        for t in range(clip_len(lens, b, T)):
            out[b, t + int(seg[b, t])] = x[b, t]
        for g in range(G):
            if g < int(nseg[b]):
                s, n = int(start[b, g]), int(ln[b, g])
                out[b, s + n + g] = x[b, s:s + n].mean(0) + q
            elif lens is None:
                out[b, T + g] = q
    return out


def agg_key_mask_ref(B, T, G, lens, nseg):
    """valid [B, T + G] bytes: 1 for the lens[b] + nseg[b] positions of clip b's interleaved row."""
    out = torch.zeros(B, T + G, dtype=torch.uint8)
    for b in range(B):
        out[b, :clip_len(lens, b, T) + int(nseg[b])] = 1
    return out


def agg_gather_ref(x, start, ln, nseg, G):
    """x [B, T + G, C] -> [B, G, C]: the row at each group's query position, exact zeros for padded groups."""
    B, _, Cc = x.shape
    out = torch.zeros(B, G, Cc, dtype=x.dtype)
    for b in range(B):
        for g in range(min(G, int(nseg[b]))):
            out[b, g] = x[b, int(start[b, g]) + int(ln[b, g]) + g]
    return out


# ------------------------------------------------------------------------------------------------ length-injected codes
def codes_inject_ref(idx, ln, K, pad_minus1):
    """idx [B, G, Q], ln [B, >= G] -> [B, Q, G]: (len - 1) * K + code; a padded group (len 0) gives code - K, or -1 with pad_minus1."""
    B, G, Q = idx.shape
    out = torch.empty(B, Q, G, dtype=I64)
    for b in range(B):
        for g in range(G):
            n = int(ln[b, g])
            for q in range(Q):
                out[b, q, g] = -1 if (pad_minus1 and n == 0) else (n - 1) * K + int(idx[b, g, q])
    return out


def token_lengths_ref(codes, K):
    """codes [B, Q, G] -> [B, G]: floor(code / K) + 1 of quantizer 0 (Python's // floors)."""
    return torch.tensor([[c // K + 1 for c in row] for row in codes[:, 0].tolist()], dtype=I64).reshape(codes.shape[0], codes.shape[2])


def adaptive_frames_ref(codes, K):
    """codes [B, Q, G] -> (totals [B], tmax): the positive token lengths summed per item."""
    totals = token_lengths_ref(codes, K).clamp_min(0).sum(1)
    return totals, int(totals.max())


def deaggregate_ref(codes, len_codes, T, K, cap=None):
    """codes, len_codes [B, Q, G] -> plain indices [B, T, Q]: group g's code % K (Python's %) repeated token_length(len_codes)[g] times,
    cut at T (and at cap[b]), index 0 behind."""
    B, Q, G = codes.shape
    out = [[[0] * Q for _ in range(T)] for _ in range(B)]
    lens = token_lengths_ref(len_codes, K).clamp_min(0).tolist()
    plain = codes.tolist()
    for b in range(B):
        end = T if cap is None else min(max(int(cap[b]), 0), T)
        pos = 0
        for g in range(G):
            for t in range(pos, min(pos + lens[b][g], end)):
                for q in range(Q):
                    out[b][t][q] = plain[b][q][g] % K
            pos += lens[b][g]
    return torch.tensor(out, dtype=I64).reshape(B, T, Q)


def random_codes(seed, B, Q, G, K):
    """Test input: idx [B, G, Q] in [0, K) and len [B, G] in 1 ... 8, item b ending in b + 2 padded groups (len 0) where G allows."""
    g = torch.Generator().manual_seed(seed)
    idx = torch.randint(K, (B, G, Q), generator=g)
    ln = torch.randint(1, 9, (B, G), generator=g)
    for b in range(B):
        ln[b, G - min(b + 2, G - 1):] = 0
    return idx, ln


# ------------------------------------------------------------------------------------------------ layout, mask, ring
def codes_bqn_ref(src, direction, lens=None):
    """direction 0: library [B, N, Q] -> reference [B, Q, N]; 1: back.  Entries at frames n >= lens[b] are -1 whatever the source holds."""
    out = src.transpose(1, 2).clone()
    if lens is not None:
        for b, n in enumerate(lens):
            if direction == 0:
                out[b, :, int(n):] = -1
            else:
                out[b, int(n):, :] = -1
    return out


def len_mask_ref(B, N, lens, mul):
    out = torch.zeros(B, N, dtype=torch.uint8)
    for b in range(B):
        out[b, :max(min(int(lens[b]) * mul, N), 0)] = 1
    return out


def ring_append_ref(k, v, kc, vc, pos0):
    """k, v [B, T, d] into copies of the caches kc, vc [B, cap, d]: row t lands at (pos0 + t) % cap."""
    kc, vc = kc.clone(), vc.clone()
    cap = kc.shape[1]
    for t in range(k.shape[1]):
        kc[:, (pos0 + t) % cap] = k[:, t]
        vc[:, (pos0 + t) % cap] = v[:, t]
    return kc, vc


# ------------------------------------------------------------------------------------------------ inputs without a near-tie
POOL = (-0.3, 0.1, 0.55, 0.97, 0.995)  # the similarities a chosen clip may take: >= 0.05 from the thresholds 0.6 / 0.7 / 0.9
THRESHOLDS = (0.6, 0.7, 0.9)
MAX_TOKENS = (1, 3, 8)
SHAPES = ((1, 1, 8), (2, 2, 12), (3, 41, 8), (4, 17, 260), (2, 300, 1024))
LENS = {(2, 2, 12): (1, 2), (3, 41, 8): (1, 41, 20), (4, 17, 260): (17, 1, 9, 16), (2, 300, 1024): (300, 131)}
MIN_MARGIN = 0.01


def pool_for(thr):
    """The members of POOL at least 0.05 away from thr (thr = 1.0 drops 0.97 and 0.995)."""
    return tuple(s for s in POOL if abs(s - thr) >= 0.05 - 1e-12)


@functools.lru_cache(maxsize=None)
def chosen_frames(seed, B, T, D, pool):
    """[B, T, D] float32: x_0 a random unit vector, x_t+1 = s x_t + sqrt(1 - s^2) u with u a random unit vector orthogonal to x_t and s
    drawn from `pool` (its members above 0.9, if any, four times out of five, so that runs reach max_tokens); every frame scaled by a
    random magnitude in [0.05, 4].  Built in float64, rounded once."""
    g = torch.Generator().manual_seed(seed)
    high = [s for s in pool if s > 0.9]
    low = [s for s in pool if s <= 0.9]
    x = torch.empty(B, T, D, dtype=F64)
    for b in range(B):
        cur = torch.randn(D, generator=g, dtype=F64)
        cur /= cur.norm()
        for t in range(T):
            if t:
                side = high if high and float(torch.rand((), generator=g)) < 0.8 else low
                s = side[int(torch.randint(len(side), (), generator=g))]
                u = torch.randn(D, generator=g, dtype=F64)
                u -= (u @ cur) * cur
                u /= u.norm()
                cur = s * cur + math.sqrt(1.0 - s * s) * u
                cur /= cur.norm()
            x[b, t] = cur
    mag = 0.05 + 3.95 * torch.rand(B, T, 1, generator=g, dtype=F64)
    return (x * mag).float()


def _same_frames():
    """[3, 41, 8]: clip 0 is one frame 41 times; clip 1 the same with an all-zero frame 20 (the eps clamp gives sim 0 on both sides of
    it: boundaries at 20 and 21); clip 2 chosen."""
    h = chosen_frames(77, 3, 41, 8, pool_for(0.9)).clone()
    h[0] = h[0, 0]
    h[1] = h[1, 0]
    h[1, 20] = 0.0
    return h


def _tie_frames():
    """[1, 2, 8]: two identical unit frames of one power-of-two component: every step of the similarity is exact, sim == 1.0 == thr."""
    h = torch.zeros(1, 2, 8)
    h[0, :, 2] = 0.5
    return h


def _cases():
    out = []
    for (B, T, D) in SHAPES:
        for thr in THRESHOLDS:
            for mt in MAX_TOKENS:
                out.append(dict(kind="chosen", shape=(B, T, D), thr=thr, mt=mt, lens=None))
    for shape, lens in LENS.items():
        for thr, mt in ((0.7, 3), (0.6, 8)):
            out.append(dict(kind="chosen", shape=shape, thr=thr, mt=mt, lens=lens))
    # thr = -1: no boundary, runs cut by the cap alone - 17 = 8 + 8 + 1 (a remainder group of one frame at the end), 16 = 8 + 8 (a group
    # of exactly max_tokens ends on the clip's last frame), 41 = 13 x 3 + 2
    out.append(dict(kind="chosen", shape=(4, 17, 260), thr=-1.0, mt=8, lens=None))
    out.append(dict(kind="chosen", shape=(4, 17, 260), thr=-1.0, mt=8, lens=(17, 16, 8, 1)))
    out.append(dict(kind="chosen", shape=(3, 41, 8), thr=-1.0, mt=3, lens=None))
    out.append(dict(kind="chosen", shape=(3, 41, 8), thr=-1.0, mt=1, lens=None))
    # thr = 1: every frame its own group, nseg == T
    out.append(dict(kind="chosen", shape=(3, 41, 8), thr=1.0, mt=3, lens=None))
    out.append(dict(kind="chosen", shape=(2, 300, 1024), thr=1.0, mt=8, lens=None))
    out.append(dict(kind="same", shape=(3, 41, 8), thr=0.9, mt=8, lens=None))
    out.append(dict(kind="same", shape=(3, 41, 8), thr=0.9, mt=3, lens=(41, 21, 30)))  # clip 1 ends on its zero frame
    out.append(dict(kind="tie", shape=(1, 2, 8), thr=1.0, mt=8, lens=None))
    for c in out:
        c["id"] = "{}-{}x{}x{}-thr{}-mt{}{}".format(c["kind"], *c["shape"], c["thr"], c["mt"], "" if c["lens"] is None else "-lens")
    return out


ALIGN_CASES = _cases()
# the aggregator kernels run on align's output for these: D in {8, 260, 1024}, every kind, with and without lens
AGG_CASES = [c for c in ALIGN_CASES if c["shape"][2] != 12 and (c["kind"] != "chosen" or c["lens"] is not None or c["thr"] in (-1.0, 1.0)
                                                                or (c["thr"], c["mt"]) in ((0.6, 8), (0.9, 3), (0.7, 1)))]


def align_input(case):
    """The frames of a case, [B, T, D] float32; behind lens[b] they are NaN (never to be read)."""
    B, T, D = case["shape"]
    if case["kind"] == "same":
        h = _same_frames()
    elif case["kind"] == "tie":
        h = _tie_frames()
    else:
        h = chosen_frames(1000 + T + D, B, T, D, pool_for(case["thr"]))
    h = h.clone()
    if case["lens"] is not None:
        for b, n in enumerate(case["lens"]):
            h[b, n:] = float("nan")
    return h


def margin(case, dtype=F64):
    """min |sim - thr| over the live frame pairs of a case (inf where it has none)."""
    h = align_input(case)
    B, T, _ = h.shape
    m = float("inf")
    for b in range(B):
        n = clip_len(case["lens"], b, T)
        if n > 1:
            m = min(m, float((cosine_sims(h[b, :n], dtype).double() - case["thr"]).abs().min()))
    return m
