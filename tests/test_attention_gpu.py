"""attention_kernel (csrc/attention.hip) in every mode its callers use and in both arithmetic forms (QA_ATT_MATH = 0: the fp32 chain,
1: split-6; (a), (b) and (d) run once per form), through the test hook qa_debug_attention_ex, against a float64 truth built from the
reference's semantics (not from the kernel's formulas).

    mode     layout (the caller's)                                          mask / bias
    self     fused QKV [B, N, 3d] (H-Codec transformers, HuBERT / XLSR)     none
    cross    Q [B, n_q, inner], interleaved K / V [B, n_keys, 2 inner]      none (BiCodec perceiver)
    cache    Q in a QKV buffer, K / V caches [B, max_len, d]                key j visible iff j <= i + (n_keys - n_q) (UniSE LM prefill,
                                                                            LLM_SFT.forward scoring; chunked at pos0 = n_keys - n_q)
    window   fused QKV, causal with `context`                               ... and (i + off) - j < context (mimi / H-Codec 1.5 stacks)
    ring     Q in a QKV buffer, K / V = the slots of a RingKVCache          slot positions from oracle.hcodec15_ref.MimiStreamState.complete
                                                                            (mimi streaming: ring_end, q_pos0, context)
    bias     fused QKV + gate [B, H, N] + relbias [H, 2R + 1]               gate * bucket-embedding(j - i), oracle.ssl_ref.relative_position_bucket
                                                                            at the UNCLAMPED distance (WavLM)

(a) fp64 parity: every head_dim x mode over lengths on the 32-key / 128-query edges (1, 2, 31, 32, 33, 127, 128, 129, 283; a last
    query block with idle waves), B in {1, 3}, H in {1, 5}, in two input regimes - unit-variance randn, and "peaked" inputs whose
    scores follow a ramp over the key index spanning 160 units (the largest visible score sits in each query's LAST visible tile, so
    the running maximum moves late and the early tiles' exponentials underflow to 0).  Each window width and ring geometry meets the
    tile edges: context 34 puts the first visible key of the wave at query 64 on key 31, the last key of a tile (the wave-uniform skip
    `wave_first_key`); ring_end below, at and far past the capacity, the cursor mid-ring, n_q = cap (the first query sees nothing);
    the WavLM clamp at R = 20 with 64 buckets (bucket(R - 1) != bucket(R), N up to 283) and the WavLM base+ geometry (R = 800, 320
    buckets, N >= 1000).
(b) the callers' own geometries at size, sampled query rows checked in fp64.
(c) memory contract, on every launch of (a), (b) and (d): the output lands in tests/util.guarded_out (ldo = d + 4, sentinel gaps and
    tail rows); everything the kernel must never read is NaN: rows before and after every input, the Q buffer's K / V columns where
    the caller's K / V live elsewhere, cache rows n_keys .. max_len, gate past B * H * n_q and guard rows around the relbias table.
    Masked keys below n_keys are NOT poisoned: the kernel reads them and multiplies them by p = 0 (so does the reference).
(d) bit-exact invariance in every mode: QA_ATT_DEBUG bits (8: no tile skip, 16: mask every tile - the slow paths against the fast),
    chunked causal queries against one launch, any query subset of a cross-attention, a batch item alone, three identical runs.
(e) every contract error of launch_attention: non-zero status, qa_last_error set, output untouched.

Error metric: e = max |o - o64| / max |o64| per case.  The bound is C_PARITY * max(e_cpu32, E_FLOOR, S_ULP * s_max), e_cpu32 the same
metric of the same formula evaluated by torch in fp32 on the host, s_max the largest visible |score| of the case.  E_FLOOR: e_cpu32 is 0
where a query sees one key (p = 1 on both sides) and small by luck elsewhere; the largest e_hip measured where e_cpu32 < E_FLOOR is 6.5e-7
(ring, one query over 37 keys, hd 96).  S_ULP: the kernel folds scale * log2(e) into Q and exponentiates in base 2, one more rounding of
every score, whose effect on p grows with |score| (2^-24 * 80 = 4.8e-6 on the peaked inputs).  Measured on MI355X over 619 cases (a, b):
per mode, e_hip (e_cpu32) ranges
    self    0 .. 2.1e-5 (0 .. 2.8e-5)     cross   0 .. 2.2e-5 (0 .. 2.3e-5)     cache   0 .. 1.6e-5 (0 .. 1.6e-5)
    window  0 .. 1.5e-5 (0 .. 2.0e-5)     ring    0 .. 1.5e-5 (0 .. 1.4e-5)     bias    0 .. 2.2e-5 (0 .. 1.6e-5)
(randn inputs alone: e_hip <= 1.9e-6, e_cpu32 <= 1.4e-6); bounds 1.0e-6 .. 1.1e-4, largest fraction used 0.65 (ring), 0.61 (bias, WavLM
base+ at N = 1031), 0.55 (cross), 0.50 (self), 0.46 (cache), 0.41 (window).  test_parity_report prints these per session (pytest -s).
Sensitivity (uncommitted builds): ring positions with `delta < 0` fail parity[ring-*] and at_caller_size[mimi_ring_*];
`wave_first_key` one key late fails parity and invariance [window-*] (context 34); the bias clamp at R - 1 fails parity[bias-*] (R = 20);
the hd = 96 output x (1 + 2^-10) fails parity[*-96]; `need_mask` without its window term fails parity / invariance[window-*] and
at_caller_size[hcodec15_bottleneck_causal].
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import functools
import zlib

import pytest
import torch
import torch.nn.functional as F

from oracle.hcodec15_ref import MimiStreamState
from oracle.ssl_ref import relative_position_bucket
from tests.util import SENTINEL_BITS, check_guarded_out, guarded_out, with_knob

pytestmark = pytest.mark.gpu

C_PARITY = 4.0
E_FLOOR = 2.5e-7
S_ULP = 2.0 ** -24  # floor per unit of the largest visible |score|: one fp32 rounding of it (module docstring)
HEAD_ROWS, TAIL_ROWS = 2, 32  # NaN rows around every input buffer: a clamped or unclamped row read past either end finds NaN
OUT_HEAD = 4                  # output offset into its guarded buffer (floats; stores are 16-byte aligned)
HDS = (32, 64, 96, 128)
MATHS = (0, 1)                # QA_ATT_MATH: the fp32 chain, split-6
REPORT = []                   # (math, mode, hd, regime, geometry, e_hip, e_cpu32, bound), printed by test_parity_report


@dataclasses.dataclass(frozen=True)
class Case:
    mode: str
    B: int
    H: int
    hd: int
    n_q: int
    n_keys: int
    pos0: int = 0        # cache: n_keys - n_q
    max_len: int = 0     # cache: rows per batch item of the K / V caches
    context: int = 0
    ring_end: int = 0
    R: int = 0
    buckets: int = 0

    @property
    def d(self):
        return self.H * self.hd

    @property
    def causal(self):
        return int(self.mode in ("cache", "window", "ring"))

    @property
    def q_pos0(self):
        return self.ring_end - self.n_q if self.mode == "ring" else 0

    def tag(self):
        f = [f"B{self.B}", f"H{self.H}", f"nq{self.n_q}", f"nk{self.n_keys}"]
        f += [f"{k}{getattr(self, k)}" for k in ("pos0", "context", "ring_end", "R") if getattr(self, k)]
        return "-".join(f)


# ------------------------------------------------------------------------------------------------ the truth
def reference_mask(c: Case, qi: torch.Tensor) -> torch.Tensor:
    """[len(qi), n_keys] bool: key j visible to query qi, by the reference's rules (module docstring)."""
    kj = torch.arange(c.n_keys)
    if c.mode == "ring":
        # RingKVCache.complete() of a chunk of n_q tokens written at offset ring_end - n_q: its slot positions (-1 = never written;
        # the slot at the write cursor reports position `end` and is invisible); mimi_transformer's mask over them
        st = MimiStreamState(1, 1, 1, 1, c.n_keys)
        st.offset = c.q_pos0
        z = torch.zeros(1, 1, c.n_q, 1)
        pos = st.complete(0, z, z)[2]
        delta = (c.q_pos0 + qi).view(-1, 1) - pos.view(1, -1)
        return (pos.view(1, -1) >= 0) & (delta >= 0) & (delta < c.context)
    m = torch.ones(len(qi), c.n_keys, dtype=torch.bool)
    if c.causal:
        last = (qi + c.n_keys - c.n_q).view(-1, 1)
        m &= kj.view(1, -1) <= last
        if c.context:
            m &= last - kj.view(1, -1) < c.context
    return m


def scores(c: Case, x: dict, dtype, qi: torch.Tensor) -> torch.Tensor:
    """scale Q K^T [+ gate * bias] with the hidden keys at -inf, in `dtype` -> [B, H, len(qi), n_keys]."""
    q = x["q"][:, qi].transpose(1, 2).to(dtype)
    k = x["k"].transpose(1, 2).to(dtype)
    s = (q * c.hd ** -0.5) @ k.transpose(-1, -2)
    if c.mode == "bias":
        rel = torch.arange(c.n_keys).view(1, -1) - qi.view(-1, 1)  # memory - context position, unclamped
        bias = F.embedding(relative_position_bucket(rel, c.buckets, c.R), x["emb"]).permute(2, 0, 1).to(dtype)
        s = s + x["gate"][:, :, qi, None].to(dtype) * bias[None]
    return s.masked_fill(~reference_mask(c, qi), float("-inf"))


def attention_truth(c: Case, x: dict, dtype, rows=None) -> torch.Tensor:
    """softmax(scale Q K^T [+ gate * bias] + mask) V in `dtype` on the host; rows: the query rows to evaluate (default all).
    A query with no visible key gives 0.  -> [B, len(rows), H, hd]"""
    s = scores(c, x, dtype, torch.arange(c.n_q) if rows is None else torch.as_tensor(rows))
    m = s.amax(-1, keepdim=True)
    p = torch.exp(s - torch.where(torch.isfinite(m), m, torch.zeros_like(m)))
    l = p.sum(-1, keepdim=True)
    return ((p @ x["v"].transpose(1, 2).to(dtype)) / torch.where(l > 0, l, torch.ones_like(l))).transpose(1, 2)


def make_inputs(c: Case, regime: str, seed: int) -> dict:
    """Logical fp32 host tensors q [B, n_q, H, hd], k / v [B, n_keys, H, hd] (+ gate [B, H, n_q], emb [buckets, H])."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(c.B, c.n_q, c.H, c.hd, generator=g)
    k = torch.randn(c.B, c.n_keys, c.H, c.hd, generator=g)
    v = torch.randn(c.B, c.n_keys, c.H, c.hd, generator=g)
    if regime == "peaked":
        # score(i, j) ~ ramp[j] + O(1): q = sqrt(hd) u + noise, k_j = ramp[j] u + noise, u a unit vector per head; the ramp spans
        # 160 units over the keys (exp(-160) is 0 in fp32), so every query's largest visible score is at its last visible key
        u = F.normalize(torch.randn(c.H, c.hd, generator=g), dim=-1)
        ramp = 160.0 * (torch.arange(c.n_keys) / max(c.n_keys - 1, 1) - 0.5)
        q = c.hd ** 0.5 * u + 0.3 * q
        k = ramp.view(1, -1, 1, 1) * u + 0.5 * k
    x = dict(q=q.contiguous(), k=k.contiguous(), v=v)
    if c.mode == "bias":
        # WavLM's gate is a * (b * const - 1) + 2 with a, b sigmoids: between 1 and 3 for const near 1
        x["gate"] = 1.0 + 2.0 * torch.rand(c.B, c.H, c.n_q, generator=g)
        x["emb"] = torch.randn(c.buckets, c.H, generator=g)
    return x


def relbias_table(c: Case, emb: torch.Tensor) -> torch.Tensor:
    """The table the library hands the kernel (ssl.cpp): the same bucket function at distances -R .. R -> [H, 2R + 1]."""
    r = torch.arange(-c.R, c.R + 1)
    return emb[relative_position_bucket(r, c.buckets, c.R)].t().contiguous()


# ------------------------------------------------------------------------------------------------ the kernel
def _hook(lib):
    fn = lib.qa_debug_attention_ex
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_int,
                   C.c_longlong, C.c_int, C.c_int, C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                   C.c_void_p]
    return fn


def _poisoned(rows, ld, device):
    """(buffer, view [rows, ld]) with HEAD_ROWS / TAIL_ROWS NaN rows around the view."""
    buf = torch.full((HEAD_ROWS + rows + TAIL_ROWS, ld), float("nan"), device=device)
    return buf, buf[HEAD_ROWS:HEAD_ROWS + rows]


@dataclasses.dataclass
class Packed:
    """The caller's layout of one case on the device: pointers (bytes), strides (floats) and the buffers that own them."""
    q: int
    ldq: int
    k: int
    v: int
    ldkv: int
    kv_bstride: int
    gate: int = 0
    relbias: int = 0
    qrows: torch.Tensor = None  # [B, n_q, ldq] view of the Q rows (query splits copy from it)
    keep: list = dataclasses.field(default_factory=list)


def pack(c: Case, x: dict, device) -> Packed:
    B, d = c.B, c.d
    Q = x["q"].reshape(B * c.n_q, d).to(device)
    K, V = (x[n].reshape(B, c.n_keys, d).to(device) for n in ("k", "v"))
    if c.mode in ("self", "window", "bias"):  # fused QKV, n_q == n_keys
        buf, rows = _poisoned(B * c.n_q, 3 * d, device)
        rows[:, :d] = Q
        rows.view(B, c.n_q, 3 * d)[:, :, d:2 * d] = K
        rows.view(B, c.n_q, 3 * d)[:, :, 2 * d:] = V
        p = Packed(rows.data_ptr(), 3 * d, rows.data_ptr() + 4 * d, rows.data_ptr() + 8 * d, 3 * d, c.n_keys * 3 * d,
                   qrows=rows.view(B, c.n_q, 3 * d), keep=[buf])
    elif c.mode == "cross":  # Q [B, n_q, inner]; K / V interleaved per row [B, n_keys, 2 inner]
        qb, qr = _poisoned(B * c.n_q, d, device)
        qr.copy_(Q)
        kvb, kvr = _poisoned(B * c.n_keys, 2 * d, device)
        kvr.view(B, c.n_keys, 2 * d)[:, :, :d] = K
        kvr.view(B, c.n_keys, 2 * d)[:, :, d:] = V
        p = Packed(qr.data_ptr(), d, kvr.data_ptr(), kvr.data_ptr() + 4 * d, 2 * d, c.n_keys * 2 * d, qrows=qr.view(B, c.n_q, d),
                   keep=[qb, kvb])
    else:  # cache / ring: Q in a QKV buffer whose K / V columns are never read; K / V caches [B, max_len, d] (ring: max_len = cap)
        max_len = c.max_len if c.mode == "cache" else c.n_keys
        qb, qr = _poisoned(B * c.n_q, 3 * d, device)
        qr[:, :d] = Q
        kb, kr = _poisoned(B * max_len, d, device)
        vb, vr = _poisoned(B * max_len, d, device)
        kr.view(B, max_len, d)[:, :c.n_keys] = K
        vr.view(B, max_len, d)[:, :c.n_keys] = V
        p = Packed(qr.data_ptr(), 3 * d, kr.data_ptr(), vr.data_ptr(), d, max_len * d, qrows=qr.view(B, c.n_q, 3 * d),
                   keep=[qb, kb, vb])
    if c.mode == "bias":
        gb = torch.full((B * c.H * c.n_q + 64,), float("nan"), device=device)  # gate past B * H * n_q: NaN
        gb[:B * c.H * c.n_q] = x["gate"].reshape(-1).to(device)
        rb, rr = _poisoned(c.H, 2 * c.R + 1, device)  # NaN rows before and after the [H, 2R + 1] table
        rr.copy_(relbias_table(c, x["emb"]).to(device))
        p.gate, p.relbias = gb.data_ptr(), rr.data_ptr()
        p.keep += [gb, rb]
    return p


def launch(lib, c: Case, p: Packed, *, q=None, n_q=None, n_keys=None, B=None, boff=0, expect_ok=True):
    """One launch of the hook into a guarded output; overrides for query splits (q pointer / n_q / n_keys) and a batch item alone
    (B = 1, boff = the item).  -> output [B, n_q, H, hd] on the device."""
    n_q = c.n_q if n_q is None else n_q
    n_keys = c.n_keys if n_keys is None else n_keys
    nb = c.B if B is None else B
    qp = (p.q if q is None else q) + 4 * boff * c.n_q * p.ldq
    kvo = 4 * boff * p.kv_bstride
    gate = p.gate + 4 * boff * c.H * c.n_q if p.gate else None
    ldo = c.d + 4
    buf, out = guarded_out(nb * n_q, c.d, ldo, OUT_HEAD, torch.device("cuda"))
    st = _hook(lib)(qp, p.ldq, p.k + kvo, p.v + kvo, p.ldkv, out.data_ptr(), ldo, nb, n_q, n_keys, p.kv_bstride, c.H, c.hd,
                    c.hd ** -0.5, c.causal, gate, p.relbias or None, c.R, c.context, c.q_pos0, c.ring_end,
                    torch.cuda.current_stream().cuda_stream)
    assert st == 0, lib.qa_last_error()
    torch.cuda.synchronize()
    check_guarded_out(buf, out, OUT_HEAD)
    return out.reshape(nb, n_q, c.H, c.hd).clone()


def _seed(c: Case, regime: str) -> int:
    return zlib.crc32(f"{c}{regime}".encode())


def _truth(c: Case, regime: str, rows, x):
    """-> (t64, e_cpu32, s_max, blind) of inputs x: the fp64 truth, the host's own fp32 error, the largest visible |score| and the
    queries with no visible key."""
    t64 = attention_truth(c, x, torch.float64, rows)
    t32 = attention_truth(c, x, torch.float32, rows)
    e_cpu = float((t32.double() - t64).abs().max()) / max(float(t64.abs().max()), 1e-300)
    qi = torch.arange(c.n_q) if rows is None else torch.as_tensor(rows)
    s64 = scores(c, x, torch.float64, qi)
    s_max = float(s64[torch.isfinite(s64)].abs().max()) if torch.isfinite(s64).any() else 0.0
    return t64, e_cpu, s_max, ~reference_mask(c, qi).any(-1)


@functools.lru_cache(maxsize=64)  # the two forms of one (mode, hd) run back to back and share the truth of the seeded inputs
def _seeded_truth(c: Case, regime: str, rows):
    return _truth(c, regime, rows, make_inputs(c, regime, _seed(c, regime)))


def check_parity(lib, c: Case, regime: str, rows=None, x=None):
    """The form QA_ATT_MATH selects at the time of the call -> (e_hip, e_cpu32, bound, message or None)."""
    from unified_audio_amd import _lib

    math = int(_lib.get_knob("QA_ATT_MATH"))
    t64, e_cpu, s_max, blind = _seeded_truth(c, regime, rows and tuple(rows)) if x is None else _truth(c, regime, rows, x)
    x = make_inputs(c, regime, _seed(c, regime)) if x is None else x
    out = launch(lib, c, pack(c, x, torch.device("cuda"))).cpu()
    if rows is not None:
        out = out[:, torch.as_tensor(rows)]
    e_hip = float((out.double() - t64).abs().max()) / max(float(t64.abs().max()), 1e-300)
    bound = C_PARITY * max(e_cpu, E_FLOOR, S_ULP * s_max)
    msg = None
    if blind.any() and not torch.equal(out[:, blind], torch.zeros_like(out[:, blind])):
        msg = f"{c.tag()} {regime}: a query with no visible key is not exactly 0"
    elif not e_hip <= bound:
        msg = f"{c.tag()} {regime}: e_hip {e_hip:.3e} > bound {bound:.3e} (e_cpu32 {e_cpu:.3e})"
    REPORT.append((math, c.mode, c.hd, regime, c.tag(), e_hip, e_cpu, bound))
    print(f"ATTN math{math} {c.mode} hd{c.hd} {regime} {c.tag()} e_hip {e_hip:.3e} e_cpu32 {e_cpu:.3e} bound {bound:.3e} frac {e_hip / bound:.3f}")
    return e_hip, e_cpu, bound, msg


# ------------------------------------------------------------------------------------------------ (a) the parity matrix
LENS = (1, 2, 31, 32, 33, 127, 128, 129, 283)
BH = ((1, 1), (3, 5), (1, 5), (3, 1))


def matrix_cases(mode: str, hd: int):
    bh = lambda i: dict(zip(("B", "H"), BH[i % len(BH)]))  # noqa: E731
    out = []
    if mode == "self":
        out = [Case(mode, hd=hd, n_q=n, n_keys=n, **bh(i)) for i, n in enumerate(LENS)]
    elif mode == "cross":
        pairs = [(1, 283), (2, 33), (31, 129), (32, 1), (33, 2), (127, 32), (128, 31), (129, 128), (283, 127), (129, 333)]
        out = [Case(mode, hd=hd, n_q=a, n_keys=b, **bh(i)) for i, (a, b) in enumerate(pairs)]
    elif mode == "cache":  # batch stride max_len > n_keys: the rows between are NaN
        pairs = [(1, 0), (2, 500), (31, 32), (32, 31), (33, 1), (127, 33), (128, 0), (129, 500), (283, 31), (1, 32), (129, 1)]
        out = [Case(mode, hd=hd, n_q=n, n_keys=n + p0, pos0=p0, max_len=n + p0 + 37, **bh(i)) for i, (n, p0) in enumerate(pairs)]
    elif mode == "window":
        pairs = [(1, 1), (2, 16), (31, 31), (32, 32), (33, 33), (127, 34), (128, 250), (129, 16), (283, 34), (283, 1), (283, 33),
                 (129, 250), (283, 32), (283, 31)]
        out = [Case(mode, hd=hd, n_q=n, n_keys=n, context=ctx, **bh(i)) for i, (n, ctx) in enumerate(pairs)]
    elif mode == "ring":  # (cap, n_q, ring_end, context); context = cap as in the caller unless given
        rings = [(32, 1, 1, 32), (32, 7, 20, 32), (32, 32, 32, 32), (32, 7, 32 * 9 + 13, 32), (32, 1, 32 * 5, 32), (32, 32, 32 * 3 + 17, 32),
                 (37, 1, 36, 37), (37, 7, 37, 37), (37, 37, 37 * 4 + 20, 37), (37, 7, 1000, 37), (37, 37, 37, 37),
                 (129, 129, 129 * 2 + 64, 129), (129, 2, 131, 129),
                 (250, 1, 1, 250), (250, 7, 250, 250), (250, 250, 250 * 3 + 111, 250), (250, 1, 999, 250), (250, 7, 120, 250),
                 (250, 250, 250, 250), (250, 7, 600, 100), (250, 33, 1283, 31)]
        out = [Case(mode, hd=hd, n_q=n, n_keys=cap, ring_end=end, context=ctx, **bh(i)) for i, (cap, n, end, ctx) in enumerate(rings)]
    elif mode == "bias":  # R = 20 with 64 buckets: bucket(19) = 28 != bucket(20) = 31, so the clamp at R is visible
        out = [Case(mode, hd=hd, n_q=n, n_keys=n, R=20, buckets=64, **bh(i)) for i, n in enumerate(LENS)]
        out += [Case(mode, B=1, H=1, hd=hd, n_q=n, n_keys=n, R=800, buckets=320) for n in (1000, 1031)]  # WavLM base+
    return out


MODES = ("self", "cross", "cache", "window", "ring", "bias")


def per_form(cases):
    """pytest params of every case (a tuple of arguments) in both forms, the two side by side (they share _seeded_truth).  The split-6
    case keeps the id the case had when this file ran the default form alone; the fp32 case adds "-fp32"."""
    return [pytest.param(*c, math, id="-".join(map(str, c)) + ("" if math else "-fp32")) for c in cases for math in MATHS]



@pytest.mark.parametrize("mode,hd,math", per_form([(mode, hd) for mode in MODES for hd in HDS]))
def test_attention_fp64_parity_matrix(qa_lib, gpu_device, mode, hd, math):
    bad = []
    with with_knob("QA_ATT_MATH", math):
        for c in matrix_cases(mode, hd):
            for regime in ("randn", "peaked"):
                msg = check_parity(qa_lib, c, regime)[3]
                if msg:
                    bad.append(msg)
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------ (b) at size
AT_SIZE = {
    "hcodec20_30s": Case("self", B=16, H=24, hd=64, n_q=1500, n_keys=1500),               # 30 s at 50 frames/s, d 1536
    "hcodec15_bottleneck": Case("self", B=32, H=8, hd=128, n_q=500, n_keys=500),          # d 1024, 8 heads, 10 s at 50 frames/s
    "hcodec15_bottleneck_causal": Case("window", B=32, H=8, hd=128, n_q=500, n_keys=500, context=16),  # bt_causal with context 16
    "xlsr53_6s": Case("self", B=16, H=16, hd=64, n_q=299, n_keys=299),                    # 6 s at 16 kHz: 299 frames, d 1024
    "wavlm_base_plus_6s": Case("bias", B=16, H=12, hd=64, n_q=299, n_keys=299, R=800, buckets=320),
    "lm_prompt": Case("cache", B=16, H=8, hd=64, n_q=252, n_keys=252, max_len=576),      # prefill of the 252-position prompt
    "lm_score_full": Case("cache", B=16, H=8, hd=64, n_q=535, n_keys=535, max_len=576),  # teacher-forced 252 + 283
    "lm_chunk": Case("cache", B=16, H=8, hd=64, n_q=283, n_keys=535, pos0=252, max_len=576),
    "bicodec_perceiver": Case("cross", B=16, H=8, hd=64, n_q=32, n_keys=333),            # 32 latents over 32 + 301 frames (6 s)
    "mimi_ring_step": Case("ring", B=16, H=8, hd=64, n_q=1, n_keys=250, ring_end=1001, context=250),
    "mimi_ring_chunk": Case("ring", B=16, H=8, hd=64, n_q=7, n_keys=250, ring_end=2046, context=250),
}


@pytest.mark.parametrize("name,math", per_form([(name,) for name in sorted(AT_SIZE)]))
def test_attention_at_caller_size(qa_lib, gpu_device, name, math):
    c = AT_SIZE[name]
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    edges = {0, 1, 31, 32, 33, 127, 128, 129, c.n_q - 1}
    rows = sorted({r for r in edges if r < c.n_q} | set(torch.randint(0, c.n_q, (24,), generator=g).tolist()))
    with with_knob("QA_ATT_MATH", math):
        msg = check_parity(qa_lib, c, "randn", rows=rows)[3]
    assert msg is None, msg


# ------------------------------------------------------------------------------------------------ (d) invariance
INVARIANCE = {
    "self": Case("self", B=3, H=5, hd=0, n_q=283, n_keys=283),
    "cross": Case("cross", B=3, H=5, hd=0, n_q=283, n_keys=129),
    "cache": Case("cache", B=3, H=5, hd=0, n_q=283, n_keys=316, pos0=33, max_len=353),
    "window": Case("window", B=3, H=5, hd=0, n_q=283, n_keys=283, context=34),
    "ring": Case("ring", B=3, H=5, hd=0, n_q=37, n_keys=250, ring_end=1111, context=250),
    "bias": Case("bias", B=3, H=5, hd=0, n_q=283, n_keys=283, R=20, buckets=64),
}
SPLITS = [(0, 1), (1, 31), (31, 64), (64, 129), (129, 130), (130, 283), (250, 283), (0, 283)]


@pytest.mark.parametrize("mode,hd,math", per_form([(mode, hd) for mode in MODES for hd in HDS]))
def test_attention_bit_exact_invariance(qa_lib, gpu_device, mode, hd, math):
    c = dataclasses.replace(INVARIANCE[mode], hd=hd)
    p = pack(c, make_inputs(c, "randn", _seed(c, "inv")), gpu_device)
    with with_knob("QA_ATT_MATH", math):
        ref = launch(qa_lib, c, p)
        for _ in range(2):  # three identical runs
            assert torch.equal(launch(qa_lib, c, p), ref), "run-to-run"
        for dbg in (1, 2, 4, 8, 16, 31):
            with with_knob("QA_ATT_DEBUG", dbg):
                assert torch.equal(launch(qa_lib, c, p), ref), f"QA_ATT_DEBUG={dbg}"
        for b in range(c.B):  # a batch item alone
            assert torch.equal(launch(qa_lib, c, p, B=1, boff=b)[0], ref[b]), f"batch item {b} alone"
        if mode in ("cache", "window", "cross"):
            subsets = [torch.arange(a, b) for a, b in SPLITS]
            if mode == "cross":  # any subset of the queries, in any order
                subsets.append(torch.randperm(c.n_q, generator=torch.Generator().manual_seed(hd))[:150])
            off = c.n_keys - c.n_q
            for idx in subsets:
                qbuf, qrows = _poisoned(c.B * len(idx), p.ldq, gpu_device)
                qrows.view(c.B, len(idx), p.ldq).copy_(p.qrows[:, idx.to(gpu_device)])
                # causal: queries [a, b) over keys [0, b + off) - a chunk of a chunked prefill; cross: every key
                nk = c.n_keys if mode == "cross" else int(idx[-1]) + 1 + off
                got = launch(qa_lib, c, p, q=qrows.data_ptr(), n_q=len(idx), n_keys=nk)
                assert torch.equal(got, ref[:, idx.to(gpu_device)]), f"queries {int(idx[0])} .. {int(idx[-1])} ({len(idx)})"


# ------------------------------------------------------------------------------------------------ (e) contract errors
ERRORS = {  # name -> (Case overrides, launch overrides, expected fragment of qa_last_error)
    "n_q_0": (dict(mode="self"), dict(n_q=0), "n_q=0"),
    "n_keys_0": (dict(mode="cross"), dict(n_keys=0), "n_keys=0"),
    "causal_fewer_keys": (dict(mode="cache"), dict(n_keys=63), "n_keys=63"),
    "context_negative": (dict(mode="window"), dict(context=-1), "context window"),
    "context_not_causal": (dict(mode="self"), dict(context=16), "context window"),
    "ring_not_causal": (dict(mode="self"), dict(context=16, ring_end=70), "context window"),
    "ring_without_context": (dict(mode="ring"), dict(context=0), "context window"),
    "ring_with_gate": (dict(mode="ring"), dict(gate=True), "context window"),
    "ldq_odd": (dict(mode="self"), dict(ldq=3 * 128 + 2), "multiples of 4"),
    "ldkv_odd": (dict(mode="self"), dict(ldkv=3 * 128 + 1), "multiples of 4"),
    "ldo_odd": (dict(mode="self"), dict(ldo=128 + 2), "multiples of 4"),
    "gate_without_relbias": (dict(mode="bias"), dict(relbias=False), "gate and relbias"),
    "relbias_without_gate": (dict(mode="bias"), dict(gate=False), "gate and relbias"),
    "bias_negative_R": (dict(mode="bias"), dict(R=-1), "gate and relbias"),
    "bias_causal": (dict(mode="bias"), dict(causal=1), "gate and relbias"),
    "bias_cross": (dict(mode="bias"), dict(n_keys=63), "gate and relbias"),
    "hd_48": (dict(mode="self"), dict(hd=48), "head_dim=48"),
    "hd_256": (dict(mode="self"), dict(hd=256), "head_dim=256"),
}


@pytest.mark.parametrize("name", sorted(ERRORS))
def test_attention_contract_errors(qa_lib, gpu_device, name):
    case_kw, kw, fragment = ERRORS[name]
    c = Case(B=2, H=2, hd=64, n_q=64, n_keys=64, **case_kw)
    c = {"cache": dataclasses.replace(c, max_len=96), "ring": dataclasses.replace(c, n_q=7, n_keys=32, ring_end=70, context=32),
         "window": dataclasses.replace(c, context=16), "bias": dataclasses.replace(c, R=20, buckets=64),
         "cross": dataclasses.replace(c, n_keys=33)}.get(c.mode, c)
    p = pack(c, make_inputs(c, "randn", 1), gpu_device)  # the valid launch these arguments were changed from
    spare = torch.zeros(4096, device=gpu_device)           # gate / relbias where the case adds one
    gate = p.gate or (spare.data_ptr() if kw.get("gate") else None)
    relbias = p.relbias or None
    if kw.get("gate") is False:
        gate = None
    if kw.get("relbias") is False:
        relbias = None
    fn = _hook(qa_lib)
    args = dict(q=p.q, ldq=p.ldq, k=p.k, v=p.v, ldkv=p.ldkv, ldo=c.d + 4, B=c.B, n_q=c.n_q, n_keys=c.n_keys, kv_bstride=p.kv_bstride,
                H=c.H, hd=c.hd, scale=c.hd ** -0.5, causal=c.causal, gate=gate, relbias=relbias, R=c.R, context=c.context,
                q_pos0=c.q_pos0, ring_end=c.ring_end)
    buf = torch.empty(OUT_HEAD + (c.B * c.n_q + 256) * (c.d + 8), device=gpu_device)
    buf.view(torch.int32).fill_(SENTINEL_BITS)

    def call(**over):
        a = {**args, **over}
        return fn(a["q"], a["ldq"], a["k"], a["v"], a["ldkv"], buf.data_ptr() + 4 * OUT_HEAD, a["ldo"], a["B"], a["n_q"], a["n_keys"],
                  a["kv_bstride"], a["H"], a["hd"], a["scale"], a["causal"], a["gate"], a["relbias"], a["R"], a["context"], a["q_pos0"],
                  a["ring_end"], torch.cuda.current_stream().cuda_stream)

    assert call(n_q=-7) != 0  # a different message first: the one checked below is this call's own
    assert "n_q=-7" in qa_lib.qa_last_error().decode()
    st = call(**{k: v for k, v in kw.items() if k not in ("gate", "relbias")})
    torch.cuda.synchronize()
    err = qa_lib.qa_last_error().decode()
    assert st != 0, f"{name}: accepted"
    assert fragment in err, f"{name}: qa_last_error {err!r}"
    assert bool((buf.view(torch.int32) == SENTINEL_BITS).all()), f"{name}: the output buffer was written"


# ------------------------------------------------------------------------------------------------ report
def test_parity_report():
    """Per form and mode: the range of e_hip and e_cpu32 and the largest fraction of the bound used by the cases of this session."""
    by = {}
    for math, mode, hd, regime, tag, e_hip, e_cpu, bound in REPORT:
        by.setdefault((math, mode), []).append((e_hip, e_cpu, bound))
    for (math, mode), v in sorted(by.items()):
        eh, ec, bd = zip(*v)
        print(f"ATTN-SUMMARY math{math} {mode}: {len(v)} cases, e_hip {min(eh):.2e} .. {max(eh):.2e}, e_cpu32 {min(ec):.2e} .. {max(ec):.2e}, "
              f"bound {min(bd):.2e} .. {max(bd):.2e}, largest fraction {max(a / b for a, _, b in v):.3f}")
