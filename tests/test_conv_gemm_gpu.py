"""The implicit-GEMM convolution (conv_gemm_kernel through qa_conv1d_cl) on every launch variant, against a float64 truth.

(a) fp64 parity of every legal (tile, path) instantiation, forced with knobs: tiles QA_GEMM_CFG 0 .. 5 x {table BK 32, table BK 16,
    LINEAR BK 32, LINEAR BK 16, ELU prologue, C_in % 32 != 0}, each over geometries with ragged M / N, the scalar epilogue (N % 4 != 0,
    misaligned y, odd ldr), ksize 9 / 16 (> TAP_WIN: the tap table is rebuilt), reflect padding longer than the input, in_rep 2 / 3,
    an input slice of a wider row (the SSL positional conv: ldx 768, k 128), strided residual / gate and M = 1.  The profiler's
    per-configuration launch counts confirm the tile that ran; every output is written into a guarded buffer (tests/util.guarded_out).
(b) bit-exact invariance of the same problems over every tile, BK 16 / 32, QA_GEMM_LINEAR, QA_GEMM_XCD and QA_GEMM_PANEL: the cost
    model picks the tile and the BK from M, i.e. from the batch, so "a clip's result does not depend on its batch" needs them all
    to give the same bits.
(c) the headline's own layers (profiles/r05_hcodec15_gemm_shapes_serial.md, H-Codec 1.5, 32 clips x 10 s) at full size with the cost
    model's choices, checked in fp64 on a seeded sample of rows: the rows around every clip boundary and the last row tile, and 256 more.
(d) batch-split invariance at those layers: the last clip alone and a sub-batch that the cost model gives another tile and / or the
    other side of the 384-tile BK 16 threshold reproduce the full batch's rows bit for bit.

Error metric (tests/util.conv_ref): e = max |y - y64| / (|g| |gamma| (sum_k |a_k w_k| + |b|) + |r|) over the output, the standard
scale of a dot product's rounding error (ELU adds exp(v): the library evaluates it as exp(v) - 1); the HIP bound is
C_PARITY * max(e_cpu32, E_FLOOR) with e_cpu32 the same metric of the plain fp32 CPU evaluation.  Measured on MI355X over the 302
parity checks: e_hip 6.1e-8 .. 3.5e-7, e_cpu32 1.7e-8 .. 2.7e-7.  Per path (every tile of a case gives the same bits, hence the same
e): table / LINEAR, BK 32 / 16: 7.5e-8 .. 2.8e-7 (e_cpu32 2.6e-8 .. 2.7e-7); ELU prologue 6.1e-8 .. 2.0e-7 (1.7e-8 .. 2.3e-7);
C_in 48: 9.1e-8 .. 2.8e-7 (2.8e-8 .. 2.7e-7); (c) at size 1.3e-7 .. 3.5e-7 (3.8e-8 .. 1.5e-7).  The kernel sums K in one fp32
chain per element, the CPU in blocks: at K <= 512 the two are on a par, at K = 8192 (ssl_pos) the kernel is 10x further from the
truth (2.8e-7 vs 2.8e-8) - hence a floor, not a ratio alone.  C_PARITY 4 and E_FLOOR 1.5e-7 give bounds of 6.0e-7 .. 1.1e-6, of
which at most 0.58 was used.  Sensitivity (uncommitted builds): the last row tile's accumulators of the table-form BK 16 instance
scaled by 1 + 2^-10 give e = 7.1e-5 .. 7.4e-4 and fail every parity case of that instance; the 128 x 32 tile without its last
K chunk gives 5.5e-3 .. 5.2e-1 and fails parity and invariance.
"""
import ctypes as C
import functools
import zlib

import pytest
import torch

from tests.util import conv1d_cl, conv_ref, scaled_err, strided_rows

pytestmark = pytest.mark.gpu

C_PARITY = 4.0
E_FLOOR = 1.5e-7

TILES = {0: (128, 32), 1: (128, 64), 2: (128, 128), 3: (64, 128), 4: (64, 64), 5: (256, 128)}  # QA_GEMM_CFG -> (BM, BN)
GEMM_KNOBS = ("QA_GEMM_CFG", "QA_GEMM_256", "QA_GEMM_BK16", "QA_GEMM_BK16_MIN_TILES", "QA_GEMM_LINEAR", "QA_GEMM_XCD", "QA_GEMM_PANEL")

# kernel-level geometries (B, T, C_in, N, ksize, ...); C_in is replaced by 48 on the `cin48` path
GEOS = {
    "ragged": dict(B=2, T=550, Cin=64, N=200, k=1, act=2),                       # M 1100, N 200: ragged against every tile
    "scalar_epi": dict(B=1, T=333, Cin=96, N=70, k=1, act=3, gate=True, res=True,  # N % 4 = 2, y 4 bytes off, odd ldr: scalar epilogue
                       ldy=75, y_off=1, ldr=73),
    "strided_res_gate": dict(B=2, T=150, Cin=64, N=96, k=1, gamma=True, res=True, gate=True, post=1, ldy=100, ldr=108, ldg=200),
    "slice_k1": dict(B=3, T=70, Cin=64, N=100, k=1, ldx=768, x_off=192),
    "m1": dict(B=1, T=1, Cin=64, N=40, k=1),
    "k9": dict(B=3, T=97, Cin=32, N=136, k=9, stride=4, mode=1, res=True),     # two tap-table windows
    "k16": dict(B=2, T=330, Cin=64, N=160, k=16, stride=8, mode=1, gamma=True),
    "reflect_short": dict(B=2, T=3, Cin=32, N=96, k=16, stride=8, mode=1),      # input shorter than the reflect pad
    "in_rep2": dict(B=2, T=50, Cin=64, N=96, k=3, pad=(1, 1), in_rep=2),
    "in_rep3": dict(B=1, T=41, Cin=32, N=130, k=4, pad=(2, 1), in_rep=3, act=1),
    "ssl_pos": dict(B=2, T=200, Cin=64, N=48, k=128, pad=(64, 64), ldx=768, x_off=-1),  # x_off -1: the last channel group of the row
}

PATHS = {  # name -> (knobs, overrides of the geometry)
    "table_bk32": ({"QA_GEMM_LINEAR": 0, "QA_GEMM_BK16": 0}, {}),
    "table_bk16": ({"QA_GEMM_LINEAR": 0, "QA_GEMM_BK16_MIN_TILES": 0}, {}),
    "linear_bk32": ({"QA_GEMM_LINEAR": 1, "QA_GEMM_BK16": 0}, {}),
    "linear_bk16": ({"QA_GEMM_LINEAR": 1, "QA_GEMM_BK16_MIN_TILES": 0}, {}),
    "elu": ({}, {"prologue": 1}),
    "cin48": ({}, {"Cin": 48}),
}


def _is_linear(c):
    return c["k"] == 1 and c.get("stride", 1) == 1 and c.get("mode", 0) == 0 and c.get("pad", (0, 0)) == (0, 0) and \
        c.get("in_rep", 1) <= 1 and not c.get("prologue")


def _legal(tile, path, c):
    if path.startswith("linear") and not _is_linear(c):
        return False
    if tile == 0:
        return path not in ("table_bk16", "linear_bk16")  # 128 x 32 has BK 32 only
    if tile == 5:
        return path in ("linear_bk16", "table_bk32", "elu", "cin48")  # BK 16 always; the others fall back to 128 x 128
    return True


def _launched(tile, path, c):
    """(configuration, BK) that launch_conv_gemm / launch_cfg take for a forced tile."""
    lin = _is_linear(c) and path not in ("table_bk32", "table_bk16")
    cfg = tile
    if tile == 0 and c["Cin"] % 32:
        cfg = 1
    if tile == 5 and not lin:
        cfg = 2
    if cfg == 5 or (TILES[cfg][1] >= 64 and not c.get("prologue") and (path.endswith("bk16") or c["Cin"] % 32)):
        return cfg, 16
    return cfg, 32  # the small problems here stay below the 384-tile BK 16 threshold on the default-knob paths


PARITY = [(t, p, g) for t in TILES for p in PATHS for g in GEOS if _legal(t, p, {**GEOS[g], **PATHS[p][1]})]


def _geometry(c):
    """Fill in pad / pad_mode / T_out (reflect: the SConv1d geometry of the reference, extra right padding included)."""
    c = dict(c)
    k, s, T = c["k"], c.get("stride", 1), c["T"]
    if c.get("mode") == 1:
        pt = k - s
        c["T_out"] = -(-T // s)
        c["pad"] = (pt - pt // 2, pt // 2 + c["T_out"] * s - T)
        c["pad_mode"] = 1
    else:
        c.setdefault("pad", (0, 0))
        c["pad_mode"] = 0
        c["T_out"] = (T * c.get("in_rep", 1) + sum(c["pad"]) - k) // s + 1
    return c


class Problem:
    """Seeded operands of one case on the host and on the device, and its float64 / float32 references."""

    def __init__(self, c, dev, seed, rows=None):
        self.c = c = _geometry(c)
        g = torch.Generator().manual_seed(seed)
        B, T, Cin, N, k, To = c["B"], c["T"], c["Cin"], c["N"], c["k"], c["T_out"]
        self.x = torch.randn(B, T, Cin, generator=g)
        self.w = torch.randn(N, k, Cin, generator=g) / (k * Cin) ** 0.5
        self.bias = torch.randn(N, generator=g)
        self.gamma = torch.rand(N, generator=g) + 0.5 if c.get("gamma") else None
        self.res = torch.randn(B, To, N, generator=g) if c.get("res") else None
        self.gate = torch.randn(B, To, N, generator=g) if c.get("gate") else None
        if rows is None:  # kernel-level cases: x lies inside other numbers (strided_rows), so a read past a frame is wrong, not out of bounds
            off = c.get("x_off", 0) if c.get("x_off", 0) >= 0 else c["ldx"] - Cin
            self.xd = strided_rows(self.x.to(dev), c.get("ldx", Cin), off, generator=g)
        else:
            self.xd = self.x.to(dev)
        self.wd, self.bd = self.w.to(dev), self.bias.to(dev)
        self.gd = self.gamma.to(dev) if self.gamma is not None else None
        self.rd = strided_rows(self.res.to(dev), c.get("ldr", N), generator=g) if self.res is not None else None
        self.gtd = strided_rows(self.gate.to(dev), c.get("ldg", N), generator=g) if self.gate is not None else None
        self.rows = rows

    def references(self):
        kw = dict(gamma=self.gamma, residual=self.res, gate=self.gate, rows=self.rows)
        y64, scale = conv_ref(self.x, self.w, self.bias, self.c, torch.float64, **kw)
        y32, _ = conv_ref(self.x, self.w, self.bias, self.c, torch.float32, **kw)
        return y64, scale, scaled_err(y32, y64, scale)

    def run(self, lib, sub=None):
        """HIP output [B * T_out, N] (device); sub = a slice of clips."""
        c = self.c
        sl = sub or slice(None)
        pick = (lambda t: None if t is None else t[sl])  # noqa: E731
        y = conv1d_cl(lib, self.xd[sl], self.wd, self.bd, stride=c.get("stride", 1), pad=c["pad"], pad_mode=c["pad_mode"],
                      prologue=c.get("prologue", 0), act=c.get("act", 0), post_act=c.get("post", 0), gamma=self.gd,
                      residual=pick(self.rd), gate=pick(self.gtd), T_out=c["T_out"], in_rep=c.get("in_rep", 1),
                      ldy=c.get("ldy", c["N"]), y_offset=c.get("y_off", 0))
        return y.reshape(-1, c["N"])


@functools.lru_cache(maxsize=None)
def _small(geo, path, dev):
    c = {**GEOS[geo], **PATHS[path][1]}
    p = Problem(c, dev, zlib.crc32(f"{geo}/{c['Cin']}/{c.get('prologue', 0)}".encode()))
    return p, p.references()


def _profiled(lib, fn):
    """(fn(), launches per tile configuration) of the conv_gemm launches fn makes."""
    from unified_audio_amd import _lib

    _lib.check(lib.qa_profile_begin())
    try:
        out = fn()
    finally:
        buf = (C.c_double * 24)()
        _lib.check(lib.qa_profile_end(buf, 24))
    return out, [int(buf[4 * i + 2]) for i in range(6)]


def _pin_defaults(lib, knob):
    """Every conv_gemm knob at its built-in default (an environment override would change what the cost model picks)."""
    from unified_audio_amd import _lib

    for i in range(lib.qa_knob_count()):
        name, dflt = C.c_char_p(), C.c_int64()
        _lib.check(lib.qa_knob_info(i, C.byref(name), None, C.byref(dflt), None))
        if name.value.decode() in GEMM_KNOBS:
            knob(name.value.decode(), dflt.value)


def _check_parity(label, y, ref):
    y64, scale, e32 = ref
    e = scaled_err(y.cpu(), y64, scale)
    bound = C_PARITY * max(e32, E_FLOOR)
    print(f"conv parity {label}: e_hip {e:.3e} e_cpu32 {e32:.3e} ratio {e / max(e32, 1e-30):.2f} bound {bound:.3e}")
    assert e <= bound, f"{label}: {e:.3e} from the fp64 truth, bound {bound:.3e} (fp32 CPU {e32:.3e})"


# ---------------------------------------------------------------------------------------------------------------------------------
# (a)

@pytest.mark.parametrize("tile,path,geo", PARITY, ids=[f"cfg{t}-{p}-{g}" for t, p, g in PARITY])
def test_conv_gemm_instantiation_matches_fp64(qa_lib, gpu_device, knob, tile, path, geo):
    _pin_defaults(qa_lib, knob)
    prob, ref = _small(geo, path, gpu_device)
    knob("QA_GEMM_CFG", tile)
    for k, v in PATHS[path][0].items():
        knob(k, v)
    y, launches = _profiled(qa_lib, lambda: prob.run(qa_lib))
    cfg, bk = _launched(tile, path, prob.c)
    _check_parity(f"cfg{tile}->{TILES[cfg][0]}x{TILES[cfg][1]} BK{bk} {path} {geo}", y, ref)
    assert launches == [int(i == cfg) for i in range(6)], f"expected one launch of configuration {cfg}, got {launches}"


# ---------------------------------------------------------------------------------------------------------------------------------
# (b)

INVARIANCE = [(g, v) for g in GEOS for v in ("table_bk32", "elu", "cin48")]


@pytest.mark.parametrize("geo,variant", INVARIANCE, ids=[f"{g}-{v}" for g, v in INVARIANCE])
def test_conv_gemm_knobs_are_bit_identical(qa_lib, gpu_device, knob, geo, variant):
    """Every tile x BK x LINEAR, and every tile x XCD swizzle x panel width (0, 1, 2, 3, 8 and wider than the grid), gives the bits
    of the cost model's default launch."""
    from unified_audio_amd import _lib

    _pin_defaults(qa_lib, knob)
    prob, _ = _small(geo, variant, gpu_device)
    base = prob.run(qa_lib).clone()
    settings = []
    for tile in (-1, 0, 1, 2, 3, 4, 5):
        settings += [{"QA_GEMM_CFG": tile, "QA_GEMM_LINEAR": lin, bk: v} for lin in (0, 1)
                     for bk, v in (("QA_GEMM_BK16", 0), ("QA_GEMM_BK16_MIN_TILES", 0))]
        settings += [{"QA_GEMM_CFG": tile, "QA_GEMM_XCD": x, "QA_GEMM_PANEL": pw} for x in (0, 1) for pw in (0, 1, 2, 3, 8, 1 << 20)]
    defaults = {n: _lib.get_knob(n) for n in GEMM_KNOBS}
    odd_grid = odd_panel = False
    for s in settings:
        for k, v in {**defaults, **s}.items():
            knob(k, v)
        y, launches = _profiled(qa_lib, lambda: prob.run(qa_lib))
        cfg = launches.index(1)
        bm, bn = TILES[cfg]
        tiles_n = -(-prob.c["N"] // bn)
        odd_grid |= (-(-y.shape[0] // bm) * tiles_n) % 8 != 0
        odd_panel |= s.get("QA_GEMM_PANEL", 0) > 1 and tiles_n > s["QA_GEMM_PANEL"] and tiles_n % s["QA_GEMM_PANEL"] != 0
        assert torch.equal(y, base), f"{s} (ran {bm}x{bn}) differs from the default launch"
    assert odd_grid, "no launch had a grid of a size that is not a multiple of 8"
    if prob.c["N"] > 128:
        assert odd_panel, "no launch had a partial column panel"


# ---------------------------------------------------------------------------------------------------------------------------------
# (c), (d): rows of profiles/r05_hcodec15_gemm_shapes_serial.md (M = B * T_out, N, K = ksize * C_in), 32 clips of 10 s

SHAPES = {
    "seanet_down_640000x64x512_k16": dict(B=32, T=160000, Cin=32, N=64, k=16, stride=8, mode=1),
    "seanet_res_640000x32x192_k3_elu": dict(B=32, T=20000, Cin=64, N=32, k=3, mode=1, prologue=1, act=1),
    "agg_9056x1536x512": dict(B=32, T=283, Cin=512, N=1536, k=1),
    "agg_9056x2048x512_gelu": dict(B=32, T=283, Cin=512, N=2048, k=1, act=2),
    "agg_9056x512x2048_res": dict(B=32, T=283, Cin=2048, N=512, k=1, res=True),
    "bt_8000x3072x1024": dict(B=32, T=250, Cin=1024, N=3072, k=1),
    "dec_16000x1024x3072_k3": dict(B=32, T=500, Cin=1024, N=1024, k=3, mode=1),
    "istft_16000x1282x1024": dict(B=32, T=500, Cin=1024, N=1282, k=1),
    "down_8000x512x2048_k4_elu": dict(B=32, T=500, Cin=512, N=512, k=4, stride=2, mode=1, prologue=1),
    "rvq_1056x1024x512": dict(B=32, T=33, Cin=512, N=1024, k=1),
}


def _cost_model(M, N):
    """launch_conv_gemm's tile choice at the default knobs (QA_GEMM_256 = 0); every use is checked against the profiler."""
    if N <= 32:
        return 0
    if N <= 64:
        return 1
    best, cfg = 0.0, 2
    for c, eff in ((2, 1.0), (3, 0.914), (1, 0.913), (4, 0.871)):
        bm, bn = TILES[c]
        tiles = -(-M // bm) * -(-N // bn)
        cost = -(-tiles // 256) * bm * bn / eff * (1.25 if tiles <= 256 else 1.0)
        if best == 0.0 or cost < best * 0.995:
            best, cfg = cost, c
    return cfg


def _bk(cfg, M, c):
    """launch_cfg's K-chunk width at the default knobs: BK 16 from 384 tiles on (the profiler does not report it)."""
    bm, bn = TILES[cfg]
    tiles = -(-M // bm) * -(-c["N"] // bn)
    return 16 if bn >= 64 and not c.get("prologue") and (tiles >= 384 or c["Cin"] % 32) else 32


def _sample_rows(c, seed):
    B, To = c["B"], c["T_out"]
    M = B * To
    rows = {r for b in range(B) for r in (b * To, b * To + To - 1)}  # every clip boundary
    for bm in (64, 128, 256):  # the first and last row of the last (ragged) row tile of every tile height
        rows |= {(M - 1) // bm * bm, M - 1}
    g = torch.Generator().manual_seed(seed)
    rows |= set(torch.randint(0, M, (256,), generator=g).tolist())
    return torch.tensor(sorted(rows))


@functools.lru_cache(maxsize=1)
def _at_size(name, dev):
    c = _geometry(SHAPES[name])
    return Problem(c, dev, zlib.crc32(name.encode()), rows=_sample_rows(c, zlib.crc32(name.encode()) + 1))


@pytest.mark.parametrize("name", list(SHAPES))
def test_conv_gemm_headline_shapes_match_fp64_on_sampled_rows(qa_lib, gpu_device, knob, name):
    _pin_defaults(qa_lib, knob)
    prob = _at_size(name, gpu_device)
    c = prob.c
    M = c["B"] * c["T_out"]
    y, launches = _profiled(qa_lib, lambda: prob.run(qa_lib))
    cfg = _cost_model(M, c["N"])
    assert launches == [int(i == cfg) for i in range(6)], f"cost model: expected configuration {cfg}, got {launches}"
    ys = y[prob.rows.to(gpu_device)]
    _check_parity(f"{name} {TILES[cfg][0]}x{TILES[cfg][1]} BK{_bk(cfg, M, c)} ({len(prob.rows)} rows)", ys, prob.references())


SPLITS = [n for n in SHAPES if n not in ("seanet_res_640000x32x192_k3_elu", "rvq_1056x1024x512")]  # these two: one (tile, BK) for any batch


@pytest.mark.parametrize("name", SPLITS)
def test_conv_gemm_headline_shapes_batch_split_is_bit_identical(qa_lib, gpu_device, knob, name):
    _pin_defaults(qa_lib, knob)
    prob = _at_size(name, gpu_device)
    c = prob.c
    B, To, N = c["B"], c["T_out"], c["N"]
    full, launches = _profiled(qa_lib, lambda: prob.run(qa_lib))
    pair = lambda b: (_cost_model(b * To, N), _bk(_cost_model(b * To, N), b * To, c))  # noqa: E731
    assert launches.index(1) == pair(B)[0]
    # the last clip alone, and the smallest sub-batch of the first clips whose (tile, BK) differs from the full batch's and the
    # clip's - or at least from the full batch's
    subs = [b for b in range(2, B) if pair(b) not in (pair(B), pair(1))] or [b for b in range(2, B) if pair(b) != pair(B)]
    splits = [("last clip", slice(B - 1, B), pair(1))] + ([(f"first {subs[0]} clips", slice(0, subs[0]), pair(subs[0]))] if subs else [])
    for label, sl, (cfg, bk) in splits:
        y, launches = _profiled(qa_lib, lambda: prob.run(qa_lib, sl))
        assert launches == [int(i == cfg) for i in range(6)], f"{label}: expected configuration {cfg}, got {launches}"
        print(f"conv split {name}: {label} ran {TILES[cfg][0]}x{TILES[cfg][1]} BK{bk}, the full batch "
              f"{TILES[pair(B)[0]][0]}x{TILES[pair(B)[0]][1]} BK{pair(B)[1]}")
        assert torch.equal(y, full[sl.start * To:sl.stop * To]), f"{label} ({cfg}, BK {bk}) differs from the full batch {pair(B)}"
    tried = [p for _, _, p in splits]
    assert all(p != pair(B) for p in tried), "a split took the full batch's own (tile, BK): it proves nothing"
    if not c.get("prologue"):  # the ELU prologue exists with BK = 32 only
        assert any(p[1] != pair(B)[1] for p in tried), "no split crossed the BK 16 threshold"
    if N > 64:  # N <= 64 takes 128 x 64 (N <= 32: 128 x 32) for any M
        assert any(p[0] != pair(B)[0] for p in tried), "no split changed the tile"
