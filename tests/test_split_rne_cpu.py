"""The split of conv_gemm's split-6 arithmetic (csrc/conv_gemm.hip split4_rne), emulated in numpy: h = rne_bf16(x),
r = x - h (zeroed when not finite), m = rne_bf16(r), l = rne_bf16(r - m).  Claims checked: both subtractions are exact and, for
|x| >= 2^-110, r - m is itself a bf16, so x == h + m + l exactly, |m| <= 2^-8 |x| and |l| <= 2^-16 |x|; below 2^-110 the last plane
can fall under bf16's subnormal grid (2^-133) and the split is off by at most 2^-134; inf gives h = inf, m = l = 0; NaN gives
h = NaN, m = l = 0."""
import numpy as np


def rne_bf16(x):
    """float32 -> nearest bf16 (ties to even), returned as float32; NaN stays NaN (v_cvt_pk_bf16_f32)."""
    u = np.asarray(x, np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32).view(np.float32)
    return np.where(np.isnan(x), np.float32(np.nan), r).astype(np.float32)


def split(x):
    x = np.asarray(x, np.float32)
    h = rne_bf16(x)
    with np.errstate(invalid="ignore", over="ignore"):
        r = (x - h).astype(np.float32)
    r = np.where(np.isfinite(r), r, np.float32(0)).astype(np.float32)
    m = rne_bf16(r)
    lo = rne_bf16((r - m).astype(np.float32))
    return h, m, lo


def _values():
    rng = np.random.default_rng(3)
    vals = [
        rng.standard_normal(20000).astype(np.float32),
        (rng.standard_normal(20000) * np.exp2(rng.integers(-120, 120, 20000))).astype(np.float32),
        rng.integers(0, 0x7F7F8000, 20000, dtype=np.uint32).view(np.float32),        # every finite bit pattern below 2^128 (1 - 2^-9)
        (rng.integers(1, 1 << 23, 5000, dtype=np.uint32)).view(np.float32),          # subnormals
        np.array([0.0, -0.0, 1.0, -1.0, 1.0 + 2.0 ** -23, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -9, 1.0 + 2.0 ** -9 + 2.0 ** -17,
                  1.0 - 2.0 ** -24, 3.3895314e38, -3.3895314e38, 2.0 ** -126, 2.0 ** -149, 65504.0], np.float32),
    ]
    v = np.concatenate(vals)
    return np.concatenate([v, -v])


def test_split_is_exact_and_the_planes_are_bf16():
    x = _values()
    h, m, lo = split(x)
    for p in (h, m, lo):
        assert np.all(p.view(np.uint32) & 0xFFFF == 0), "a plane holds more than 8 significand bits"
    ax = np.abs(x.astype(np.float64))
    s = h.astype(np.float64) + m.astype(np.float64) + lo.astype(np.float64)
    big = ax >= 2.0 ** -110
    assert np.array_equal(s[big], x.astype(np.float64)[big])
    assert np.all(np.abs(s - x.astype(np.float64))[~big] <= 2.0 ** -134)
    assert np.all(np.abs(m.astype(np.float64)) <= ax * 2.0 ** -8)
    assert np.all(np.abs(lo.astype(np.float64)) <= ax * 2.0 ** -16 + 2.0 ** -149)


def test_split_of_non_finite_values():
    x = np.array([np.inf, -np.inf, np.nan], np.float32)
    h, m, lo = split(x)
    assert h[0] == np.inf and h[1] == -np.inf and np.isnan(h[2])
    assert np.all(m == 0) and np.all(lo == 0)


def test_six_products_drop_at_most_three_fp32_roundings():
    """|ml + lm + ll| <= 3 * 2^-24 |a b| for normal operands: what the six-product form leaves out."""
    rng = np.random.default_rng(4)
    a = (rng.standard_normal(50000) * np.exp2(rng.integers(-30, 30, 50000))).astype(np.float32)
    b = (rng.standard_normal(50000) * np.exp2(rng.integers(-30, 30, 50000))).astype(np.float32)
    ah, am, al = (p.astype(np.float64) for p in split(a))
    bh, bm, bl = (p.astype(np.float64) for p in split(b))
    dropped = am * bl + al * bm + al * bl
    kept = ah * bl + al * bh + am * bm + ah * bm + am * bh + ah * bh
    ab = a.astype(np.float64) * b.astype(np.float64)
    assert np.all(np.abs(kept + dropped - ab) <= np.abs(ab) * 2.0 ** -50)
    assert np.all(np.abs(dropped) <= 3 * 2.0 ** -24 * np.abs(ab))
