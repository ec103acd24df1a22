"""The operand split of conv_gemm's bf16-plane arithmetics (csrc/split_planes.h), restated with torch's own round-to-nearest-even
bfloat16 conversion: x = h + m + l with h = rne(x), m = rne(x - h), l = rne(x - h - m), the residual zeroed where it is not finite
(inf, NaN, and finite values that round to bf16 inf).  QA_GEMM_MATH = 1 (split-6) keeps three planes, 2 (split-3) the first two,
3 (bf16) the first."""
import torch

PLANES_OF_MODE = {1: 3, 2: 2, 3: 1}  # QA_GEMM_MATH -> planes kept
UNIT = {1: 2.0 ** -8, 2: 2.0 ** -16}   # planes kept -> bound of |x - rounded(x, n)| / |x|


def _rne(x):
    return x.to(torch.bfloat16).to(torch.float32)


def planes(x, n=3):
    """The first n of the fp32 tensors (h, m, l)."""
    assert x.dtype == torch.float32 and 1 <= n <= 3
    out, r = [], x
    for i in range(n):
        if i:
            r = r - out[-1]  # exact in fp32
            r = torch.where(torch.isfinite(r), r, torch.zeros_like(r))
        out.append(_rne(r))
    return tuple(out)


def rounded(x, n):
    """The operand a mode with n planes multiplies: the sum of the first n planes (exact in fp32: at most 24 significant bits of x)."""
    p = planes(x, n)
    y = p[0]
    for q in p[1:]:
        y = y + q
    return y
