// split_planes.h - the operand split of the split-6 arithmetic (conv_gemm, attention) and the memory layout of a pre-split weight image.
//
// The K loop (activations, and weights without an image) and the load-time image builder run the SAME device function, so an image
// holds bit for bit what the loop would have produced.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace qa {

typedef float f32x4 __attribute__((ext_vector_type(4)));  // native vector: stays in VGPRs (float4 arrays were left as scratch allocas)
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));   // one operand fragment of v_mfma_f32_32x32x16_bf16 / v_mfma_f32_16x16x32_bf16
typedef float f32x16 __attribute__((ext_vector_type(16)));  // one 32x32 accumulator

// Split-6 math (QA_GEMM_MATH = 1).  Each operand is split, exactly, into three bf16 planes x = h + m + l by round-to-nearest-even:
// h = rne(x), m = rne(x - h), l = x - h - m.  Both subtractions are exact and l keeps <= 8 significant bits (sign borrowing), so
// |m| <= 2^-8 |x| and |l| <= 2^-16 |x|.  A k group - 32 wide in conv_gemm (v_mfma_f32_16x16x32_bf16), 16 wide in attention
// (v_mfma_f32_32x32x16_bf16) - then takes six MFMAs (every bf16 x bf16 product is exact in fp32), smallest terms first: hl, lh, mm, hm,
// mh, hh (activation plane first).  The dropped ml, lm and ll are each <= 2^-24 |ab|,
// the size of one fp32 rounding, of random sign.  Non-finite x: h = x and m = l = 0 (the residual is zeroed when it is not finite),
// so inf and NaN reach the sum through hh exactly as through the fp32 chain.  A finite |x| that rounds past the largest bf16
// (>= 2^128 (1 - 2^-9)) becomes h = inf.
// The plane pairs of a k group in issue order (planes 0 = h, 1 = m, 2 = l).  Smallest terms first: the accumulator takes the 2^-16-sized
// hl and lh and the mm before the 2^-8-sized hm and mh and the full-sized hh, so the small terms are summed among themselves before a
// large partial sum can round them away.  PAIR_A is the plane of the first-named operand (conv_gemm: the activation; attention: the LDS
// operand, K or V), PAIR_B that of the second (conv_gemm: the weight; attention: the register operand, Q or P).
constexpr int PAIR_A[6] = {0, 2, 1, 0, 1, 0}, PAIR_B[6] = {2, 0, 1, 1, 0, 0};
__device__ __forceinline__ unsigned rne_bf16x2(float a, float b) {  // low half bf16(a), high half bf16(b): one v_cvt_pk_bf16_f32
    const f32x2 v = {a, b};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
}
__device__ __forceinline__ void split4_rne(const f32x4 x, u32x2& ph, u32x2& pm, u32x2& pl) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const float a = x[2 * i], b = x[2 * i + 1];
        const unsigned h = rne_bf16x2(a, b);
        float ra = a - __builtin_bit_cast(float, h << 16), rb = b - __builtin_bit_cast(float, h & 0xffff0000u);
        ra = __builtin_isfinite(ra) ? ra : 0.f;
        rb = __builtin_isfinite(rb) ? rb : 0.f;
        const unsigned m = rne_bf16x2(ra, rb);
        ph[i] = h;
        pm[i] = m;
        pl[i] = rne_bf16x2(ra - __builtin_bit_cast(float, m << 16), rb - __builtin_bit_cast(float, m & 0xffff0000u));  // exact
    }
}
// The reduced arithmetics of conv_gemm keep the first NPL planes of the same split and, of the table above, the pairs of kept planes whose
// product is at least as large as the operands' own truncation: plane p is 2^-8p of its operand, so pair (a, b) is 2^-8(a + b) of the product,
// and a form with NPL planes issues the pairs with a + b < NPL, in the table's order.  NPL = 3 is split-6 (ml, lm, ll dropped).  Split-3
// (QA_GEMM_MATH = 2, NPL = 2): x ~ h + m, exact to 2^-16 |x|, products hm, mh, hh; the dropped mm is <= 2^-16 |ab|.  bf16 (QA_GEMM_MATH = 3,
// NPL = 1): x ~ h, exact to 2^-8 |x|, the one product hh.
__host__ __device__ constexpr bool pair_kept(int q, int npl) { return PAIR_A[q] + PAIR_B[q] < npl; }
// split4_rne's first two planes (the same bits) without the third
__device__ __forceinline__ void split4_rne2(const f32x4 x, u32x2& ph, u32x2& pm) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const float a = x[2 * i], b = x[2 * i + 1];
        const unsigned h = rne_bf16x2(a, b);
        float ra = a - __builtin_bit_cast(float, h << 16), rb = b - __builtin_bit_cast(float, h & 0xffff0000u);
        ra = __builtin_isfinite(ra) ? ra : 0.f;
        rb = __builtin_isfinite(rb) ? rb : 0.f;
        ph[i] = h;
        pm[i] = rne_bf16x2(ra, rb);
    }
}
// ... and its first plane alone
__device__ __forceinline__ void split4_rne1(const f32x4 x, u32x2& ph) {
    ph[0] = rne_bf16x2(x[0], x[1]);
    ph[1] = rne_bf16x2(x[2], x[3]);
}
template <int NPL>  // the first NPL planes; the others are left untouched
__device__ __forceinline__ void split4_planes(const f32x4 x, u32x2& ph, u32x2& pm, u32x2& pl) {
    static_assert(NPL >= 1 && NPL <= 3, "one to three planes");
    if constexpr (NPL == 3) split4_rne(x, ph, pm, pl);
    else if constexpr (NPL == 2) split4_rne2(x, ph, pm);
    else split4_rne1(x, ph);
}
__device__ __forceinline__ void split4_unit(const f32x4 x, u32x2& ph, u32x2& pm, u32x2& pl) {  // split4_rne for x in [0, 1]
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const float a = x[2 * i], b = x[2 * i + 1];
        const unsigned h = rne_bf16x2(a, b);
        const float ra = a - __builtin_bit_cast(float, h << 16), rb = b - __builtin_bit_cast(float, h & 0xffff0000u);
        const unsigned m = rne_bf16x2(ra, rb);
        ph[i] = h;
        pm[i] = m;
        pl[i] = rne_bf16x2(ra - __builtin_bit_cast(float, m << 16), rb - __builtin_bit_cast(float, m & 0xffff0000u));  // exact
    }
}
__device__ __forceinline__ bf16x8 frag8(const u32x2 lo, const u32x2 hi) {  // two split4 halves of one plane -> an MFMA fragment
    const u32x4 t = {lo[0], lo[1], hi[0], hi[1]};
    return __builtin_bit_cast(bf16x8, t);
}

// Pre-split weight image (QA_GEMM_PRESPLIT).  The image of a float array w[0 .. n), n % 8 == 0, holds 6 bytes per weight: every
// aligned group of 8 floats becomes three consecutive 16-byte units - its h, m and l planes, 8 bf16 each, in the order of the floats.
// A unit is exactly one 16-byte slot of one plane row of the K loop's LDS image, so a staging thread moves it with one 16-byte global
// load and one ds_write_b128, and the 32-wide chunk of a weight row is 192 contiguous bytes.  The address depends on the float's index
// alone: the image of a row slice w + r * K (K % 8 == 0) is the image of w advanced by plane_byte_offset(r * K, 0).
constexpr int PLANE_GROUP_BYTES = 48;  // image bytes per 8 floats
__host__ __device__ constexpr long long plane_byte_offset(long long index, int plane) {
    return (index >> 3) * PLANE_GROUP_BYTES + plane * 16 + (index & 7) * 2;
}

}  // namespace qa
