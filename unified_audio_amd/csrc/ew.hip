// ew.hip - HBM-bound row / elementwise kernels of the codec graph (channel-last [rows, C] activations):
// first conv (C_in = 1), RMSNorm, LayerNorm, depthwise conv (+ fused LayerNorm), GroupNorm (+ swish),
// RoPE, layout conversions, ISTFT spectrum + overlap-add.  All are one-pass, float4-coalesced, one wave64
// per activation row where a row reduction is needed.
#include "kernels.h"

namespace qa {

// ------------------------------------------------------------------------------------------------
// conv_in: SConv1d with C_in = 1 (reference: encoder.model.0, encoder_modules/conv.py:195-211; seanet.py:121-124)
// y[b, t, co] = bias[co] + sum_j w[co, j] * x[b, reflect(t - pad_left + j)]
// one thread = one output frame x 4 channels -> float4 stores, consecutive threads write consecutive 16 B.
// Tx: the frames of x per item (= T, or T + ksize - 1 in the window form, whose taps all land inside the window: pad_left = 0, Lp = Tx).
__global__ __launch_bounds__(256) void conv_in_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                      const float* __restrict__ bias, float* __restrict__ y, int B,
                                                      int T, int Cout, int ksize, int pad_left, int Lp,
                                                      const int* __restrict__ lens, int len_mul, int max_pad, int Tx) {
    const int c4n = Cout >> 2;
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long total = (long long)B * T * c4n;
    if (gid >= total) return;
    const int c4 = (int)(gid % c4n);
    const long long m = gid / c4n;
    const int b = (int)(m / T), t = (int)(m - (long long)b * T);
    const float* xb = x + (long long)b * Tx;
    int len = Tx;
    if (lens) {  // launch-uniform: a ragged call reflects at the clip's own end (short-input rule included)
        len = min(lens[b] * len_mul, T);
        Lp = len <= max_pad ? max_pad + 1 : len;
    }
    float4 acc = bias ? *reinterpret_cast<const float4*>(bias + c4 * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
    for (int j = 0; j < ksize; ++j) {
        const int src = resolve_frame(t - pad_left + j, len, Lp, PAD_REFLECT);
        const float xv = src >= 0 ? xb[src] : 0.f;
        const float* wj = w + (long long)j * Cout + c4 * 4;  // library layout [ksize][Cout]
        acc.x = fmaf(xv, wj[0], acc.x);
        acc.y = fmaf(xv, wj[1], acc.y);
        acc.z = fmaf(xv, wj[2], acc.z);
        acc.w = fmaf(xv, wj[3], acc.w);
    }
    *reinterpret_cast<float4*>(y + m * Cout + c4 * 4) = acc;
}

int launch_conv_in(const float* x, const float* w_kc, const float* bias, float* y, int B, int T, int Cout, int ksize,
                   hipStream_t s, int pad_left, ClipLens rl) {
    QA_REQUIRE(Cout % 4 == 0 && pad_left < ksize, "conv_in: Cout=%d must be a multiple of 4 (pad_left %d, ksize %d)", Cout, pad_left, ksize);
    const int pad_total = ksize - 1;
    const int left = pad_left >= 0 ? pad_left : pad_total - pad_total / 2, right = pad_total - left;
    const int max_pad = left > right ? left : right;
    const int Lp = (T <= max_pad) ? max_pad + 1 : T;
    const long long total = (long long)B * T * (Cout / 4);
    HbmProf prof_(HK_CONV_IN, 4.0 * ((double)B * T + (double)B * T * Cout), s);
    hipLaunchKernelGGL(conv_in_kernel, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, s, x, w_kc, bias, y, B, T,
                       Cout, ksize, left, Lp, rl.n, rl.mul, max_pad, T);
    QA_LAUNCH_CHECK();
    return QA_OK;
}

int launch_conv_in_window(const float* x, const float* w_kc, const float* bias, float* y, int B, int T_in, int Cout, int ksize, hipStream_t s) {
    QA_REQUIRE(Cout % 4 == 0 && ksize >= 1 && T_in >= ksize, "conv_in (window): Cout=%d must be a multiple of 4, the window of %d frames "
               "at least ksize = %d", Cout, T_in, ksize);
    const int T = T_in - ksize + 1;  // tap j of output t reads window frame t + j <= T_in - 1: resolve_frame returns it as it is
    const long long total = (long long)B * T * (Cout / 4);
    HbmProf prof_(HK_CONV_IN, 4.0 * ((double)B * T_in + (double)B * T * Cout), s);
    hipLaunchKernelGGL(conv_in_kernel, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, s, x, w_kc, bias, y, B, T, Cout, ksize, 0, T_in,
                       static_cast<const int*>(nullptr), 0, 0, T_in);
    QA_LAUNCH_CHECK();
    return QA_OK;
}

// ------------------------------------------------------------------------------------------------
// Row norms: one wave per row, up to 8 float4 per lane (C <= 2048).
constexpr int MAX_V4 = 8;

// mode 0: RMSNorm (transformer.py:77-96, eps inside the sqrt of mean(x^2)), mode 1: LayerNorm (biased variance)
template <int MODE>
__global__ __launch_bounds__(256) void rownorm_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                      const float* __restrict__ b, float* __restrict__ y,
                                                      long long rows, int C, float eps) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* xr = x + row * C;
    float4 v[MAX_V4];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < MAX_V4; ++i) {
        const int c = lane * 4 + i * 256;
        if (c < C) {
            v[i] = *reinterpret_cast<const float4*>(xr + c);
            s += (MODE == 0) ? (v[i].x * v[i].x + v[i].y * v[i].y + v[i].z * v[i].z + v[i].w * v[i].w)
                             : (v[i].x + v[i].y + v[i].z + v[i].w);
        }
    }
    s = wave_sum(s);
    float mean = 0.f, rstd;
    if (MODE == 0) {
        rstd = rsqrtf(s / C + eps);
    } else {
        mean = s / C;
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < MAX_V4; ++i) {
            if (lane * 4 + i * 256 < C) {
                const float a = v[i].x - mean, bb = v[i].y - mean, cc = v[i].z - mean, d = v[i].w - mean;
                q += a * a + bb * bb + cc * cc + d * d;
            }
        }
        q = wave_sum(q);
        rstd = rsqrtf(q / C + eps);
    }
    float* yr = y + row * C;
#pragma unroll
    for (int i = 0; i < MAX_V4; ++i) {
        const int c = lane * 4 + i * 256;
        if (c >= C) continue;
        const float4 ww = *reinterpret_cast<const float4*>(w + c);
        float4 o;
        o.x = (v[i].x - mean) * rstd * ww.x;
        o.y = (v[i].y - mean) * rstd * ww.y;
        o.z = (v[i].z - mean) * rstd * ww.z;
        o.w = (v[i].w - mean) * rstd * ww.w;
        if (MODE == 1 && b) {
            const float4 bv = *reinterpret_cast<const float4*>(b + c);
            o.x += bv.x; o.y += bv.y; o.z += bv.z; o.w += bv.w;
        }
        *reinterpret_cast<float4*>(yr + c) = o;
    }
}

int launch_rmsnorm(const float* x, const float* w, float* y, long long rows, int C, float eps, hipStream_t s) {
    QA_REQUIRE(C % 4 == 0 && C <= 256 * MAX_V4, "rmsnorm: C=%d unsupported", C);
    HbmProf prof_(HK_ROWNORM, 8.0 * (double)rows * C, s);
    hipLaunchKernelGGL(rownorm_kernel<0>, dim3((unsigned)ceil_div(rows, 4)), dim3(256), 0, s, x, w, nullptr, y, rows,
                       C, eps);
    QA_LAUNCH_CHECK();
    return QA_OK;
}
int launch_layernorm(const float* x, const float* w, const float* b, float* y, long long rows, int C, float eps,
                     hipStream_t s) {
    QA_REQUIRE(C % 4 == 0 && C <= 256 * MAX_V4, "layernorm: C=%d unsupported", C);
    HbmProf prof_(HK_ROWNORM, 8.0 * (double)rows * C, s);
    hipLaunchKernelGGL(rownorm_kernel<1>, dim3((unsigned)ceil_div(rows, 4)), dim3(256), 0, s, x, w, b, y, rows, C,
                       eps);
    QA_LAUNCH_CHECK();
    return QA_OK;
}

// ------------------------------------------------------------------------------------------------
// Depthwise Conv1d (zero "same" padding, vq/conv.py:33-56) with optional fused LayerNorm over channels
// (ConvNeXtBlock: dwconv k7 -> LN, vq/conv.py:200-203; sub-pixel upsampler's dw k5, vq/conv.py:86-90).
// w layout [ksize][C] so that lanes read consecutive channels.
template <bool LN>
__global__ __launch_bounds__(256) void dwconv_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                     const float* __restrict__ bias, const float* __restrict__ lnw,
                                                     const float* __restrict__ lnb, float* __restrict__ y, int B, int T,
                                                     int C, int ksize, float eps, int pad, const int* __restrict__ lens, int len_mul) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= (long long)B * T) return;
    const int b = (int)(row / T), t = (int)(row - (long long)b * T);
    const float* xb = x + (long long)b * T * C;
    const int len = lens ? min(lens[b] * len_mul, T) : T;  // launch-uniform test; ragged: zero padding starts at the clip's own end
    float4 v[MAX_V4];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < MAX_V4; ++i) {
        const int c = lane * 4 + i * 256;
        if (c >= C) continue;
        float4 acc = *reinterpret_cast<const float4*>(bias + c);
        for (int j = 0; j < ksize; ++j) {
            const int src = t + j - pad;
            if (src < 0 || src >= len) continue;
            const float4 xv = *reinterpret_cast<const float4*>(xb + (long long)src * C + c);
            const float4 wv = *reinterpret_cast<const float4*>(w + (long long)j * C + c);
            acc.x = fmaf(xv.x, wv.x, acc.x);
            acc.y = fmaf(xv.y, wv.y, acc.y);
            acc.z = fmaf(xv.z, wv.z, acc.z);
            acc.w = fmaf(xv.w, wv.w, acc.w);
        }
        v[i] = acc;
        s += acc.x + acc.y + acc.z + acc.w;
    }
    float mean = 0.f, rstd = 1.f;
    if (LN) {
        mean = wave_sum(s) / C;
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < MAX_V4; ++i) {
            if (lane * 4 + i * 256 < C) {
                const float a = v[i].x - mean, bb = v[i].y - mean, cc = v[i].z - mean, d = v[i].w - mean;
                q += a * a + bb * bb + cc * cc + d * d;
            }
        }
        rstd = rsqrtf(wave_sum(q) / C + eps);
    }
    float* yr = y + row * C;
#pragma unroll
    for (int i = 0; i < MAX_V4; ++i) {
        const int c = lane * 4 + i * 256;
        if (c >= C) continue;
        float4 o = v[i];
        if (LN) {
            const float4 ww = *reinterpret_cast<const float4*>(lnw + c);
            const float4 bv = *reinterpret_cast<const float4*>(lnb + c);
            o.x = (o.x - mean) * rstd * ww.x + bv.x;
            o.y = (o.y - mean) * rstd * ww.y + bv.y;
            o.z = (o.z - mean) * rstd * ww.z + bv.z;
            o.w = (o.w - mean) * rstd * ww.w + bv.w;
        }
        *reinterpret_cast<float4*>(yr + c) = o;
    }
}

int launch_dwconv(const float* x, const float* w_kc, const float* bias, const float* lnw, const float* lnb, float* y,
                  int B, int T, int C, int ksize, float eps, hipStream_t s, int pad_left, ClipLens rl) {
    QA_REQUIRE(C % 4 == 0 && C <= 256 * MAX_V4 && (ksize & 1) && pad_left < ksize, "dwconv: C=%d ksize=%d pad_left=%d unsupported", C,
               ksize, pad_left);
    const unsigned grid = (unsigned)ceil_div((long long)B * T, 4);
    const int pad = pad_left >= 0 ? pad_left : ksize / 2;
    HbmProf prof_(HK_DWCONV_LN, 8.0 * (double)B * T * C, s);
    if (lnw)
        hipLaunchKernelGGL(dwconv_kernel<true>, dim3(grid), dim3(256), 0, s, x, w_kc, bias, lnw, lnb, y, B, T, C, ksize,
                           eps, pad, rl.n, rl.mul);
    else
        hipLaunchKernelGGL(dwconv_kernel<false>, dim3(grid), dim3(256), 0, s, x, w_kc, bias, lnw, lnb, y, B, T, C,
                           ksize, eps, pad, rl.n, rl.mul);
    QA_LAUNCH_CHECK();
    return QA_OK;
}

// ------------------------------------------------------------------------------------------------
// GroupNorm(G, C, eps) over [B, T, C] channel-last (vq/conv.py:259-260 "Normalize"), optional swish after it
// (ResnetBlock.nonlinearity, vq/conv.py:303-304).  Two deterministic passes, no atomics, a fixed fold order:
//   1. gn_partial: grid (chunks, B); each block reduces `rows_per_chunk` frames: thread = one float4 channel
//      column, running sum / sum of squares in DOUBLE, as ssl_conv0_kernel keeps them (a float squared is exact in
//      double, so var = E[x^2] - mean^2 keeps 29 more bits than the data has when the group's mean is large against its
//      deviation, as behind a swish; with fp32 sums a group at 100 +- 0.5 came out wrong by 4e-3), then a group
//      reduction in LDS -> partial[b][chunk][g][2] (double)
//   2. gn_apply: every block first folds the partials of its batch item in a fixed order (LDS), then streams.  The
//      mean is kept as a float pair (hi + lo): x - hi is exact for x near the mean, so the fp32 rounding of a large
//      mean does not enter the output either.
// 32 frames per chunk: twice the workgroups of the 64-frame chunks this kernel had with fp32 sums, which more than pays for the double
// arithmetic (profiles/groupnorm_offset_fix.md)
constexpr int GN_ROWS = 32;
constexpr int GN_MAX_C = 4096;  // gn_partial's LDS: 2 * C doubles

__global__ __launch_bounds__(256) void gn_partial_kernel(const float* __restrict__ x, double* __restrict__ partial,
                                                         int T, int C, int G, const int* __restrict__ lens, int len_mul) {
    extern __shared__ double shd[];  // [2][C]
    const int b = blockIdx.y, chunk = blockIdx.x, nchunk = gridDim.x;
    const int len = lens ? min(lens[b] * len_mul, T) : T;  // ragged: a chunk behind the clip's end sums nothing and stores exact zeros
    const int t0 = chunk * GN_ROWS, t1 = min(len, t0 + GN_ROWS);
    const float* xb = x + (long long)b * T * C;
    for (int c = threadIdx.x * 4; c < C; c += blockDim.x * 4) {
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, q0 = 0.0, q1 = 0.0, q2 = 0.0, q3 = 0.0;
        for (int t = t0; t < t1; ++t) {
            const float4 v = *reinterpret_cast<const float4*>(xb + (long long)t * C + c);
            const double a0 = v.x, a1 = v.y, a2 = v.z, a3 = v.w;
            s0 += a0; s1 += a1; s2 += a2; s3 += a3;
            q0 = fma(a0, a0, q0); q1 = fma(a1, a1, q1); q2 = fma(a2, a2, q2); q3 = fma(a3, a3, q3);
        }
        shd[c] = s0; shd[c + 1] = s1; shd[c + 2] = s2; shd[c + 3] = s3;
        shd[C + c] = q0; shd[C + c + 1] = q1; shd[C + c + 2] = q2; shd[C + c + 3] = q3;
    }
    __syncthreads();
    const int cpg = C / G;
    for (int g = threadIdx.x; g < G; g += blockDim.x) {
        double s = 0.0, q = 0.0;
        for (int c = g * cpg; c < (g + 1) * cpg; ++c) {
            s += shd[c];
            q += shd[C + c];
        }
        double* out = partial + (((long long)b * nchunk + chunk) * G + g) * 2;
        out[0] = s;
        out[1] = q;
    }
}

__global__ __launch_bounds__(256) void gn_apply_kernel(const float* __restrict__ x, const double* __restrict__ partial,
                                                       const float* __restrict__ w, const float* __restrict__ bias,
                                                       float* __restrict__ y, int T, int C, int G, int nchunk, float eps,
                                                       int swish, const int* __restrict__ lens, int len_mul) {
    extern __shared__ float sh[];  // [3][G]: mean (hi), mean (lo), rstd
    const int b = blockIdx.y;
    const int cpg = C / G;
    for (int g = threadIdx.x; g < G; g += blockDim.x) {
        double s = 0.0, q = 0.0;
        for (int k = 0; k < nchunk; ++k) {
            const double* pp = partial + (((long long)b * nchunk + k) * G + g) * 2;
            s += pp[0];
            q += pp[1];
        }
        const double n = (double)(lens ? min(lens[b] * len_mul, T) : T) * cpg;  // ragged: statistics over the clip's own frames
        const double mean = s / n;
        double var = q / n - mean * mean;
        if (var < 0.0) var = 0.0;
        const float hi = (float)mean;
        sh[g] = hi;
        sh[G + g] = (float)(mean - (double)hi);
        sh[2 * G + g] = (float)(1.0 / sqrt(var + (double)eps));
    }
    __syncthreads();
    const int c4n = C >> 2;
    const long long n4 = (long long)T * c4n;
    const float* xb = x + (long long)b * T * C;
    float* yb = y + (long long)b * T * C;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % c4n) * 4;
        const float4 v = *reinterpret_cast<const float4*>(xb + i * 4);
        const float4 ww = *reinterpret_cast<const float4*>(w + c);
        const float4 bv = *reinterpret_cast<const float4*>(bias + c);
        // channels c..c+3 may straddle groups only if cpg % 4 != 0 -> resolve per element
        const int g0 = (c + 0) / cpg, g1 = (c + 1) / cpg, g2 = (c + 2) / cpg, g3 = (c + 3) / cpg;
        float4 o;
        o.x = ((v.x - sh[g0]) - sh[G + g0]) * sh[2 * G + g0] * ww.x + bv.x;
        o.y = ((v.y - sh[g1]) - sh[G + g1]) * sh[2 * G + g1] * ww.y + bv.y;
        o.z = ((v.z - sh[g2]) - sh[G + g2]) * sh[2 * G + g2] * ww.z + bv.z;
        o.w = ((v.w - sh[g3]) - sh[G + g3]) * sh[2 * G + g3] * ww.w + bv.w;
        if (swish) {
            o.x = silu_f(o.x); o.y = silu_f(o.y); o.z = silu_f(o.z); o.w = silu_f(o.w);
        }
        *reinterpret_cast<float4*>(yb + i * 4) = o;
    }
}

size_t groupnorm_scratch_bytes(int B, int T, int G) { return (size_t)B * ceil_div(T, GN_ROWS) * G * 2 * sizeof(double); }

int launch_groupnorm(const float* x, const float* w, const float* bias, float* y, double* scratch, int B, int T, int C,
                     int G, float eps, int swish, hipStream_t s, ClipLens rl) {
    QA_REQUIRE(C % 4 == 0 && C <= GN_MAX_C && G >= 1 && C % G == 0, "groupnorm: C=%d G=%d unsupported", C, G);
    const int nchunk = (int)ceil_div(T, GN_ROWS);
    HbmProf prof_(HK_GROUPNORM, 8.0 * (double)B * T * C, s);  // algorithmic: x once in, y once out (the two-pass form reads x twice)
    hipLaunchKernelGGL(gn_partial_kernel, dim3(nchunk, B), dim3(256), 2 * C * sizeof(double), s, x, scratch, T, C, G, rl.n, rl.mul);
    QA_LAUNCH_CHECK();
    const long long n4 = (long long)T * (C / 4);
    const unsigned gx = (unsigned)std::min<long long>(ceil_div(n4, 256), 64);
    hipLaunchKernelGGL(gn_apply_kernel, dim3(gx, B), dim3(256), 3 * G * sizeof(float), s, x, scratch, w, bias, y, T, C,
                       G, nchunk, eps, swish, rl.n, rl.mul);
    QA_LAUNCH_CHECK();
    return QA_OK;
}

// ------------------------------------------------------------------------------------------------
// Rotate-half RoPE applied in place to the q and k parts of a fused [rows, 3*d] QKV buffer
// (transformer.py:182-215: q*cos + rotate_half(q)*sin, positions 0..N-1, tables as RotaryEmbedding.forward).
__global__ __launch_bounds__(256) void rope_kernel(float* __restrict__ qkv, const float* __restrict__ cs, int B, int N,
                                                   int H, int hd, long long ld, int pos0, int interleaved, int Hr) {
    // one thread: one (row, head < Hr, pair i < hd/2) for q and for k
    const int half = hd >> 1;
    const long long total = (long long)B * N * Hr * half;
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= total) return;
    const int i = (int)(gid % half);
    const int h = (int)((gid / half) % Hr);
    const long long row = gid / ((long long)half * Hr);
    const int t = (int)(row % N) + pos0;
    const float c = cs[((long long)t * half + i) * 2], s = cs[((long long)t * half + i) * 2 + 1];
    const int d = H * hd;
    float* q = qkv + row * ld + h * hd;
    float* k = q + d;
    // rotate-half pairs (i, i + hd/2) (HF Llama / codec transformers) or interleaved pairs (2i, 2i+1) (mimi, module/rope.py:13-69)
    const int i0 = interleaved ? 2 * i : i, i1 = interleaved ? 2 * i + 1 : i + half;
    const float q1 = q[i0], q2 = q[i1];
    q[i0] = q1 * c - q2 * s;
    q[i1] = q2 * c + q1 * s;
    const float k1 = k[i0], k2 = k[i1];
    k[i0] = k1 * c - k2 * s;
    k[i1] = k2 * c + k1 * s;
}

int launch_rope(float* qkv, const float* cos_sin, int B, int N, int H, int hd, long long ld, int pos0, hipStream_t s,
                int interleaved, int rot_heads) {
    const int Hr = rot_heads > 0 ? std::min(rot_heads, H) : H;
    const long long total = (long long)B * N * Hr * (hd / 2);
    HbmProf prof_(HK_ROPE, 16.0 * (double)B * N * Hr * hd, s);  // q and k parts: read + write
    hipLaunchKernelGGL(rope_kernel, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, s, qkv, cos_sin, B, N, H, hd, ld,
                       pos0, interleaved, Hr);
    QA_LAUNCH_CHECK();
    return QA_OK;
}

// ------------------------------------------------------------------------------------------------
// Strided [B, C, T] (element strides sb, sc, st) -> contiguous channel-last [B, T, C] through a 32x32 LDS tile.
__global__ __launch_bounds__(256) void to_channel_last_kernel(const float* __restrict__ x, long long sb, long long sc,
                                                              long long st, float* __restrict__ y, int C, int T) {
    __shared__ float tile[32][33];
    const int b = blockIdx.z, c0 = blockIdx.y * 32, t0 = blockIdx.x * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
    const bool t_fast = st <= sc;  // read along the contiguous axis of the source
    for (int k = ty; k < 32; k += 8) {
        const int c = t_fast ? c0 + k : c0 + tx;
        const int t = t_fast ? t0 + tx : t0 + k;
        if (c < C && t < T) tile[t - t0][c - c0] = x[b * sb + c * sc + t * st];
    }
    __syncthreads();
    for (int k = ty; k < 32; k += 8) {
        const int t = t0 + k, c = c0 + tx;
        if (c < C && t < T) y[((long long)b * T + t) * C + c] = tile[k][tx];
    }
}

int launch_to_channel_last(const float* x, long long sb, long long sc, long long st, float* y, int B, int C, int T,
                           hipStream_t s) {
    hipLaunchKernelGGL(to_channel_last_kernel, dim3((unsigned)ceil_div(T, 32), (unsigned)ceil_div(C, 32), B), dim3(256),
                       0, s, x, sb, sc, st, y, C, T);
    QA_LAUNCH_CHECK();
    return QA_OK;
}

// codes: library [n_vec = B*N, Q] -> reference [B, Q, N] (codec.py:173-174) and back (codec.py:179-180)
// lens (ragged calls, else null): entries at frames n >= lens[b] become -1, the dropped code, whatever the source holds there
__global__ void codes_to_bqn_kernel(const long long* __restrict__ src, long long* __restrict__ dst, int B, int N, int Q,
                                    const int* __restrict__ lens) {
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (long long)B * N * Q) return;
    const int n = (int)(gid % N);
    const int q = (int)((gid / N) % Q);
    const int b = (int)(gid / ((long long)N * Q));
    const long long v = src[((long long)b * N + n) * Q + q];
    dst[gid] = (lens && n >= lens[b]) ? -1 : v;
}
__global__ void codes_from_bqn_kernel(const long long* __restrict__ src, long long* __restrict__ dst, int B, int N,
                                      int Q, const int* __restrict__ lens) {
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (long long)B * N * Q) return;
    const int q = (int)(gid % Q);
    const int n = (int)((gid / Q) % N);
    const int b = (int)(gid / ((long long)N * Q));
    const long long v = src[((long long)b * Q + q) * N + n];
    dst[gid] = (lens && n >= lens[b]) ? -1 : v;
}
int launch_codes_to_bqn(const long long* src, long long* dst, int B, int N, int Q, hipStream_t s, const int* lens) {
    const long long total = (long long)B * N * Q;
    if (total == 0) return QA_OK;
    hipLaunchKernelGGL(codes_to_bqn_kernel, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, s, src, dst, B, N, Q, lens);
    QA_LAUNCH_CHECK();
    return QA_OK;
}
int launch_codes_from_bqn(const long long* src, long long* dst, int B, int N, int Q, hipStream_t s, const int* lens) {
    const long long total = (long long)B * N * Q;
    if (total == 0) return QA_OK;
    hipLaunchKernelGGL(codes_from_bqn_kernel, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, s, src, dst, B, N, Q, lens);
    QA_LAUNCH_CHECK();
    return QA_OK;
}

// The host integers of a call with per-row lengths: clip lengths, row counts, positions, offsets.  They travel BY
// VALUE in the launch, ROW_INTS_CHUNK of them per launch: written on the call's stream in stream order, no staging buffer whose lifetime a
// later call could cut short, and the host vector may be freed or overwritten on return.
struct IntChunk {
    int v[ROW_INTS_CHUNK];
};
__global__ __launch_bounds__(ROW_INTS_CHUNK) void row_ints_kernel(int* __restrict__ dst, const IntChunk a, int n) {
    if ((int)threadIdx.x < n) dst[threadIdx.x] = a.v[threadIdx.x];
}
int launch_row_ints(int* dst, const int* src, long long count, hipStream_t s) {
    for (long long i0 = 0; i0 < count; i0 += ROW_INTS_CHUNK) {
        IntChunk a{};
        const int n = (int)std::min<long long>(ROW_INTS_CHUNK, count - i0);
        std::copy(src + i0, src + i0 + n, a.v);
        hipLaunchKernelGGL(row_ints_kernel, dim3(1), dim3(ROW_INTS_CHUNK), 0, s, dst + i0, a, n);
        QA_LAUNCH_CHECK();
    }
    return QA_OK;
}
// key-padding mask of a ragged transformer call: valid[b, n] = n < lens[b] * mul
__global__ void len_mask_kernel(unsigned char* __restrict__ valid, int B, int N, const int* __restrict__ lens, int len_mul) {
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (long long)B * N) return;
    const int b = (int)(gid / N), n = (int)(gid - (long long)b * N);
    valid[gid] = n < lens[b] * len_mul ? 1 : 0;
}
int launch_len_mask(unsigned char* valid, int B, int N, ClipLens rl, hipStream_t s) {
    QA_REQUIRE(rl.n && rl.mul >= 1, "len_mask: no lengths");
    hipLaunchKernelGGL(len_mask_kernel, dim3((unsigned)ceil_div((long long)B * N, 256)), dim3(256), 0, s, valid, B, N, rl.n, rl.mul);
    QA_LAUNCH_CHECK();
    return QA_OK;
}

// ------------------------------------------------------------------------------------------------
// ISTFT head, step 1 (vq/heads.py:137-146): head output [rows, 2*nb] = (log-mag | phase) ->
// spectrum rows [rows, ldS] = (mag*cos p | mag*sin p | 0 pad), mag = min(exp(m), 100).
__global__ __launch_bounds__(256) void istft_spec_kernel(const float* __restrict__ y, float* __restrict__ S,
                                                         long long rows, int nb, int ldy, int ldS) {
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long total = rows * (long long)(ldS - nb);  // one thread per (row, column in [0, ldS - nb))
    if (gid >= total) return;
    const int w = ldS - nb;
    const int k = (int)(gid % w);
    const long long r = gid / w;
    float re = 0.f, im = 0.f;
    if (k < nb) {
        const float m = fminf(expf(y[r * ldy + k]), 100.f);
        float sn, cs;
        sincosf(y[r * ldy + nb + k], &sn, &cs);
        re = m * cs;
        im = m * sn;
        S[r * ldS + k] = re;
    }
    S[r * ldS + nb + k] = im;  // columns [nb, ldS): imaginary part, then zeros
}

int launch_istft_spec(const float* y, float* S, long long rows, int nb, int ldy, int ldS, hipStream_t s) {
    QA_REQUIRE(ldS >= 2 * nb, "istft_spec: ldS=%d < 2*nb=%d", ldS, 2 * nb);
    const long long total = rows * (long long)(ldS - nb);
    HbmProf prof_(HK_ISTFT_SPEC, 4.0 * (double)rows * (2.0 * nb + ldS), s);
    hipLaunchKernelGGL(istft_spec_kernel, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, s, y, S, rows, nb, ldy,
                       ldS);
    QA_LAUNCH_CHECK();
    return QA_OK;
}

// H-Codec 2.0 encoder front (HCodec-2.0/vq/codec_encoder.py:66-71): STFT rows (re | im) [rows, 2*nb] ->
// (log(max(|X|, 1e-5)) | angle(X) / pi | 0 pad) [rows, ldo]
__global__ __launch_bounds__(256) void stft_post_kernel(const float* __restrict__ ri, float* __restrict__ out, long long rows,
                                                        int nb, int ldi, int ldo) {
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int w = ldo - nb;
    if (gid >= rows * (long long)w) return;
    const int k = (int)(gid % w);
    const long long r = gid / w;
    float ph = 0.f;
    if (k < nb) {
        const float re = ri[r * ldi + k], im = ri[r * ldi + nb + k];
        out[r * ldo + k] = logf(fmaxf(hypotf(re, im), 1e-5f));
        ph = atan2f(im, re) / 3.14159265358979323846f;
    }
    out[r * ldo + nb + k] = ph;
}
int launch_stft_post(const float* ri, float* out, long long rows, int nb, int ldi, int ldo, hipStream_t s) {
    QA_REQUIRE(ldo >= 2 * nb, "stft_post: ldo=%d < 2*nb", ldo);
    const long long total = rows * (long long)(ldo - nb);
    HbmProf prof_(HK_STFT_POST, 4.0 * (double)rows * (2.0 * nb + ldo), s);
    hipLaunchKernelGGL(stft_post_kernel, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, s, ri, out, rows, nb, ldi, ldo);
    QA_LAUNCH_CHECK();
    return QA_OK;
}

// ISTFT step 3 (vq/spectral_ops.py:58-73): overlap-add of the windowed frames, trim (win-hop)/2 each side,
// divide by the folded hann^2 envelope.  frames [B, T, n_fft] (already multiplied by the window inside the
// inverse-DFT basis), out [B, T*hop].
__global__ __launch_bounds__(256) void istft_ola_kernel(const float* __restrict__ frames, const float* __restrict__ win,
                                                        float* __restrict__ out, int B, int T, int n_fft, int hop,
                                                        const int* __restrict__ lens, int len_mul) {
    const long long L = (long long)T * hop;
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (long long)B * L) return;
    const int b = (int)(gid / L);
    const long long n = gid - (long long)b * L;
    // ragged (launch-uniform test): the clip has Tb frames - later frames contribute nothing, the trim and the envelope are those of a
    // Tb-frame clip, and the samples behind Tb * hop are exactly zero
    const int Tb = lens ? min(lens[b] * len_mul, T) : T;
    if (n >= (long long)Tb * hop) {
        out[gid] = 0.f;
        return;
    }
    const long long p = n + (n_fft - hop) / 2;
    int t_hi = (int)(p / hop);
    if (t_hi > Tb - 1) t_hi = Tb - 1;
    long long lo = p - n_fft + 1;
    int t_lo = lo <= 0 ? 0 : (int)((lo + hop - 1) / hop);
    float acc = 0.f, env = 0.f;
    for (int t = t_lo; t <= t_hi; ++t) {
        const int k = (int)(p - (long long)t * hop);
        acc += frames[((long long)b * T + t) * n_fft + k];
        const float w = win[k];
        env = fmaf(w, w, env);
    }
    out[gid] = acc / env;
}

int launch_istft_ola(const float* frames, const float* win, float* out, int B, int T, int n_fft, int hop, hipStream_t s, ClipLens rl) {
    const long long total = (long long)B * T * hop;
    if (total == 0) return QA_OK;
    HbmProf prof_(HK_ISTFT_OLA, 4.0 * ((double)B * T * n_fft + (double)B * T * hop), s);
    hipLaunchKernelGGL(istft_ola_kernel, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, s, frames, win, out, B, T,
                       n_fft, hop, rl.n, rl.mul);
    QA_LAUNCH_CHECK();
    return QA_OK;
}

// ------------------------------------------------------------------------------------------------
// H-Codec 1.5 adaptive frame rate (HCodec-1.5/adaptive/modeling_flexicodec_new.py:828-921): cosine similarity of
// consecutive semantic frames, a new group wherever sim <= threshold, groups capped at max_tokens frames.
// One workgroup per batch item; the scan over T (<= a few hundred frames) is sequential in thread 0.
//   seg[b][t]   group index of frame t          start[b][g], len[b][g] (0 for g >= nseg[b])      nseg[b]
//   gmax        max over b of nseg (atomicMax; zeroed by the launcher)
// lens (per-clip calls, else null): clip b holds lens[b] of the T frames; norms, similarities and the scan stop there (the frames behind
// are never read), start / len behind nseg[b] are T / 0 as ever, and seg behind lens[b] is left unwritten: nothing reads it.
__global__ __launch_bounds__(256) void align_kernel(const float* __restrict__ sem, int T, int D, float thr, int max_tokens,
                                                    int* __restrict__ seg, int* __restrict__ start, int* __restrict__ len,
                                                    int* __restrict__ nseg, int* __restrict__ gmax, const int* __restrict__ lens) {
    extern __shared__ float sh[];  // [T] 1/max(norm, eps), then [T] sim
    float* inv = sh;
    float* sim = sh + T;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* x = sem + (long long)b * T * D;
    const int Tb = lens ? min(max(lens[b], 1), T) : T;  // the strides below stay T: the buffers are [B, T]
    for (int t = wave; t < Tb; t += 4) {
        float s = 0.f;
        for (int c = lane * 4; c < D; c += 256) {
            const float4 v = *reinterpret_cast<const float4*>(x + (long long)t * D + c);
            s += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
        }
        s = wave_sum(s);
        if (lane == 0) inv[t] = 1.f / fmaxf(sqrtf(s), 1e-8f);  // F.cosine_similarity: x / clamp_min(||x||, eps)
    }
    __syncthreads();
    for (int t = wave; t < Tb - 1; t += 4) {
        const float ia = inv[t], ib = inv[t + 1];
        float s = 0.f;
        for (int c = lane * 4; c < D; c += 256) {
            const float4 a = *reinterpret_cast<const float4*>(x + (long long)t * D + c);
            const float4 bb = *reinterpret_cast<const float4*>(x + (long long)(t + 1) * D + c);
            s += (a.x * ia) * (bb.x * ib) + (a.y * ia) * (bb.y * ib) + (a.z * ia) * (bb.z * ib) + (a.w * ia) * (bb.w * ib);
        }
        s = wave_sum(s);
        if (lane == 0) sim[t] = s;
    }
    __syncthreads();
    if (tid == 0) {
        int g = -1, in_seg = 0;
        for (int t = 0; t < Tb; ++t) {
            const bool new_group = (t == 0) || (sim[t - 1] <= thr);
            in_seg = new_group ? 0 : in_seg + 1;
            if (in_seg % max_tokens == 0) {
                ++g;
                start[(long long)b * T + g] = t;
                len[(long long)b * T + g] = 0;
            }
            seg[(long long)b * T + t] = g;
            len[(long long)b * T + g] += 1;
        }
        for (int k = g + 1; k < T; ++k) {
            start[(long long)b * T + k] = T;
            len[(long long)b * T + k] = 0;
        }
        nseg[b] = g + 1;
        atomicMax(gmax, g + 1);
    }
}

constexpr int ALIGN_MAX_T = 64 * 1024 / (2 * (int)sizeof(float));  // 8192
int launch_align(const float* sem, int B, int T, int D, float thr, int max_tokens, int* seg, int* start, int* len,
                 int* nseg, int* gmax, const int* lens, hipStream_t s) {
    QA_REQUIRE(D % 4 == 0 && T >= 1 && max_tokens >= 1, "align: bad shape");
    // the kernel keeps 2 * T floats of dynamic LDS (1 / norm and sim per frame); 64 KB is what a launch gets without raising the limit
    QA_REQUIRE(T <= ALIGN_MAX_T, "align: T=%d frames exceed %d (2 * T floats of LDS in 64 KB)", T, ALIGN_MAX_T);
    QA_HIP(hipMemsetAsync(gmax, 0, sizeof(int), s));
    hipLaunchKernelGGL(align_kernel, dim3(B), dim3(256), 2 * T * sizeof(float), s, sem, T, D, thr, max_tokens, seg, start, len,
                       nseg, gmax, lens);
    QA_LAUNCH_CHECK();
    return QA_OK;
}

// QueryTokenAggregator input (mimi/transformer.py:766-806): frames interleaved with one query token after each group;
// query = mean of the group's frames + query_embedding; padded groups (g >= nseg[b]) sit at the end and carry the bare
// query embedding.  out [B, T + G, D].
// lens (per-clip calls, else null): clip b holds lens[b] frames.  Its interleaved row is lens[b] + nseg[b] positions long, as for the clip
// alone; frames behind lens[b] are not scattered and padded groups carry no query.  The T - lens[b] + G - nseg[b] blocks that have nothing
// to place write exact zeros to the positions behind it, one each: those keys are masked (agg_key_mask), and a masked key's value still
// enters the attention as 0 * V, so it has to be finite.
__global__ __launch_bounds__(256) void agg_build_kernel(const float* __restrict__ feats, const int* __restrict__ seg,
                                                        const int* __restrict__ start, const int* __restrict__ len,
                                                        const int* __restrict__ nseg, const float* __restrict__ qemb,
                                                        float* __restrict__ out, int T, int G, int D, const int* __restrict__ lens) {
    const int b = blockIdx.y, p = blockIdx.x;  // p: source element, frames 0..T-1 then queries T..T+G-1
    const int S = T + G;
    float* ob = out + (long long)b * S * D;
    if (lens) {
        const int Tb = min(max(lens[b], 1), T), used = Tb + nseg[b];
        int zero_at = -1;
        if (p < T && p >= Tb) zero_at = used + (p - Tb);  // used .. used + T - Tb - 1
        if (p >= T && p - T >= nseg[b]) zero_at = p;      // T + nseg[b] .. S - 1, which is where the first range ends
        if (zero_at >= 0) {
            for (int c = threadIdx.x * 4; c < D; c += blockDim.x * 4)
                *reinterpret_cast<float4*>(ob + (long long)zero_at * D + c) = make_float4(0.f, 0.f, 0.f, 0.f);
            return;
        }
    }
    if (p < T) {
        const int dst = p + seg[(long long)b * T + p];
        for (int c = threadIdx.x * 4; c < D; c += blockDim.x * 4)
            *reinterpret_cast<float4*>(ob + (long long)dst * D + c) =
                *reinterpret_cast<const float4*>(feats + ((long long)b * T + p) * D + c);
        return;
    }
    const int g = p - T;
    if (g >= nseg[b]) {
        for (int c = threadIdx.x * 4; c < D; c += blockDim.x * 4)
            *reinterpret_cast<float4*>(ob + (long long)(T + g) * D + c) = *reinterpret_cast<const float4*>(qemb + c);
        return;
    }
    const int st = start[(long long)b * T + g], n = len[(long long)b * T + g];
    const int dst = st + n + g;
    const float inv = 1.f / (float)n;
    for (int c = threadIdx.x * 4; c < D; c += blockDim.x * 4) {
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int t = st; t < st + n; ++t) {
            const float4 v = *reinterpret_cast<const float4*>(feats + ((long long)b * T + t) * D + c);
            acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
        }
        const float4 q = *reinterpret_cast<const float4*>(qemb + c);
        acc.x = acc.x * inv + q.x; acc.y = acc.y * inv + q.y; acc.z = acc.z * inv + q.z; acc.w = acc.w * inv + q.w;
        *reinterpret_cast<float4*>(ob + (long long)dst * D + c) = acc;
    }
}
int launch_agg_build(const float* feats, const int* seg, const int* start, const int* len, const int* nseg, const float* qemb,
                     float* out, int B, int T, int G, int D, const int* lens, hipStream_t s) {
    QA_REQUIRE(D % 4 == 0, "agg_build: D=%d must be a multiple of 4", D);
    hipLaunchKernelGGL(agg_build_kernel, dim3(T + G, B), dim3(128), 0, s, feats, seg, start, len, nseg, qemb, out, T, G, D, lens);
    QA_LAUNCH_CHECK();
    return QA_OK;
}
// key-padding mask of the aggregators in a per-clip call: valid [B, T + G] bytes, 1 for the lens[b] + nseg[b] positions clip b's
// interleaved row holds.  One launch per encode, shared by both stacks and all their layers.
__global__ void agg_key_mask_kernel(unsigned char* __restrict__ valid, int B, int T, int G, const int* __restrict__ lens,
                                    const int* __restrict__ nseg) {
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int S = T + G;
    if (gid >= (long long)B * S) return;
    const int b = (int)(gid / S), j = (int)(gid - (long long)b * S);
    valid[gid] = j < min(max(lens[b], 1), T) + nseg[b] ? 1 : 0;
}
int launch_agg_key_mask(unsigned char* valid, int B, int T, int G, const int* lens, const int* nseg, hipStream_t s) {
    QA_REQUIRE(lens && nseg, "agg_key_mask: no lengths");
    hipLaunchKernelGGL(agg_key_mask_kernel, dim3((unsigned)ceil_div((long long)B * (T + G), 256)), dim3(256), 0, s, valid, B, T, G, lens, nseg);
    QA_LAUNCH_CHECK();
    return QA_OK;
}

// transformer output at the query positions -> [B, G, D], zero for padded groups (mimi/transformer.py:812-824)
__global__ __launch_bounds__(128) void agg_gather_kernel(const float* __restrict__ x, const int* __restrict__ start,
                                                         const int* __restrict__ len, const int* __restrict__ nseg,
                                                         float* __restrict__ out, int T, int G, int D) {
    const int b = blockIdx.y, g = blockIdx.x;
    const bool valid = g < nseg[b];
    const int src = valid ? start[(long long)b * T + g] + len[(long long)b * T + g] + g : 0;
    for (int c = threadIdx.x * 4; c < D; c += blockDim.x * 4) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (valid) v = *reinterpret_cast<const float4*>(x + ((long long)b * (T + G) + src) * D + c);
        *reinterpret_cast<float4*>(out + ((long long)b * G + g) * D + c) = v;
    }
}
int launch_agg_gather(const float* x, const int* start, const int* len, const int* nseg, float* out, int B, int T, int G,
                      int D, hipStream_t s) {
    QA_REQUIRE(D % 4 == 0, "agg_gather: D=%d must be a multiple of 4", D);
    hipLaunchKernelGGL(agg_gather_kernel, dim3(G, B), dim3(128), 0, s, x, start, len, nseg, out, T, G, D);
    QA_LAUNCH_CHECK();
    return QA_OK;
}

// The last aggregator layer needs only the query rows past its key / value projection (QA_AGG_LAST_ROWS): the query rows of x
// [B, T + G, D] and the q columns of their qkv rows [B, T + G, 3 D] -> compact xq, qq [B, G, D], with agg_gather's indexing.  A padded
// group (g >= nseg[b]) reads row 0 of its clip, a valid row whose result agg_zero_padded overwrites.
__global__ __launch_bounds__(128) void agg_query_rows_kernel(const float* __restrict__ x, const float* __restrict__ qkv,
                                                             const int* __restrict__ start, const int* __restrict__ len,
                                                             const int* __restrict__ nseg, float* __restrict__ xq,
                                                             float* __restrict__ qq, int T, int G, int D) {
    const int b = blockIdx.y, g = blockIdx.x;
    const int src = g < nseg[b] ? start[(long long)b * T + g] + len[(long long)b * T + g] + g : 0;
    const long long row = (long long)b * (T + G) + src, dst = ((long long)b * G + g) * D;
    for (int c = threadIdx.x * 4; c < D; c += blockDim.x * 4) {
        *reinterpret_cast<float4*>(xq + dst + c) = *reinterpret_cast<const float4*>(x + row * D + c);
        *reinterpret_cast<float4*>(qq + dst + c) = *reinterpret_cast<const float4*>(qkv + row * 3 * D + c);
    }
}
int launch_agg_query_rows(const float* x, const float* qkv, const int* start, const int* len, const int* nseg, float* xq, float* qq,
                          int B, int T, int G, int D, hipStream_t s) {
    QA_REQUIRE(D % 4 == 0, "agg_query_rows: D=%d must be a multiple of 4", D);
    hipLaunchKernelGGL(agg_query_rows_kernel, dim3(G, B), dim3(128), 0, s, x, qkv, start, len, nseg, xq, qq, T, G, D);
    QA_LAUNCH_CHECK();
    return QA_OK;
}
// out [B, G, D]: zero the padded groups, as agg_gather writes them
__global__ __launch_bounds__(128) void agg_zero_padded_kernel(const int* __restrict__ nseg, float* __restrict__ out, int G, int D) {
    const int b = blockIdx.y, g = blockIdx.x;
    if (g < nseg[b]) return;
    for (int c = threadIdx.x * 4; c < D; c += blockDim.x * 4)
        *reinterpret_cast<float4*>(out + ((long long)b * G + g) * D + c) = make_float4(0.f, 0.f, 0.f, 0.f);
}
int launch_agg_zero_padded(const int* nseg, float* out, int B, int G, int D, hipStream_t s) {
    QA_REQUIRE(D % 4 == 0, "agg_zero_padded: D=%d must be a multiple of 4", D);
    hipLaunchKernelGGL(agg_zero_padded_kernel, dim3(G, B), dim3(128), 0, s, nseg, out, G, D);
    QA_LAUNCH_CHECK();
    return QA_OK;
}

// library indices [B*G, Q] -> reference layout [B, Q, G] with the group length injected:
// code' = (len - 1) * K + code (codec_adaptive.py:68-73; len = 0 for padded groups gives code - K, as in the reference)
// pad_minus1 (per-clip calls): a padded group is written as -1 instead, the length-0 entry that is also the library's dropped code
__global__ void codes_inject_kernel(const long long* __restrict__ idx, const int* __restrict__ len, long long* __restrict__ dst,
                                    int B, int T, int G, int Q, int K, int pad_minus1) {
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (long long)B * Q * G) return;
    const int g = (int)(gid % G);
    const int q = (int)((gid / G) % Q);
    const int b = (int)(gid / ((long long)G * Q));
    const int n = len[(long long)b * T + g];
    const long long v = (long long)(n - 1) * K + idx[((long long)b * G + g) * Q + q];
    dst[gid] = (pad_minus1 && n == 0) ? -1 : v;
}
int launch_codes_inject(const long long* idx, const int* len, long long* dst, int B, int T, int G, int Q, int K, bool pad_minus1,
                        hipStream_t s) {
    QA_REQUIRE(G <= T, "codes_inject: G=%d groups exceed the T=%d rows of len", G, T);
    const long long total = (long long)B * Q * G;
    hipLaunchKernelGGL(codes_inject_kernel, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, s, idx, len, dst, B, T, G, Q, K,
                       pad_minus1 ? 1 : 0);
    QA_LAUNCH_CHECK();
    return QA_OK;
}

__device__ __forceinline__ long long floordiv_ll(long long a, long long b) {
    long long q = a / b;
    if ((a % b != 0) && ((a < 0) != (b < 0))) --q;
    return q;
}

// total frames per item from length-injected codes: len = floor(code / K) + 1 of quantizer 0 (codec_adaptive.py:75-80)
__global__ void adaptive_frames_kernel(const long long* __restrict__ codes, int B, int Q, int G, int K, int* __restrict__ totals,
                                       int* __restrict__ tmax) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    int tot = 0;
    for (int g = 0; g < G; ++g) {
        const long long l = floordiv_ll(codes[((long long)b * Q) * G + g], K) + 1;
        tot += l > 0 ? (int)l : 0;
    }
    totals[b] = tot;
    atomicMax(tmax, tot);
}
int launch_adaptive_frames(const long long* codes, int B, int Q, int G, int K, int* totals, int* tmax, hipStream_t s) {
    QA_HIP(hipMemsetAsync(tmax, 0, sizeof(int), s));
    hipLaunchKernelGGL(adaptive_frames_kernel, dim3((unsigned)ceil_div(B, 64)), dim3(64), 0, s, codes, B, Q, G, K, totals, tmax);
    QA_LAUNCH_CHECK();
    return QA_OK;
}

// token_lengths [B, G] = floor(code / K) + 1 of quantizer 0 of length-injected codes [B, Q, G] (codec_adaptive.py:145: the alignment
// matrices' row sums, which is what encode injects)
__global__ void token_lengths_kernel(const long long* __restrict__ codes, long long* __restrict__ out, int B, int Q, int G, int K) {
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (long long)B * G) return;
    const int g = (int)(gid % G), b = (int)(gid / G);
    out[gid] = floordiv_ll(codes[((long long)b * Q) * G + g], K) + 1;
}
int launch_token_lengths(const long long* codes, long long* out, int B, int Q, int G, int K, hipStream_t s) {
    const long long total = (long long)B * G;
    if (total == 0) return QA_OK;
    hipLaunchKernelGGL(token_lengths_kernel, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, s, codes, out, B, Q, G, K);
    QA_LAUNCH_CHECK();
    return QA_OK;
}

// _deaggregate_features_from_token_lengths on index tensors (modeling_flexicodec_new.py:1007-1041, codec_adaptive.py:184-189):
// codes [B, Q, G] (length-injected) -> plain indices [B*T, Q], each group repeated len times, rows past an item's total = 0.
// Lengths come from `len_codes` (the reference ends up using the semantic stream's lengths for both streams).
// cap (per-clip calls, else null): item b de-aggregates at most cap[b] frames; the rows behind hold index 0 like every row past a total.
__global__ __launch_bounds__(64) void deaggregate_kernel(const long long* __restrict__ codes, const long long* __restrict__ len_codes,
                                                          long long* __restrict__ out, int Q, int G, int T, int K,
                                                          const int* __restrict__ cap) {
    const int b = blockIdx.x;
    const int Tb = cap ? min(max(cap[b], 0), T) : T;
    __shared__ int s_start[1024];
    __shared__ int s_n;
    if (threadIdx.x == 0) {
        int pos = 0;
        for (int g = 0; g < G && g < 1024; ++g) {
            s_start[g] = pos;
            const long long l = floordiv_ll(len_codes[((long long)b * Q) * G + g], K) + 1;
            pos += l > 0 ? (int)l : 0;
        }
        s_n = pos;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < T * Q; i += blockDim.x) out[((long long)b * T) * Q + i] = 0;
    __syncthreads();
    for (int g = threadIdx.x; g < G; g += blockDim.x) {
        const int st = s_start[g];
        const int en = (g + 1 < G) ? s_start[g + 1] : s_n;
        for (int q = 0; q < Q; ++q) {
            const long long c = codes[((long long)b * Q + q) * G + g];
            long long plain = c % K;
            if (plain < 0) plain += K;  // python modulo
            for (int t = st; t < en && t < Tb; ++t) out[((long long)b * T + t) * Q + q] = plain;
        }
    }
}
int launch_deaggregate(const long long* codes, const long long* len_codes, long long* out, int B, int Q, int G, int T, int K,
                       const int* cap, hipStream_t s) {
    QA_REQUIRE(G <= 1024, "deaggregate: %d groups per item exceed 1024", G);
    hipLaunchKernelGGL(deaggregate_kernel, dim3(B), dim3(64), 0, s, codes, len_codes, out, Q, G, T, K, cap);
    QA_LAUNCH_CHECK();
    return QA_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// number of codes outside [0, limit): what F.embedding would refuse (Codec.decode, vq/codec.py:183-184)
__global__ __launch_bounds__(256) void codes_check_kernel(const long long* __restrict__ codes, long long n, long long lo, long long limit,
                                                          unsigned long long* __restrict__ bad) {
    unsigned long long local = 0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const long long c = codes[i];
        local += (c < lo || c >= limit) ? 1ull : 0ull;
    }
    local += __shfl_xor(local, 32, 64);
    local += __shfl_xor(local, 16, 64);
    local += __shfl_xor(local, 8, 64);
    local += __shfl_xor(local, 4, 64);
    local += __shfl_xor(local, 2, 64);
    local += __shfl_xor(local, 1, 64);
    if ((threadIdx.x & 63) == 0 && local) atomicAdd(bad, local);  // integer count: order-independent
}
int launch_codes_check(const long long* codes, long long n, long long limit, unsigned long long* bad, hipStream_t s) {
    QA_HIP(hipMemsetAsync(bad, 0, sizeof(unsigned long long), s));
    return launch_codes_count(codes, n, 0, limit, bad, s);
}
// *bad += number of entries outside [lo, limit): no memset, no copy, no synchronisation (qa_codes_check_async)
int launch_codes_count(const long long* codes, long long n, long long lo, long long limit, unsigned long long* bad, hipStream_t s) {
    if (n <= 0) return QA_OK;
    const unsigned grid = (unsigned)std::min<long long>(ceil_div(n, 256), 1024);
    hipLaunchKernelGGL(codes_check_kernel, dim3(grid), dim3(256), 0, s, codes, n, lo, limit, bad);
    QA_LAUNCH_CHECK();
    return QA_OK;
}

// torchaudio.functional.resample's polyphase FIR (transforms.Resample, HCodec-2.0/audio_tokenizer.py:44,51):
//   out[b, q * new + i] = sum_j kernel[i][j] * padded[b, q * orig + j],  padded = wav with `width` zeros in front and
//   width + orig behind, kernel [new][2 * width + orig]; the output is cut to ceil(new * T / orig) samples.
// HBM-bound (one read of the waveform, 1/3 of it written for 48 -> 16 kHz): one thread per output sample, taps from LDS.
// lens [B] (device) or null: a per-clip call - row b holds lens[b] of its T samples.  Samples behind them read as
// zero and are never loaded, so an output is the same fmaf chain as on the clip alone; outputs behind ceil(new * lens[b] / orig) are
// written as exactly zero (a zero-filled row would carry the filter's ringing there).
__global__ __launch_bounds__(256) void resample_kernel(const float* __restrict__ wav, const float* __restrict__ taps, float* __restrict__ out,
                                                       long long T, long long T_out, int orig, int nw, int width, int ktaps,
                                                       int use_lds, const int* __restrict__ lens) {
    extern __shared__ float s_taps[];
    if (use_lds) {  // small filter banks (48 -> 16 kHz: 1 x 41 taps) live in LDS; large ones (44.1 -> 16 kHz: 160 x 475) stay in L2
        for (int i = threadIdx.x; i < nw * ktaps; i += 256) s_taps[i] = taps[i];
        __syncthreads();
    }
    const long long o = (long long)blockIdx.x * 256 + threadIdx.x;
    if (o >= T_out) return;
    const int b = blockIdx.y;
    const long long q = o / nw;
    const int ph = (int)(o - q * nw);
    const float* x = wav + (long long)b * T;
    const float* k = (use_lds ? s_taps : taps) + ph * ktaps;
    const long long base = q * orig - width;
    long long len = T;
    if (lens) {  // launch-uniform
        len = min((long long)lens[b], T);
        if (o >= (len * nw + orig - 1) / orig) {
            out[(long long)b * T_out + o] = 0.f;
            return;
        }
    }
    float acc = 0.f;
    for (int j = 0; j < ktaps; ++j) {
        const long long t = base + j;
        const float v = (t >= 0 && t < len) ? x[t] : 0.f;
        acc = fmaf(k[j], v, acc);
    }
    out[(long long)b * T_out + o] = acc;
}
int launch_resample(const float* wav, const float* taps, float* out, int B, long long T, long long T_out, int orig, int nw, int width,
                    int ktaps, hipStream_t s, const int* lens) {
    const size_t bytes = (size_t)nw * ktaps * sizeof(float);
    const int use_lds = bytes <= 48 * 1024;
    hipLaunchKernelGGL(resample_kernel, dim3((unsigned)ceil_div(T_out, 256), (unsigned)B), dim3(256), use_lds ? bytes : 0, s, wav, taps, out, T,
                       T_out, orig, nw, width, ktaps, use_lds, lens);
    QA_LAUNCH_CHECK();
    return QA_OK;
}

// ------------------------------------------------------------------------------------------------
// RingKVCache.complete() write (mimi/transformer.py:243-250): cache[:, (pos0 + t) % cap] = k[:, t]
__global__ __launch_bounds__(256) void ring_append_kernel(const float* __restrict__ k, const float* __restrict__ v, long long ld,
                                                          float* __restrict__ kc, float* __restrict__ vc, int B, int T, int d,
                                                          int cap, int pos0) {
    const int d4 = d >> 2;
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (long long)B * T * d4) return;
    const int c = (int)(gid % d4) * 4;
    const long long row = gid / d4;
    const int b = (int)(row / T), t = (int)(row - (long long)b * T);
    const long long dst = ((long long)b * cap + (pos0 + t) % cap) * d + c;
    *reinterpret_cast<float4*>(kc + dst) = *reinterpret_cast<const float4*>(k + row * ld + c);
    *reinterpret_cast<float4*>(vc + dst) = *reinterpret_cast<const float4*>(v + row * ld + c);
}

int launch_ring_append(const float* k, const float* v, long long ld, float* kc, float* vc, int B, int T, int d, int cap, int pos0,
                       hipStream_t s) {
    QA_REQUIRE(d % 4 == 0 && ld % 4 == 0 && T >= 1 && T <= cap && pos0 >= 0, "ring_append: T=%d cap=%d d=%d (a chunk must fit the ring)", T, cap, d);
    const long long total = (long long)B * T * (d / 4);
    hipLaunchKernelGGL(ring_append_kernel, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, s, k, v, ld, kc, vc, B, T, d, cap, pos0);
    QA_LAUNCH_CHECK();
    return QA_OK;
}

}  // namespace qa

// ------------------------------------------------------------------------------------------------
// test hooks (not part of the public header): the float kernels above alone on caller-provided device buffers, one launcher call each
// (tests/test_ew_kernels_gpu.py).  lens: device int32 [B] or null, with len_mul the ClipLens of the launchers.
extern "C" int qa_debug_rownorm(int mode, const float* x, const float* w, const float* b, float* y, long long rows, int C, float eps,
                                void* stream) {
    return mode == 0 ? qa::launch_rmsnorm(x, w, y, rows, C, eps, static_cast<hipStream_t>(stream))
                     : qa::launch_layernorm(x, w, b, y, rows, C, eps, static_cast<hipStream_t>(stream));
}
extern "C" int qa_debug_dwconv(const float* x, const float* w_kc, const float* bias, const float* lnw, const float* lnb, float* y, int B,
                               int T, int C, int ksize, float eps, int pad_left, const int* lens, int len_mul, void* stream) {
    return qa::launch_dwconv(x, w_kc, bias, lnw, lnb, y, B, T, C, ksize, eps, static_cast<hipStream_t>(stream), pad_left,
                             qa::ClipLens{lens, len_mul});
}
extern "C" long long qa_debug_groupnorm_scratch_bytes(int B, int T, int G) { return (long long)qa::groupnorm_scratch_bytes(B, T, G); }
extern "C" int qa_debug_groupnorm(const float* x, const float* w, const float* bias, float* y, void* scratch, int B, int T, int C, int G,
                                  float eps, int swish, const int* lens, int len_mul, void* stream) {
    return qa::launch_groupnorm(x, w, bias, y, static_cast<double*>(scratch), B, T, C, G, eps, swish, static_cast<hipStream_t>(stream),
                                qa::ClipLens{lens, len_mul});
}
extern "C" int qa_debug_conv_in(const float* x, const float* w_kc, const float* bias, float* y, int B, int T, int Cout, int ksize,
                                int pad_left, const int* lens, int len_mul, void* stream) {
    return qa::launch_conv_in(x, w_kc, bias, y, B, T, Cout, ksize, static_cast<hipStream_t>(stream), pad_left, qa::ClipLens{lens, len_mul});
}
extern "C" int qa_debug_rope(float* qkv, const float* cos_sin, int B, int N, int H, int hd, long long ld, int pos0, int interleaved,
                             int rot_heads, void* stream) {
    return qa::launch_rope(qkv, cos_sin, B, N, H, hd, ld, pos0, static_cast<hipStream_t>(stream), interleaved, rot_heads);
}
extern "C" int qa_debug_istft_spec(const float* y, float* S, long long rows, int nb, int ldy, int ldS, void* stream) {
    return qa::launch_istft_spec(y, S, rows, nb, ldy, ldS, static_cast<hipStream_t>(stream));
}
extern "C" int qa_debug_stft_post(const float* ri, float* out, long long rows, int nb, int ldi, int ldo, void* stream) {
    return qa::launch_stft_post(ri, out, rows, nb, ldi, ldo, static_cast<hipStream_t>(stream));
}
extern "C" int qa_debug_istft_ola(const float* frames, const float* win, float* out, int B, int T, int n_fft, int hop, const int* lens,
                                  int len_mul, void* stream) {
    return qa::launch_istft_ola(frames, win, out, B, T, n_fft, hop, static_cast<hipStream_t>(stream), qa::ClipLens{lens, len_mul});
}
// host_src: HOST int32 [count]; dst: device int32 [count] (tests/test_row_ints_gpu.py)
extern "C" int qa_debug_row_ints(int* dst, const int* host_src, long long count, void* stream) {
    return qa::launch_row_ints(dst, host_src, count, static_cast<hipStream_t>(stream));
}
extern "C" int qa_debug_to_channel_last(const float* x, long long sb, long long sc, long long st, float* y, int B, int C, int T,
                                        void* stream) {
    return qa::launch_to_channel_last(x, sb, sc, st, y, B, C, T, static_cast<hipStream_t>(stream));
}

// the adaptive-rate, code-layout, mask and ring kernels, the same way (tests/test_agg_kernels_gpu.py): int32 / int64 / byte device buffers
extern "C" int qa_debug_align(const float* sem, int B, int T, int D, float thr, int max_tokens, int* seg, int* start, int* len, int* nseg,
                              int* gmax, const int* lens, void* stream) {
    return qa::launch_align(sem, B, T, D, thr, max_tokens, seg, start, len, nseg, gmax, lens, static_cast<hipStream_t>(stream));
}
extern "C" int qa_debug_agg_build(const float* feats, const int* seg, const int* start, const int* len, const int* nseg, const float* qemb,
                                  float* out, int B, int T, int G, int D, const int* lens, void* stream) {
    return qa::launch_agg_build(feats, seg, start, len, nseg, qemb, out, B, T, G, D, lens, static_cast<hipStream_t>(stream));
}
extern "C" int qa_debug_agg_key_mask(unsigned char* valid, int B, int T, int G, const int* lens, const int* nseg, void* stream) {
    return qa::launch_agg_key_mask(valid, B, T, G, lens, nseg, static_cast<hipStream_t>(stream));
}
extern "C" int qa_debug_agg_gather(const float* x, const int* start, const int* len, const int* nseg, float* out, int B, int T, int G, int D,
                                   void* stream) {
    return qa::launch_agg_gather(x, start, len, nseg, out, B, T, G, D, static_cast<hipStream_t>(stream));
}
extern "C" int qa_debug_agg_query_rows(const float* x, const float* qkv, const int* start, const int* len, const int* nseg, float* xq,
                                       float* qq, int B, int T, int G, int D, void* stream) {
    return qa::launch_agg_query_rows(x, qkv, start, len, nseg, xq, qq, B, T, G, D, static_cast<hipStream_t>(stream));
}
extern "C" int qa_debug_agg_zero_padded(const int* nseg, float* out, int B, int G, int D, void* stream) {
    return qa::launch_agg_zero_padded(nseg, out, B, G, D, static_cast<hipStream_t>(stream));
}
extern "C" int qa_debug_codes_inject(const long long* idx, const int* len, long long* dst, int B, int T, int G, int Q, int K, int pad_minus1,
                                     void* stream) {
    return qa::launch_codes_inject(idx, len, dst, B, T, G, Q, K, pad_minus1 != 0, static_cast<hipStream_t>(stream));
}
extern "C" int qa_debug_adaptive_frames(const long long* codes, int B, int Q, int G, int K, int* totals, int* tmax, void* stream) {
    return qa::launch_adaptive_frames(codes, B, Q, G, K, totals, tmax, static_cast<hipStream_t>(stream));
}
extern "C" int qa_debug_token_lengths(const long long* codes, long long* out, int B, int Q, int G, int K, void* stream) {
    return qa::launch_token_lengths(codes, out, B, Q, G, K, static_cast<hipStream_t>(stream));
}
extern "C" int qa_debug_deaggregate(const long long* codes, const long long* len_codes, long long* out, int B, int Q, int G, int T, int K,
                                    const int* cap, void* stream) {
    return qa::launch_deaggregate(codes, len_codes, out, B, Q, G, T, K, cap, static_cast<hipStream_t>(stream));
}
// dir 0: library [B * N, Q] -> reference [B, Q, N]; dir 1: back
extern "C" int qa_debug_codes_bqn(int dir, const long long* src, long long* dst, int B, int N, int Q, const int* lens, void* stream) {
    return dir == 0 ? qa::launch_codes_to_bqn(src, dst, B, N, Q, static_cast<hipStream_t>(stream), lens)
                    : qa::launch_codes_from_bqn(src, dst, B, N, Q, static_cast<hipStream_t>(stream), lens);
}
extern "C" int qa_debug_len_mask(unsigned char* valid, int B, int N, const int* lens, int len_mul, void* stream) {
    return qa::launch_len_mask(valid, B, N, qa::ClipLens{lens, len_mul}, static_cast<hipStream_t>(stream));
}
extern "C" int qa_debug_ring_append(const float* k, const float* v, long long ld, float* kc, float* vc, int B, int T, int d, int cap, int pos0,
                                    void* stream) {
    return qa::launch_ring_append(k, v, ld, kc, vc, B, T, d, cap, pos0, static_cast<hipStream_t>(stream));
}
