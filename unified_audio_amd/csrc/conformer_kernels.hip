// conformer_kernels.hip - the byte-bound kernels of the UniSE condition encoder (QuarkAudio-UniSE/model/llm/conformer.py) and of the
// log-mel front that feeds it (model/model.py:53-79).
#include "kernels.h"

namespace qa {

// ------------------------------------------------------------------------------------------------
// ConvolutionModule's middle (conformer.py:345-358, eval mode) in one pass:
//   GLU over channels -> depthwise Conv1d(k odd <= 31, "same" zero padding, bias) -> BatchNorm1d (running statistics folded into
//   scale / shift at load) -> SiLU
// u [B, T, 2C] is the first 1x1 convolution's output (value half, then gate half), y [B, T, C].
// A workgroup owns 64 output frames x 64 channels: the GLU values of the 64 + 30 frames it needs go to LDS once (lane = channel, so a
// frame's 64 channels are one 256-byte row in memory and one conflict-free row in LDS), then wave g produces frames 16 g .. 16 g + 15 of
// every channel from registers.  The filter is held as 31 centred taps (a shorter kernel has zeros outside), so every index of the
// inner loops is a compile-time constant: no scratch, and an output's sum runs over the taps in one fixed order wherever its tile lies.
// rows (device int [B], nullable): item b holds rows[b] of the T frames.  Its "same" zero padding then starts at
// frame rows[b], the frames behind are stored as 0 and never read, and a tile that lies wholly behind stores its zeros and loads nothing.
constexpr int GDW_K = 31, GDW_H = GDW_K / 2, GDW_TT = 64, GDW_PER = 16, GDW_CT = 64;
__global__ __launch_bounds__(256) void glu_dwconv_bn_silu_kernel(const float* __restrict__ u, const float* __restrict__ w31,
                                                                 const float* __restrict__ bias, const float* __restrict__ scale,
                                                                 const float* __restrict__ shift, float* __restrict__ y, int T, int C,
                                                                 const int* __restrict__ rows) {
    __shared__ float xs[(GDW_TT + GDW_K - 1) * GDW_CT];
    const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int b = blockIdx.z, c = blockIdx.y * GDW_CT + lane, t0 = blockIdx.x * GDW_TT;
    const bool cok = c < C;
    const int Tb = rows ? rows[b] : T;  // one wave-uniform load per workgroup
    if (t0 >= Tb) {                     // workgroup-uniform: the whole tile lies behind the item's frames
        for (int o = 0; o < GDW_PER; ++o) {
            const int t = t0 + g * GDW_PER + o;
            if (cok && t < T) y[((long long)b * T + t) * C + c] = 0.f;
        }
        return;
    }
    const int cc = cok ? c : C - 1;  // clamped: every load below is unconditional, out-of-range lanes are dropped at the store
    const float* ub = u + (long long)b * T * 2 * C;
    for (int f = g; f < GDW_TT + GDW_K - 1; f += 4) {
        const int t = t0 - GDW_H + f;
        const int tc = min(max(t, 0), Tb - 1);
        const float a = ub[(long long)tc * 2 * C + cc], gt = ub[(long long)tc * 2 * C + C + cc];
        xs[f * GDW_CT + lane] = (t >= 0 && t < Tb) ? a * sigmoid_f(gt) : 0.f;
    }
    float wr[GDW_K];
#pragma unroll
    for (int j = 0; j < GDW_K; ++j) wr[j] = w31[j * C + cc];
    const float bi = bias[cc], sc = scale[cc], sh = shift[cc];
    __syncthreads();
    float xr[GDW_PER + GDW_K - 1];
#pragma unroll
    for (int i = 0; i < GDW_PER + GDW_K - 1; ++i) xr[i] = xs[(g * GDW_PER + i) * GDW_CT + lane];
#pragma unroll
    for (int o = 0; o < GDW_PER; ++o) {
        float acc = bi;
#pragma unroll
        for (int j = 0; j < GDW_K; ++j) acc = fmaf(xr[o + j], wr[j], acc);
        const int t = t0 + g * GDW_PER + o;
        if (cok && t < T) y[((long long)b * T + t) * C + c] = t < Tb ? silu_f(fmaf(acc, sc, sh)) : 0.f;
    }
}

int launch_glu_dwconv_bn_silu(const float* u, const float* w31, const float* bias, const float* scale, const float* shift, float* y, int B,
                              int T, int C, hipStream_t s, const int* rows) {
    QA_REQUIRE(B > 0 && T > 0 && C > 0 && B < 65536, "glu_dwconv: B=%d T=%d C=%d", B, T, C);
    dim3 grid((unsigned)ceil_div(T, GDW_TT), (unsigned)ceil_div(C, GDW_CT), (unsigned)B);
    HbmProf prof_(HK_GLU_DWCONV, 12.0 * (double)B * T * C, s);  // algorithmic: both halves of u in, y out
    hipLaunchKernelGGL(glu_dwconv_bn_silu_kernel, grid, dim3(256), 0, s, u, w31, bias, scale, shift, y, T, C, rows);
    QA_LAUNCH_CHECK();
    return QA_OK;
}

// ------------------------------------------------------------------------------------------------
// The attention module's tail (conformer.py:183-185 and the residual of :432): rows of padded positions are zeroed AFTER to_out (bias
// included), then added to the residual stream.  y <- valid ? y : 0 (kept for the test tap), x += y.  valid == nullptr: every row counts.
__global__ __launch_bounds__(256) void masked_add_kernel(float* __restrict__ x, float* __restrict__ y, const unsigned char* __restrict__ valid,
                                                         long long rows, int C4) {
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= rows * C4) return;
    const long long row = gid / C4;
    float4 v = reinterpret_cast<float4*>(y)[gid];
    if (valid && !valid[row]) {
        v = make_float4(0.f, 0.f, 0.f, 0.f);
        reinterpret_cast<float4*>(y)[gid] = v;
    }
    float4 r = reinterpret_cast<float4*>(x)[gid];
    r.x += v.x; r.y += v.y; r.z += v.z; r.w += v.w;
    reinterpret_cast<float4*>(x)[gid] = r;
}
int launch_masked_add(float* x, float* y, const unsigned char* valid, long long rows, int C, hipStream_t s) {
    QA_REQUIRE(C % 4 == 0 && rows > 0, "masked_add: rows=%lld C=%d", rows, C);
    hipLaunchKernelGGL(masked_add_kernel, dim3((unsigned)ceil_div(rows * (C / 4), 256)), dim3(256), 0, s, x, y, valid, rows, C / 4);
    QA_LAUNCH_CHECK();
    return QA_OK;
}

// valid keys per batch item of a [B, T] byte mask -> counts [B] (one wave per item, fixed order)
__global__ __launch_bounds__(64) void mask_count_kernel(const unsigned char* __restrict__ valid, int T, int* __restrict__ counts) {
    const int b = blockIdx.x, lane = threadIdx.x;
    float n = 0.f;
    for (int t = lane; t < T; t += 64) n += valid[(long long)b * T + t] ? 1.f : 0.f;
    n = wave_sum(n);
    if (lane == 0) counts[b] = (int)n;
}
int launch_mask_count(const unsigned char* valid, int B, int T, int* counts, hipStream_t s) {
    hipLaunchKernelGGL(mask_count_kernel, dim3((unsigned)B), dim3(64), 0, s, valid, T, counts);
    QA_LAUNCH_CHECK();
    return QA_OK;
}

// ------------------------------------------------------------------------------------------------
// Model.stft_logmel's framing (model.py:61-62): the signal zero-padded by `pad` samples in front and up to n_out samples behind, as the
// [B, frames + 1, hop] image whose rows t and t + 1 are frame t of a window of 2 hop samples (the k = 2 convolution of the DFT GEMM).
// rows (device int [B], nullable): row b holds rows[b] of the n samples; the samples behind count as that zero padding and are never read.
__global__ __launch_bounds__(256) void logmel_frames_kernel(const float* __restrict__ wav, long long n, int pad, long long n_out,
                                                            float* __restrict__ P, const int* __restrict__ rows) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_out) return;
    const int b = blockIdx.y;
    const long long nb = rows ? rows[b] : n;
    const long long k = i - pad;
    const long long kc = k < 0 ? 0 : (k >= nb ? nb - 1 : k);
    const float v = wav[(long long)b * n + kc];
    P[(long long)b * n_out + i] = (k >= 0 && k < nb) ? v : 0.f;
}
int launch_logmel_frames(const float* wav, int B, long long n, int pad, long long n_out, float* P, hipStream_t s, const int* rows) {
    QA_REQUIRE(B > 0 && B < 65536 && n > 0 && n_out > 0, "logmel_frames: B=%d n=%lld", B, n);
    hipLaunchKernelGGL(logmel_frames_kernel, dim3((unsigned)ceil_div(n_out, 256), (unsigned)B), dim3(256), 0, s, wav, n, pad, n_out, P, rows);
    QA_LAUNCH_CHECK();
    return QA_OK;
}

// y = log(x + eps), in place (model.py:78).  frames (device int [n / (F C)], nullable): x is [., F, C] and item b holds frames[b] of its F
// rows; the rows behind are written as 0 in the same pass (what they held is not read).
__global__ __launch_bounds__(256) void log_eps_kernel(float* __restrict__ x, long long n, float eps, const int* __restrict__ frames, int F,
                                                      int C) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (frames) {
        const long long row = i / C;
        if ((int)(row % F) >= frames[row / F]) {
            x[i] = 0.f;
            return;
        }
    }
    x[i] = logf(x[i] + eps);
}
int launch_log_eps(float* x, long long n, float eps, hipStream_t s, const int* frames, int F, int C) {
    if (n <= 0) return QA_OK;
    QA_REQUIRE(!frames || (F > 0 && C > 0 && n % ((long long)F * C) == 0), "log_eps: n=%lld is no multiple of F=%d x C=%d", n, F, C);
    hipLaunchKernelGGL(log_eps_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, s, x, n, eps, frames, F, C);
    QA_LAUNCH_CHECK();
    return QA_OK;
}

// [mix_sos, cond] prompt rows (llm.py:133-134,307-308): x [B, T + 1, d].  off (device int [B], nullable): row b holds T + off[b] condition
// frames (off[b] <= 0, the decode kernels' position offset); the positions behind its prompt are written as 0 and their frames never read.
__global__ __launch_bounds__(256) void cond_prompt_kernel(float* __restrict__ x, const float* __restrict__ sos, const float* __restrict__ cond,
                                                          int T, int d, long long total, const int* __restrict__ off) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int ch = (int)(i % d);
    const long long row = i / d;
    const int t = (int)(row % (T + 1));
    const long long b = row / (T + 1);
    if (off && t > T + off[b]) {
        x[i] = 0.f;
        return;
    }
    x[i] = t == 0 ? sos[ch] : cond[(b * T + (t - 1)) * d + ch];
}
int launch_cond_prompt(float* x, const float* sos, const float* cond, int B, int T, int d, hipStream_t s, const int* off) {
    const long long total = (long long)B * (T + 1) * d;
    hipLaunchKernelGGL(cond_prompt_kernel, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, s, x, sos, cond, T, d, total, off);
    QA_LAUNCH_CHECK();
    return QA_OK;
}

}  // namespace qa

// ------------------------------------------------------------------------------------------------
// test hooks (not part of the public header): one launcher each on caller-provided device buffers, the launcher's arguments in its
// order and the stream last (tests/test_front_kernels_gpu.py)
extern "C" int qa_debug_glu_dwconv_bn_silu(const float* u, const float* w31, const float* bias, const float* scale, const float* shift,
                                           float* y, int B, int T, int C, void* stream) {
    return qa::launch_glu_dwconv_bn_silu(u, w31, bias, scale, shift, y, B, T, C, static_cast<hipStream_t>(stream));
}
// rows: device int [B], the items' frame counts (1 .. T each), or null
extern "C" int qa_debug_glu_dwconv_bn_silu_rows(const float* u, const float* w31, const float* bias, const float* scale, const float* shift,
                                                float* y, int B, int T, int C, const int* rows, void* stream) {
    return qa::launch_glu_dwconv_bn_silu(u, w31, bias, scale, shift, y, B, T, C, static_cast<hipStream_t>(stream), rows);
}
extern "C" int qa_debug_masked_add(float* x, float* y, const unsigned char* valid, long long rows, int C, void* stream) {
    return qa::launch_masked_add(x, y, valid, rows, C, static_cast<hipStream_t>(stream));
}
extern "C" int qa_debug_mask_count(const unsigned char* valid, int B, int T, int* counts, void* stream) {
    return qa::launch_mask_count(valid, B, T, counts, static_cast<hipStream_t>(stream));
}
extern "C" int qa_debug_logmel_frames(const float* wav, int B, long long n, int pad, long long n_out, float* P, void* stream) {
    return qa::launch_logmel_frames(wav, B, n, pad, n_out, P, static_cast<hipStream_t>(stream));
}
extern "C" int qa_debug_log_eps(float* x, long long n, float eps, void* stream) {
    return qa::launch_log_eps(x, n, eps, static_cast<hipStream_t>(stream));
}
extern "C" int qa_debug_cond_prompt(float* x, const float* sos, const float* cond, int B, int T, int d, void* stream) {
    return qa::launch_cond_prompt(x, sos, cond, B, T, d, static_cast<hipStream_t>(stream));
}
