// bicodec_kernels.hip - the pieces of BiCodec.detokenize (QuarkAudio-UniSE/model/bicodec/bicodec.py:182-199) and BiCodec.tokenize
// (bicodec.py:151-180) that are not plain contractions: token look-ups into folded tables, AdaLayerNorm, the d-vector broadcast add;
// the feature normalisation, the mel framing / magnitude, the Res2 chain, SE, perceiver glue, FSQ.  Everything with a large contraction
// (linears, k7 / dilated k7 convolutions, the polyphase ConvTranspose1d, the DFT and the mel filterbank) runs on conv_gemm.hip.
#include <algorithm>
#include <cmath>

#include "kernels.h"

namespace qa {

// out[i, :] = table[clamp(tok[i]), :]   (FactorizedVectorQuantize.detokenize with out_project folded into the table)
// lens [n / T] (device) or null: row i = b * T + t of a per-clip call with t >= lens[b] is padding - its token is
// not loaded, the table is not indexed, and the row is exact zeros (finite: the zero-padding taps of the convolutions multiply it by 0)
__global__ __launch_bounds__(256) void gather_rows_kernel(const long long* __restrict__ tok, const float* __restrict__ table, float* __restrict__ out,
                                                          long long n, int V, int D, int T, const int* __restrict__ lens) {
    const int d4 = D >> 2;
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= n * d4) return;
    const long long i = gid / d4;
    const int c = (int)(gid - i * d4) * 4;
    if (lens) {  // launch-uniform
        const long long b = i / T;
        if ((int)(i - b * T) >= lens[b]) {
            *reinterpret_cast<float4*>(out + i * D + c) = make_float4(0.f, 0.f, 0.f, 0.f);
            return;
        }
    }
    long long t = tok[i];
    t = t < 0 ? 0 : (t >= V ? V - 1 : t);  // memory safety only; callers validate (qa_codes_check)
    *reinterpret_cast<float4*>(out + i * D + c) = *reinterpret_cast<const float4*>(table + t * D + c);
}
int launch_gather_rows(const long long* tok, const float* table, float* out, long long n, int V, int D, hipStream_t s, int T, const int* lens) {
    QA_REQUIRE(D % 4 == 0, "gather_rows: D=%d must be a multiple of 4", D);
    QA_REQUIRE(!lens || (T >= 1 && n % T == 0), "gather_rows: per-clip lengths need rows = B * T (rows %lld, T %d)", n, T);
    if (n <= 0) return QA_OK;
    hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)ceil_div(n * (D / 4), 256)), dim3(256), 0, s, tok, table, out, n, V, D, T, lens);
    QA_LAUNCH_CHECK();
    return QA_OK;
}

// The tails of a per-clip call, each behind the last writer of its output: tok[b, n] = -1 for n >= lens[b] (the
// semantic tokens behind a clip's last frame) and x[b, t] = 0.0f for t >= lens[b] * mul (the waveform behind a clip's last sample).
// Nothing in front of a clip's end is touched.
__global__ __launch_bounds__(256) void tokens_fill_behind_kernel(long long* __restrict__ tok, long long total, int N, const int* __restrict__ lens) {
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= total) return;
    const long long b = gid / N;
    if ((int)(gid - b * N) >= lens[b]) tok[gid] = -1;
}
int launch_tokens_fill_behind(long long* tok, int B, int N, const int* lens, hipStream_t s) {
    QA_REQUIRE(lens && B > 0 && N > 0, "tokens_fill_behind: [%d, %d] without lengths", B, N);
    const long long total = (long long)B * N;
    hipLaunchKernelGGL(tokens_fill_behind_kernel, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, s, tok, total, N, lens);
    QA_LAUNCH_CHECK();
    return QA_OK;
}
__global__ __launch_bounds__(256) void zero_behind_kernel(float* __restrict__ x, long long total, long long T, const int* __restrict__ lens, int mul) {
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= total) return;
    const long long b = gid / T;
    if (gid - b * T >= (long long)lens[b] * mul) x[gid] = 0.f;
}
int launch_zero_behind(float* x, int B, long long T, ClipLens rl, hipStream_t s) {
    QA_REQUIRE(rl.n && rl.mul >= 1 && B > 0 && T > 0, "zero_behind: [%d, %lld] without lengths", B, T);
    const long long total = (long long)B * T;
    hipLaunchKernelGGL(zero_behind_kernel, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, s, x, total, T, rl.n, rl.mul);
    QA_LAUNCH_CHECK();
    return QA_OK;
}

// SpeakerEncoder.detokenize up to the flatten (speaker_encoder.py:111-114): zq [B, n, L] = table[tok[b, n]] (FSQ codes x project_out
// folded), then zq.transpose(1, 2).reshape(B, -1): out[b, c * N + n] = table[tok[b, n]][c]
__global__ __launch_bounds__(256) void gather_global_kernel(const long long* __restrict__ tok, const float* __restrict__ table,
                                                            float* __restrict__ out, int B, int N, int V, int L) {
    const int gid = blockIdx.x * 256 + threadIdx.x;
    if (gid >= B * N * L) return;
    const int n = gid % N, c = (gid / N) % L, b = gid / (N * L);
    long long t = tok[b * N + n];
    t = t < 0 ? 0 : (t >= V ? V - 1 : t);
    out[gid] = table[t * L + c];
}
int launch_gather_global(const long long* tok, const float* table, float* out, int B, int N, int V, int L, hipStream_t s) {
    hipLaunchKernelGGL(gather_global_kernel, dim3((unsigned)ceil_div((long long)B * N * L, 256)), dim3(256), 0, s, tok, table, out, B, N, V, L);
    QA_LAUNCH_CHECK();
    return QA_OK;
}

// AdaLayerNorm (blocks/vocos.py:113-136): y = LayerNorm(x, no affine, eps) * scale[b, :] + shift[b, :]; one wave per row of C channels
__global__ __launch_bounds__(256) void adaln_kernel(const float* __restrict__ x, const float* __restrict__ scale, const float* __restrict__ shift,
                                                    long long ld_cond, float* __restrict__ y, long long rows, int T, int C, float eps) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* xr = x + row * C;
    float s = 0.f, ss = 0.f;
    for (int c = lane * 4; c < C; c += 256) {
        const float4 t = *reinterpret_cast<const float4*>(xr + c);
        s += (t.x + t.y) + (t.z + t.w);
    }
    s = wave_sum(s);
    const float mean = s / C;
    for (int c = lane * 4; c < C; c += 256) {
        const float4 t = *reinterpret_cast<const float4*>(xr + c);
        const float a = t.x - mean, b = t.y - mean, cc = t.z - mean, d = t.w - mean;
        ss += (a * a + b * b) + (cc * cc + d * d);
    }
    ss = wave_sum(ss);
    const float rstd = rsqrtf(ss / C + eps);
    const long long b = row / T;
    const float* sc = scale + b * ld_cond;
    const float* sh = shift + b * ld_cond;
    for (int c = lane * 4; c < C; c += 256) {
        const float4 t = *reinterpret_cast<const float4*>(xr + c);
        const float4 g = *reinterpret_cast<const float4*>(sc + c);
        const float4 h = *reinterpret_cast<const float4*>(sh + c);
        float4 o;
        o.x = (t.x - mean) * rstd * g.x + h.x;
        o.y = (t.y - mean) * rstd * g.y + h.y;
        o.z = (t.z - mean) * rstd * g.z + h.z;
        o.w = (t.w - mean) * rstd * g.w + h.w;
        *reinterpret_cast<float4*>(y + row * C + c) = o;
    }
}
int launch_adaln(const float* x, const float* scale, const float* shift, long long ld_cond, float* y, int B, int T, int C, float eps,
                 hipStream_t s) {
    QA_REQUIRE(C % 4 == 0 && ld_cond % 4 == 0, "adaln: C=%d / ld=%lld must be multiples of 4", C, ld_cond);
    const long long rows = (long long)B * T;
    hipLaunchKernelGGL(adaln_kernel, dim3((unsigned)ceil_div(rows, 4)), dim3(256), 0, s, x, scale, shift, ld_cond, y, rows, T, C, eps);
    QA_LAUNCH_CHECK();
    return QA_OK;
}

// x[b, t, :] += v[b, :]   (bicodec.py:196: x = x + d_vector.unsqueeze(-1))
__global__ __launch_bounds__(256) void add_rowvec_kernel(float* __restrict__ x, const float* __restrict__ v, long long n4, int T, int C) {
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= n4) return;
    const int c4 = C >> 2;
    const long long row = gid / c4;
    const int c = (int)(gid - row * c4) * 4;
    float4 t = *reinterpret_cast<float4*>(x + row * C + c);
    const float4 a = *reinterpret_cast<const float4*>(v + (row / T) * C + c);
    t.x += a.x; t.y += a.y; t.z += a.z; t.w += a.w;
    *reinterpret_cast<float4*>(x + row * C + c) = t;
}
int launch_add_rowvec(float* x, const float* v, int B, int T, int C, hipStream_t s) {
    QA_REQUIRE(C % 4 == 0, "add_rowvec: C=%d must be a multiple of 4", C);
    const long long n4 = (long long)B * T * (C / 4);
    hipLaunchKernelGGL(add_rowvec_kernel, dim3((unsigned)ceil_div(n4, 256)), dim3(256), 0, s, x, v, n4, T, C);
    QA_LAUNCH_CHECK();
    return QA_OK;
}

// ---------------------------------------------------------------- encoder side (BiCodec.get_semantic_tokens, bicodec.py:168-173)

// Wav2Vec2FeatureExtractor(do_normalize=True) on one unpadded row (feature_extraction_wav2vec2.py zero_mean_unit_var_norm):
// y = (x - mean) / sqrt(var + eps), population variance.  One workgroup per row; the two moments are accumulated in fp64 (the
// reference does this in numpy float32 on the host: fp64 sums are at least as close to the exact value as its pairwise fp32 sums).
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double block_sum_d(double v, double* red) {  // 256 threads, red[4]; every thread gets the total
    v = wave_sum_d(v);
    __syncthreads();  // red[] may still be read by the previous call
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}
// one row: the moments over its first `len` samples, (x - mean) / sqrt(var + eps) there and exact zeros from `len` to T
__device__ __forceinline__ void wav_normalize_row(const float* xr, float* yr, long long len, long long T, float eps, double* red) {
    double s = 0.0;
    for (long long t = threadIdx.x; t < len; t += 256) s += (double)xr[t];
    const double mean = block_sum_d(s, red) / (double)len;
    double ss = 0.0;
    for (long long t = threadIdx.x; t < len; t += 256) {
        const double d = (double)xr[t] - mean;
        ss += d * d;
    }
    const double var = block_sum_d(ss, red) / (double)len;
    const float m = (float)mean, inv = (float)(1.0 / sqrt(var + (double)eps));
    for (long long t = threadIdx.x; t < len; t += 256) yr[t] = (xr[t] - m) * inv;
    for (long long t = len + threadIdx.x; t < T; t += 256) yr[t] = 0.f;
}
__global__ __launch_bounds__(256) void wav_normalize_kernel(const float* x, float* y, long long T, float eps) {
    __shared__ double red[4];
    wav_normalize_row(x + (long long)blockIdx.x * T, y + (long long)blockIdx.x * T, T, T, eps, red);
}
// Per-clip lengths: row b is normalised over its own lens.n[b] samples - the same loops, so the same summation
// order, as the kernel above on a [1, lens.n[b]] row - and nothing behind them is read.  The lengths ride BY VALUE in the launch, as
// row_ints_kernel's do (ew.hip): this entry point has no handle that could own a device array.
constexpr int WAV_LENS_CHUNK = 256;
struct WavLensArg {
    long long n[WAV_LENS_CHUNK];
};
__global__ __launch_bounds__(256) void wav_normalize_ragged_kernel(const float* x, float* y, long long T, float eps, const WavLensArg lens) {
    __shared__ double red[4];
    wav_normalize_row(x + (long long)blockIdx.x * T, y + (long long)blockIdx.x * T, lens.n[blockIdx.x], T, eps, red);
}
int launch_wav_normalize(const float* x, float* y, int B, long long T, float eps, hipStream_t s, const long long* lens_host) {
    QA_REQUIRE(B > 0 && T > 0, "wav_normalize: [%d, %lld]", B, T);
    if (!lens_host) {
        hipLaunchKernelGGL(wav_normalize_kernel, dim3((unsigned)B), dim3(256), 0, s, x, y, T, eps);
        QA_LAUNCH_CHECK();
        return QA_OK;
    }
    for (int b0 = 0; b0 < B; b0 += WAV_LENS_CHUNK) {
        WavLensArg a{};
        const int m = std::min(WAV_LENS_CHUNK, B - b0);
        for (int i = 0; i < m; ++i) {
            QA_REQUIRE(lens_host[b0 + i] >= 1 && lens_host[b0 + i] <= T, "wav_normalize: row %d holds %lld of %lld samples", b0 + i, lens_host[b0 + i], T);
            a.n[i] = lens_host[b0 + i];
        }
        hipLaunchKernelGGL(wav_normalize_ragged_kernel, dim3((unsigned)m), dim3(256), 0, s, x + (long long)b0 * T, y + (long long)b0 * T, T, eps, a);
        QA_LAUNCH_CHECK();
    }
    return QA_OK;
}

// F.normalize(x, dim=-1) on rows of D <= 64 floats (the 8-wide in_project latents in front of the codebook search,
// factorized_vector_quantize.py:178-179): y = x / max(||x||, 1e-12).  One wave per row, lane c owns channel c.
__global__ __launch_bounds__(256) void l2norm_rows_kernel(const float* __restrict__ x, float* __restrict__ y, long long rows, int D) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float v = lane < D ? x[row * D + lane] : 0.f;
    const float n = sqrtf(wave_sum(v * v));
    if (lane < D) y[row * D + lane] = v / fmaxf(n, 1e-12f);
}
int launch_l2norm_rows(const float* x, float* y, long long rows, int D, hipStream_t s) {
    QA_REQUIRE(D >= 1 && D <= 64, "l2norm_rows: D=%d must be 1 .. 64", D);
    if (rows <= 0) return QA_OK;
    hipLaunchKernelGGL(l2norm_rows_kernel, dim3((unsigned)ceil_div(rows, 4)), dim3(256), 0, s, x, y, rows, D);
    QA_LAUNCH_CHECK();
    return QA_OK;
}

// ---------------------------------------------------------------- encoder side: global tokens (BiCodec.get_global_tokens, bicodec.py:174-178)

// The mel front as a framed signal for an implicit-GEMM DFT.  P[b, i] = clip(i - hop) for i in [0, (n_frames + 1) * hop), where clip is
// the reference clip of ref_len samples, reflect-padded by torch.stft(center=True) (k < 0 -> -k, k >= ref_len -> 2 (ref_len - 1) - k),
// and clip[k] = wav[k % T] is BiCodecTokenizer.get_ref_clip's tile-then-truncate as index arithmetic.  Viewed as [B, n_frames + 1, hop],
// frame t of a window of 2 hop samples centred on t * hop is rows t and t + 1: a k = 2 convolution over hop channels.
// lens [B] (device) or null: the clip of row b is its first lens[b] samples (a per-clip call) - it tiles by its own
// length, and nothing behind it is read.
__global__ __launch_bounds__(256) void mel_frames_kernel(const float* __restrict__ wav, long long T, long long ref_len, int hop,
                                                         long long n_out, float* __restrict__ P, const int* __restrict__ lens) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_out) return;
    const int b = blockIdx.y;
    long long k = i - hop;
    k = k < 0 ? -k : (k >= ref_len ? 2 * (ref_len - 1) - k : k);
    const long long len = lens ? (long long)lens[b] : T;  // launch-uniform
    P[(long long)b * n_out + i] = wav[(long long)b * T + k % len];
}
int launch_mel_frames(const float* wav, int B, long long T, long long ref_len, int hop, int n_frames, float* P, hipStream_t s, const int* lens) {
    QA_REQUIRE(T > 0 && ref_len > hop && B > 0, "mel_frames: T=%lld ref_len=%lld hop=%d", T, ref_len, hop);
    const long long n_out = (long long)(n_frames + 1) * hop;
    hipLaunchKernelGGL(mel_frames_kernel, dim3((unsigned)ceil_div(n_out, 256), (unsigned)B), dim3(256), 0, s, wav, T, ref_len, hop, n_out, P, lens);
    QA_LAUNCH_CHECK();
    return QA_OK;
}

// |X_k| = sqrt(re^2 + im^2) of the DFT GEMM's [re (nbp) | im (nbp)] rows into [rows, ldm] with zeros from bin nb on (the K padding of
// the filterbank GEMM)
__global__ __launch_bounds__(256) void spec_mag_kernel(const float* __restrict__ ri, int nbp, int nb, float* __restrict__ mag, int ldm, long long n) {
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= n) return;
    const long long row = g / ldm;
    const int k = (int)(g - row * ldm);
    float v = 0.f;
    if (k < nb) {
        const float re = ri[row * 2 * nbp + k], im = ri[row * 2 * nbp + nbp + k];
        v = sqrtf(re * re + im * im);
    }
    mag[g] = v;
}
int launch_spec_mag(const float* ri, int nbp, int nb, float* mag, int ldm, long long rows, hipStream_t s) {
    const long long n = rows * ldm;
    if (n <= 0) return QA_OK;
    hipLaunchKernelGGL(spec_mag_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, s, ri, nbp, nb, mag, ldm, n);
    QA_LAUNCH_CHECK();
    return QA_OK;
}

// Res2Conv1dReluBn (ecapa_tdnn.py Res2Conv1dReluBn, scale 8): 7 DEPENDENT width-W dilated k = 3 convolutions, each
// sp_i = BN(ReLU(conv_i(sp_{i-1} + x_i))) (sp_0 = conv_0(x_0)), the last split passed through.  One launch per block: a workgroup owns a
// time tile of TT = R - 2 H output frames and recomputes a halo of H = 7 d frames on each side (every step widens the receptive field by
// d), so the chain never leaves LDS.  Frames outside [0, T) are the convolutions' zero padding and are zeroed after every step; frames
// near the region's edge go wrong (missing neighbours) but only inside the halo.  LDS: the running split [R][W] and step i's weights
// [3][W][W] (transposed: consecutive output channels consecutive, conflict-free), <= 80 KB.  Thread (c = tid % 64, g = tid / 64) owns
// output channel c of the frames g, g + 16, ...; the split's 4-channel groups are wave-uniform (broadcast) float4 reads.  16 waves per
// workgroup: at B = 16 the launch has only ~80 workgroups, so the latency of the LDS reads is hidden by waves of the same workgroup
// (256 threads per workgroup measured 570 us per launch at 16 x 6 s).
constexpr int RES2_R = 128;
constexpr int RES2_THREADS = 1024;
__global__ __launch_bounds__(RES2_THREADS) void res2_chain_kernel(const float* __restrict__ x, float* __restrict__ y, const float* __restrict__ wt,
                                                         const float* __restrict__ bst, int T, int C, int W, int d, int TT) {
    __shared__ __attribute__((aligned(16))) float sp[RES2_R * 64];
    __shared__ __attribute__((aligned(16))) float sw[3 * 64 * 64];
    constexpr int NG = RES2_THREADS / 64, NF = RES2_R / NG;
    const int tid = threadIdx.x, c = tid & 63, g = tid >> 6;
    const int b = blockIdx.y, H = 7 * d;
    const int t0 = blockIdx.x * TT, rb = t0 - H;
    const float* xb = x + (long long)b * T * C;
    float* yb = y + (long long)b * T * C;
    for (int e = tid; e < RES2_R * W; e += RES2_THREADS) {
        const int f = e / W, cc = e - f * W, t = rb + f;
        sp[f * W + cc] = (t >= 0 && t < T) ? xb[(long long)t * C + cc] : 0.f;
    }
    for (int i = 0; i < 7; ++i) {
        const float* wi = wt + (long long)i * 3 * W * W;
        for (int e = tid; e < 3 * W * W; e += RES2_THREADS) sw[e] = wi[e];
        __syncthreads();
        float acc[NF];
#pragma unroll
        for (int k = 0; k < NF; ++k) acc[k] = 0.f;
        if (c < W) {
            for (int j = 0; j < 3; ++j) {
                const int off = (j - 1) * d;
                for (int ci = 0; ci < W; ci += 4) {
                    const float w0 = sw[(j * W + ci) * W + c], w1 = sw[(j * W + ci + 1) * W + c];
                    const float w2 = sw[(j * W + ci + 2) * W + c], w3 = sw[(j * W + ci + 3) * W + c];
#pragma unroll
                    for (int k = 0; k < NF; ++k) {
                        const int fs = g + NG * k + off;
                        if (fs >= 0 && fs < RES2_R) {
                            const float4 v = *reinterpret_cast<const float4*>(sp + fs * W + ci);
                            acc[k] = fmaf(w0, v.x, acc[k]);
                            acc[k] = fmaf(w1, v.y, acc[k]);
                            acc[k] = fmaf(w2, v.z, acc[k]);
                            acc[k] = fmaf(w3, v.w, acc[k]);
                        }
                    }
                }
            }
        }
        __syncthreads();  // every read of sp (and sw) for step i is done
        if (c < W) {
            const float bias = bst[(i * 3 + 0) * W + c], sc = bst[(i * 3 + 1) * W + c], sh = bst[(i * 3 + 2) * W + c];
#pragma unroll
            for (int k = 0; k < NF; ++k) {
                const int f = g + NG * k, t = rb + f;
                float v = 0.f;
                if (t >= 0 && t < T) {
                    v = fmaxf(acc[k] + bias, 0.f) * sc + sh;  // BN(ReLU(conv)): per-channel affine after the ReLU
                    if (f >= H && f < H + TT) yb[(long long)t * C + i * W + c] = v;
                    if (i < 6) v += xb[(long long)t * C + (i + 1) * W + c];
                }
                sp[f * W + c] = v;
            }
        }
    }
    for (int e = tid; e < TT * W; e += RES2_THREADS) {  // the last split passes through
        const int f = e / W, cc = e - f * W, t = t0 + f;
        if (t < T) yb[(long long)t * C + 7 * W + cc] = xb[(long long)t * C + 7 * W + cc];
    }
}
int launch_res2_chain(const float* x, float* y, const float* wt, const float* bst, int B, int T, int C, int d, hipStream_t s) {
    const int W = C / 8;
    QA_REQUIRE(C % 8 == 0 && W % 4 == 0 && W <= 64, "res2_chain: C=%d (width C / 8 must be a multiple of 4, at most 64)", C);
    QA_REQUIRE(d >= 1 && 14 * d < RES2_R, "res2_chain: dilation %d", d);
    const int TT = RES2_R - 14 * d;
    hipLaunchKernelGGL(res2_chain_kernel, dim3((unsigned)ceil_div(T, TT), (unsigned)B), dim3(RES2_THREADS), 0, s, x, y, wt, bst, T, C, W, d, TT);
    QA_LAUNCH_CHECK();
    return QA_OK;
}

// SE_Connect + the block's residual (ecapa_tdnn.py SE_Connect, SE_Res2Block.forward): out = x + y * sigmoid(W2 relu(W1 mean_t(y) + b1) + b2).
// Two launches, neither of which moves a [T, C] tensor more than once: se_gate_kernel (one workgroup per batch item: time mean, the two
// small FCs -> gate [B, C]) and se_apply_kernel (the scaled residual sum, float4 over the whole batch, written with row stride ldo: the
// 3 block outputs are the channel slices of the concatenation the final 1x1 convolution reads).  w1t [C][Hd] and w2t [Hd][C] are the
// Linear weights transposed at load, so that the threads of a wave read consecutive addresses in the FC loops.
constexpr int SE_THREADS = 1024;
__global__ __launch_bounds__(SE_THREADS) void se_gate_kernel(const float* __restrict__ y, const float* __restrict__ w1, const float* __restrict__ b1,
                                                             const float* __restrict__ w2, const float* __restrict__ b2, float* __restrict__ gate,
                                                             int T, int C, int Hd) {
    extern __shared__ float sm[];
    float* part = sm;             // [SE_THREADS]: partial time sums, thread (c, q) sums frames q, q + Q, ...
    float* mean = sm + SE_THREADS;  // [C]
    float* hid = mean + C;        // [Hd]
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* yb = y + (long long)b * T * C;
    const int Q = SE_THREADS / C;  // C divides SE_THREADS (launcher)
    {
        const int c = tid % C, q = tid / C;
        float a = 0.f;
        for (int t = q; t < T; t += Q) a += yb[(long long)t * C + c];
        part[tid] = a;
    }
    __syncthreads();
    for (int c = tid; c < C; c += SE_THREADS) {
        float a = 0.f;
        for (int q = 0; q < Q; ++q) a += part[q * C + c];
        mean[c] = a / (float)T;
    }
    __syncthreads();
    for (int o = tid; o < Hd; o += SE_THREADS) {
        float a = 0.f;
#pragma unroll 8
        for (int c = 0; c < C; ++c) a = fmaf(w1[(long long)c * Hd + o], mean[c], a);
        hid[o] = fmaxf(a + b1[o], 0.f);
    }
    __syncthreads();
    for (int c = tid; c < C; c += SE_THREADS) {
        float a = 0.f;
#pragma unroll 8
        for (int o = 0; o < Hd; ++o) a = fmaf(w2[(long long)o * C + c], hid[o], a);
        gate[(long long)b * C + c] = 1.f / (1.f + expf(-(a + b2[c])));
    }
}
__global__ __launch_bounds__(256) void se_apply_kernel(const float* __restrict__ x, long long ldx, const float* __restrict__ y,
                                                       const float* __restrict__ gate, float* __restrict__ out, long long ldo, int T, int C4,
                                                       long long n4) {
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= n4) return;
    const long long row = g / C4;  // (b, t)
    const int c = (int)(g - row * C4) * 4;
    const long long b = row / T;
    const float4 xv = *reinterpret_cast<const float4*>(x + row * ldx + c);
    const float4 yv = *reinterpret_cast<const float4*>(y + row * 4 * C4 + c);
    const float4 gv = *reinterpret_cast<const float4*>(gate + b * 4 * C4 + c);
    float4 o;
    o.x = xv.x + yv.x * gv.x; o.y = xv.y + yv.y * gv.y; o.z = xv.z + yv.z * gv.z; o.w = xv.w + yv.w * gv.w;
    *reinterpret_cast<float4*>(out + row * ldo + c) = o;
}
int launch_se_residual(const float* x, long long ldx, const float* y, const float* w1, const float* b1, const float* w2, const float* b2,
                       float* gate, float* out, long long ldo, int B, int T, int C, int Hd, hipStream_t s) {
    QA_REQUIRE(C % 4 == 0 && C <= SE_THREADS && SE_THREADS % C == 0 && ldx % 4 == 0 && ldo % 4 == 0,
               "se_residual: C=%d must divide %d (and strides be multiples of 4)", C, SE_THREADS);
    const size_t lds = sizeof(float) * (size_t)(SE_THREADS + C + Hd);
    QA_REQUIRE(lds <= 64 * 1024, "se_residual: C=%d, bottleneck %d", C, Hd);
    hipLaunchKernelGGL(se_gate_kernel, dim3((unsigned)B), dim3(SE_THREADS), lds, s, y, w1, b1, w2, b2, gate, T, C, Hd);
    QA_LAUNCH_CHECK();
    const long long n4 = (long long)B * T * (C / 4);
    hipLaunchKernelGGL(se_apply_kernel, dim3((unsigned)ceil_div(n4, 256)), dim3(256), 0, s, x, ldx, y, gate, out, ldo, T, C / 4, n4);
    QA_LAUNCH_CHECK();
    return QA_OK;
}

// Perceiver context cat(latents, x) per batch item: ctx[b, 0:n_lat] = lat[b] (or the learned latents, broadcast, when lat_ld == 0),
// ctx[b, n_lat:] = x[b] (skipped when x == nullptr: the context rows only change in their latent part between layers)
__global__ __launch_bounds__(256) void perceiver_ctx_kernel(const float* __restrict__ lat, long long lat_b, const float* __restrict__ x, float* __restrict__ ctx,
                                                            int n_lat, int T, int D, long long n) {
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= n) return;
    const int rows = x ? n_lat + T : n_lat;
    const long long b = g / ((long long)rows * D);
    const long long r = (g / D) % rows;
    const int c = (int)(g % D);
    const float v = r < n_lat ? lat[b * lat_b + r * D + c] : x[(b * T + (r - n_lat)) * D + c];
    ctx[(b * (n_lat + T) + r) * D + c] = v;
}
int launch_perceiver_ctx(const float* lat, long long lat_b, const float* x, float* ctx, int B, int n_lat, int T, int D, hipStream_t s) {
    const long long n = (long long)B * (x ? n_lat + T : n_lat) * D;
    hipLaunchKernelGGL(perceiver_ctx_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, s, lat, lat_b, x, ctx, n_lat, T, D, n);
    QA_LAUNCH_CHECK();
    return QA_OK;
}

// GEGLU (perceiver_encoder.py GEGLU): h [rows, 2F] = [x | gate] -> out[rows, ldo] = gelu_erf(gate) * x, zeros in columns F .. ldo - 1
// (the K padding of the following Linear, whose F = 341 is odd)
__global__ __launch_bounds__(256) void geglu_kernel(const float* __restrict__ h, int F, float* __restrict__ out, int ldo, long long n) {
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= n) return;
    const long long row = g / ldo;
    const int c = (int)(g - row * ldo);
    float v = 0.f;
    if (c < F) {
        const float a = h[row * 2 * F + c], z = h[row * 2 * F + F + c];
        v = 0.5f * z * (1.f + erff(z * 0.70710678118654752f)) * a;
    }
    out[g] = v;
}
int launch_geglu(const float* h, int F, float* out, int ldo, long long rows, hipStream_t s) {
    const long long n = rows * ldo;
    hipLaunchKernelGGL(geglu_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, s, h, F, out, ldo, n);
    QA_LAUNCH_CHECK();
    return QA_OK;
}

// PerceiverResampler's final RMSNorm (perceiver_encoder.py RMSNorm): F.normalize(x) * sqrt(D) * gamma - an L2 norm clamped at 1e-12,
// not a mean square.  One wave per row, D <= 256.
__global__ __launch_bounds__(256) void l2norm_scale_kernel(const float* __restrict__ x, const float* __restrict__ gamma, float* __restrict__ y,
                                                           long long rows, int D, float scale) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    float v[4], ss = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int c = lane + 64 * k;
        v[k] = c < D ? x[row * D + c] : 0.f;
        ss = fmaf(v[k], v[k], ss);
    }
    const float n = fmaxf(sqrtf(wave_sum(ss)), 1e-12f);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int c = lane + 64 * k;
        if (c < D) y[row * D + c] = v[k] / n * scale * gamma[c];
    }
}
int launch_l2norm_scale(const float* x, const float* gamma, float* y, long long rows, int D, float scale, hipStream_t s) {
    QA_REQUIRE(D >= 1 && D <= 256, "l2norm_scale: D=%d", D);
    hipLaunchKernelGGL(l2norm_scale_kernel, dim3((unsigned)ceil_div(rows, 4)), dim3(256), 0, s, x, gamma, y, rows, D, scale);
    QA_LAUNCH_CHECK();
    return QA_OK;
}

// ResidualFSQ.forward with one quantizer (residual_fsq.py:158+, finite_scalar_quantization.py:126-160): z = project_in(x) (scale 1),
// bound(z) = tanh(z + atanh(offset / half_l)) half_l - offset, round half to even (rintf: torch.round), index = sum (q + L // 2) basis.
// One wave per token (the projection's D products spread over the lanes, one wave_sum per level); `bounded` [rows, nl] is the test tap
// (may be null).  The bound is evaluated in double on the fp32 z, with double constants, and rounded once: for an even L the result is
// a difference of two values near offset = 0.5 (L = 2: tanh(z + 3.8) * 0.5005 - 0.5 = 4e-4), and in fp32 half an ulp of that 0.5, and
// of the fp32 constants, is up to 7e-5 of the result (tests/test_bicodec_kernels_gpu.py::test_fsq).  A few tanh per token: no cost.
struct FsqConsts {
    int nl;
    int levels[8];
    double half_l[8], offset[8], shift[8];
};
__global__ __launch_bounds__(256) void fsq_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                  FsqConsts q, int D, long long rows, int* __restrict__ tokens, float* __restrict__ bounded) {
    const int lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const float* xr = x + r * D;
    int idx = 0, basis = 1;
    for (int d = 0; d < q.nl; ++d) {
        float z = 0.f;
        for (int k = lane; k < D; k += 64) z = fmaf(w[d * D + k], xr[k], z);
        z = wave_sum(z) + bias[d];
        const float bd = (float)(tanh((double)z + q.shift[d]) * q.half_l[d] - q.offset[d]);
        if (bounded && lane == 0) bounded[r * q.nl + d] = bd;
        idx += ((int)rintf(bd) + q.levels[d] / 2) * basis;
        basis *= q.levels[d];
    }
    if (lane == 0) tokens[r] = idx;
}
int launch_fsq(const float* x, const float* w, const float* bias, const int* levels, int nl, int D, long long rows, int* tokens,
               float* bounded, hipStream_t s) {
    QA_REQUIRE(nl >= 1 && nl <= 8, "fsq: %d levels", nl);
    FsqConsts q{};
    q.nl = nl;
    for (int d = 0; d < nl; ++d) {  // the reference's constants, in double: (L - 1) * (1 + 1e-3) / 2, 0.5 for even L, atanh(offset / half_l)
        q.levels[d] = levels[d];
        q.half_l[d] = (double)(levels[d] - 1) * (1.0 + 1e-3) / 2.0;
        q.offset[d] = levels[d] % 2 == 0 ? 0.5 : 0.0;
        q.shift[d] = std::atanh(q.offset[d] / q.half_l[d]);
    }
    hipLaunchKernelGGL(fsq_kernel, dim3((unsigned)ceil_div(rows, 4)), dim3(256), 0, s, x, w, bias, q, D, rows, tokens, bounded);
    QA_LAUNCH_CHECK();
    return QA_OK;
}

// ---------------------------------------------------------------- BiCodec.forward (bicodec.py:113-149): x-vector head, code statistics

// ASTP (speaker/pooling_layers.py:119-144) after linear2: per (b, c) alpha = softmax_T(logit[b, :, c]),
// mean = sum alpha x, var = sum alpha x^2 - mean^2, std = sqrt(max(var, 1e-7)) -> pool[b, c] / pool[b, C + c]; bn[b, :] = the same
// through BatchNorm1d (eval) as y = v * s + t (ecapa_tdnn.py:205).  Time-major inputs [B, T, C]: a workgroup owns 64 contiguous
// channels (one per lane, coalesced rows) and its four waves take every fourth frame with an online (running-maximum) softmax, so each
// input is read once.  The exponentials are fp32; the three running sums are fp64, and the four partial states merge in wave order,
// so the result does not depend on timing.
constexpr int ASTP_SLICES = 4;
__global__ __launch_bounds__(256) void astp_pool_kernel(const float* __restrict__ logit, const float* __restrict__ x, int T, int C,
                                                        const float* __restrict__ bn_s, const float* __restrict__ bn_t,
                                                        float* __restrict__ pool, float* __restrict__ bn) {
    __shared__ double st[ASTP_SLICES][4][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lane, b = blockIdx.y;
    float m = -INFINITY;
    double l = 0.0, s1 = 0.0, s2 = 0.0;
    if (c < C) {
        const float* lr = logit + (long long)b * T * C + c;
        const float* xr = x + (long long)b * T * C + c;
        for (int t = w; t < T; t += ASTP_SLICES) {
            const float v = lr[(long long)t * C];
            const double xv = (double)xr[(long long)t * C];
            if (v > m) {  // new maximum: rescale what was summed so far (exp(-inf) = 0 on the first frame)
                const double r = (double)expf(m - v);
                l = l * r + 1.0;
                s1 = s1 * r + xv;
                s2 = s2 * r + xv * xv;
                m = v;
            } else {
                const double e = (double)expf(v - m);
                l += e;
                s1 += e * xv;
                s2 += e * xv * xv;
            }
        }
    }
    st[w][0][lane] = (double)m;
    st[w][1][lane] = l;
    st[w][2][lane] = s1;
    st[w][3][lane] = s2;
    __syncthreads();
    if (w != 0 || c >= C) return;
    double M = st[0][0][lane], L = st[0][1][lane], S1 = st[0][2][lane], S2 = st[0][3][lane];  // slice 0 holds frame 0: M is finite
    for (int k = 1; k < ASTP_SLICES; ++k) {
        const double mk = st[k][0][lane];
        if (!(mk > -INFINITY)) continue;  // a slice without frames (T < 4)
        const double nm = fmax(M, mk), ra = exp(M - nm), rb = exp(mk - nm);
        L = L * ra + st[k][1][lane] * rb;
        S1 = S1 * ra + st[k][2][lane] * rb;
        S2 = S2 * ra + st[k][3][lane] * rb;
        M = nm;
    }
    const double mean = S1 / L, var = S2 / L - mean * mean;
    const float mf = (float)mean, sf = (float)sqrt(fmax(var, 1e-7));
    float* pr = pool + (long long)b * 2 * C;
    float* br = bn + (long long)b * 2 * C;
    pr[c] = mf;
    pr[C + c] = sf;
    br[c] = fmaf(mf, bn_s[c], bn_t[c]);
    br[C + c] = fmaf(sf, bn_s[C + c], bn_t[C + c]);
}
int launch_astp_pool(const float* logit, const float* x, int B, int T, int C, const float* bn_s, const float* bn_t, float* pool, float* bn,
                     hipStream_t s) {
    QA_REQUIRE(B > 0 && T > 0 && C > 0 && B < 65536, "astp_pool: [%d, %d, %d]", B, T, C);
    hipLaunchKernelGGL(astp_pool_kernel, dim3((unsigned)ceil_div(C, 64), (unsigned)B), dim3(256), 0, s, logit, x, T, C, bn_s, bn_t, pool, bn);
    QA_LAUNCH_CHECK();
    return QA_OK;
}

// ASTP's global context (pooling_layers.py:129-133, global_context_att=True as ECAPA_TDNN_GLOB_c512 builds it): per (b, c) the plain
// mean over frames and sqrt(var + 1e-7) with torch.var's unbiased variance (T = 1 gives NaN, as torch does) -> ctx[b, c] / ctx[b, C + c].
// Layout and parallel split as astp_pool_kernel; the sums are fp64.
__global__ __launch_bounds__(256) void frame_stats_kernel(const float* __restrict__ x, int T, int C, float* __restrict__ ctx) {
    __shared__ double st[ASTP_SLICES][2][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lane, b = blockIdx.y;
    double s1 = 0.0, s2 = 0.0;
    if (c < C) {
        const float* xr = x + (long long)b * T * C + c;
        for (int t = w; t < T; t += ASTP_SLICES) {
            const double v = (double)xr[(long long)t * C];
            s1 += v;
            s2 += v * v;
        }
    }
    st[w][0][lane] = s1;
    st[w][1][lane] = s2;
    __syncthreads();
    if (w != 0 || c >= C) return;
    double S1 = st[0][0][lane], S2 = st[0][1][lane];
    for (int k = 1; k < ASTP_SLICES; ++k) {
        S1 += st[k][0][lane];
        S2 += st[k][1][lane];
    }
    const double mean = S1 / T, var = (S2 - S1 * mean) / (double)(T - 1);
    ctx[(long long)b * 2 * C + c] = (float)mean;
    ctx[(long long)b * 2 * C + C + c] = (float)sqrt(var + 1e-7);
}
int launch_frame_stats(const float* x, int B, int T, int C, float* ctx, hipStream_t s) {
    QA_REQUIRE(B > 0 && T > 0 && C > 0 && B < 65536, "frame_stats: [%d, %d, %d]", B, T, C);
    hipLaunchKernelGGL(frame_stats_kernel, dim3((unsigned)ceil_div(C, 64), (unsigned)B), dim3(256), 0, s, x, T, C, ctx);
    QA_LAUNCH_CHECK();
    return QA_OK;
}

// FactorizedVectorQuantize.forward's code statistics (vq/factorized_vector_quantize.py:98-103) over ALL n = B * N indices of a call:
// p_k = count_k / n (fp32, as torch.mean of the one-hot), perplexity = exp(-sum_k p_k log(p_k + 1e-10)), active = #{k : count_k > 0}.
// One workgroup: an integer histogram of K bins in LDS, then every thread sums its bins k = tid, tid + 1024, ... in fp64 and the
// partial sums meet in a fixed butterfly / wave order - bitwise reproducible from run to run.
__global__ __launch_bounds__(1024) void code_usage_kernel(const long long* __restrict__ idx, long long n, int K, float* __restrict__ perplexity,
                                                          float* __restrict__ active) {
    extern __shared__ int hist[];
    __shared__ double red[16];
    __shared__ int redi[16];
    for (int k = threadIdx.x; k < K; k += 1024) hist[k] = 0;
    __syncthreads();
    for (long long i = threadIdx.x; i < n; i += 1024) {
        const long long v = idx[i];
        if (v >= 0 && v < K) atomicAdd(&hist[v], 1);
    }
    __syncthreads();
    const float nf = (float)n;
    double h = 0.0;
    int used = 0;
    for (int k = threadIdx.x; k < K; k += 1024) {
        const int cnt = hist[k];
        const float p = (float)cnt / nf;
        h += (double)p * log((double)(p + 1e-10f));
        used += cnt > 0;
    }
    h = wave_sum_d(h);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) used += __shfl_xor(used, o, 64);
    if ((threadIdx.x & 63) == 0) {
        red[threadIdx.x >> 6] = h;
        redi[threadIdx.x >> 6] = used;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double H = 0.0;
        int U = 0;
        for (int i = 0; i < 16; ++i) {
            H += red[i];
            U += redi[i];
        }
        perplexity[0] = (float)exp(-H);
        active[0] = (float)U;
    }
}
int launch_code_usage(const long long* idx, long long n, int K, float* perplexity, float* active, hipStream_t s) {
    QA_REQUIRE(n > 0 && n < (1LL << 24) && K >= 1 && K <= 16384, "code_usage: %lld indices, codebook %d (n < 2^24, K <= 16384)", n, K);
    // K * 4 B of dynamic LDS (64 KiB at the largest K) beside 192 B of static (red, redi): 65,728 B in all at K = 16384, past 64 KiB
    // from K = 16337 on.  Both sides of that line launch and count as they are without hipFuncSetAttribute (K = 16336 and 16384,
    // tests/test_bicodec_kernels_gpu.py::test_code_usage on an MI355X: the dynamic request itself never passes 64 KiB), so nothing is
    // raised here and a captured forward makes no attribute call.
    hipLaunchKernelGGL(code_usage_kernel, dim3(1), dim3(1024), (size_t)K * sizeof(int), s, idx, n, K, perplexity, active);
    QA_LAUNCH_CHECK();
    return QA_OK;
}

// int32 -> int64 (the FSQ indices of get_global_tokens as the detokenizer's global tokens)
__global__ __launch_bounds__(256) void widen_i32_kernel(const int* __restrict__ src, long long* __restrict__ dst, long long n) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] = src[i];
}
int launch_widen_i32(const int* src, long long* dst, long long n, hipStream_t s) {
    if (n <= 0) return QA_OK;
    hipLaunchKernelGGL(widen_i32_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, s, src, dst, n);
    QA_LAUNCH_CHECK();
    return QA_OK;
}

}  // namespace qa

// ------------------------------------------------------------------------------------------------
// test hooks (not part of the public header): the kernels above alone on caller-provided device buffers, one launcher call each
// (tests/test_bicodec_kernels_gpu.py).  lens: device int32 or null, as the launchers take it; levels: HOST int32 [nl].
// wav_normalize and code_usage are reached through qa_wav_normalize / qa_wav_normalize_ragged / qa_code_usage.
extern "C" int qa_debug_gather_rows(const long long* tok, const float* table, float* out, long long n, int V, int D, int T, const int* lens,
                                    void* stream) {
    return qa::launch_gather_rows(tok, table, out, n, V, D, static_cast<hipStream_t>(stream), T, lens);
}
extern "C" int qa_debug_gather_global(const long long* tok, const float* table, float* out, int B, int N, int V, int L, void* stream) {
    return qa::launch_gather_global(tok, table, out, B, N, V, L, static_cast<hipStream_t>(stream));
}
extern "C" int qa_debug_tokens_fill_behind(long long* tok, int B, int N, const int* lens, void* stream) {
    return qa::launch_tokens_fill_behind(tok, B, N, lens, static_cast<hipStream_t>(stream));
}
extern "C" int qa_debug_zero_behind(float* x, int B, long long T, const int* lens, int len_mul, void* stream) {
    return qa::launch_zero_behind(x, B, T, qa::ClipLens{lens, len_mul}, static_cast<hipStream_t>(stream));
}
extern "C" int qa_debug_adaln(const float* x, const float* scale, const float* shift, long long ld_cond, float* y, int B, int T, int C,
                              float eps, void* stream) {
    return qa::launch_adaln(x, scale, shift, ld_cond, y, B, T, C, eps, static_cast<hipStream_t>(stream));
}
extern "C" int qa_debug_add_rowvec(float* x, const float* v, int B, int T, int C, void* stream) {
    return qa::launch_add_rowvec(x, v, B, T, C, static_cast<hipStream_t>(stream));
}
extern "C" int qa_debug_l2norm_rows(const float* x, float* y, long long rows, int D, void* stream) {
    return qa::launch_l2norm_rows(x, y, rows, D, static_cast<hipStream_t>(stream));
}
extern "C" int qa_debug_l2norm_scale(const float* x, const float* gamma, float* y, long long rows, int D, float scale, void* stream) {
    return qa::launch_l2norm_scale(x, gamma, y, rows, D, scale, static_cast<hipStream_t>(stream));
}
extern "C" int qa_debug_mel_frames(const float* wav, int B, long long T, long long ref_len, int hop, int n_frames, float* P, const int* lens,
                                   void* stream) {
    return qa::launch_mel_frames(wav, B, T, ref_len, hop, n_frames, P, static_cast<hipStream_t>(stream), lens);
}
extern "C" int qa_debug_spec_mag(const float* ri, int nbp, int nb, float* mag, int ldm, long long rows, void* stream) {
    return qa::launch_spec_mag(ri, nbp, nb, mag, ldm, rows, static_cast<hipStream_t>(stream));
}
extern "C" int qa_debug_geglu(const float* h, int F, float* out, int ldo, long long rows, void* stream) {
    return qa::launch_geglu(h, F, out, ldo, rows, static_cast<hipStream_t>(stream));
}
extern "C" int qa_debug_perceiver_ctx(const float* lat, long long lat_b, const float* x, float* ctx, int B, int n_lat, int T, int D,
                                      void* stream) {
    return qa::launch_perceiver_ctx(lat, lat_b, x, ctx, B, n_lat, T, D, static_cast<hipStream_t>(stream));
}
extern "C" int qa_debug_res2_chain(const float* x, float* y, const float* wt, const float* bst, int B, int T, int C, int d, void* stream) {
    return qa::launch_res2_chain(x, y, wt, bst, B, T, C, d, static_cast<hipStream_t>(stream));
}
extern "C" int qa_debug_se_residual(const float* x, long long ldx, const float* y, const float* w1t, const float* b1, const float* w2t,
                                    const float* b2, float* gate, float* out, long long ldo, int B, int T, int C, int Hd, void* stream) {
    return qa::launch_se_residual(x, ldx, y, w1t, b1, w2t, b2, gate, out, ldo, B, T, C, Hd, static_cast<hipStream_t>(stream));
}
extern "C" int qa_debug_fsq(const float* x, const float* w, const float* bias, const int* levels, int nl, int D, long long rows, int* tokens,
                            float* bounded, void* stream) {
    return qa::launch_fsq(x, w, bias, levels, nl, D, rows, tokens, bounded, static_cast<hipStream_t>(stream));
}
extern "C" int qa_debug_astp_pool(const float* logit, const float* x, int B, int T, int C, const float* bn_s, const float* bn_t, float* pool,
                                  float* bn, void* stream) {
    return qa::launch_astp_pool(logit, x, B, T, C, bn_s, bn_t, pool, bn, static_cast<hipStream_t>(stream));
}
extern "C" int qa_debug_frame_stats(const float* x, int B, int T, int C, float* ctx, void* stream) {
    return qa::launch_frame_stats(x, B, T, C, ctx, static_cast<hipStream_t>(stream));
}
extern "C" int qa_debug_widen_i32(const int* src, long long* dst, long long n, void* stream) {
    return qa::launch_widen_i32(src, dst, n, static_cast<hipStream_t>(stream));
}
