// lm_kernels.hip - the UniSE AR-LM's prefill-side kernels: prompt assembly, RoPE + KV-cache append over a whole
// prompt, and the skinny-M weight-streaming GEMM (per-item linears of at most 32 rows: tiny prompts here, BiCodec's d-vector / AdaLN
// linears in bicodec.cpp), and the teacher-forced scoring kernels (target embedding, row loss, fixed-order reduces).  The decode step
// lives in lm_decode.hip; the round-1 per-op decode kernels (embedding gather, arg-max,
// single-query attention behind QA_LM_UNFUSED) were removed in round 5.
#include "kernels.h"

#include <cstring>

namespace qa {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------------------------------------
// llm_sft.py:110-128: prompt = [task, (enroll_sos, adapter(enroll)), mix_sos, adapter(mix)]  -> x [B, L, d]
// Ragged batches (off != nullptr): row b uses the first Ne + off[b] of its Ne enrollment rows and is laid out
// left-aligned over L + off[b] positions; the positions behind are written as zeros and the enrollment rows behind are never read.
__global__ __launch_bounds__(256) void assemble_prompt_kernel(float* __restrict__ x, const float* __restrict__ task_vec,
                                                              const float* __restrict__ enroll_sos,
                                                              const float* __restrict__ enroll_emb,
                                                              const float* __restrict__ mix_sos,
                                                              const float* __restrict__ mix_emb, int B, int Ne, int Nm,
                                                              int d, const int* __restrict__ off) {
    const int L = 1 + (enroll_emb ? 1 + Ne : 0) + 1 + Nm;
    const int d4 = d >> 2;
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (long long)B * L * d4) return;
    const int c = (int)(gid % d4) * 4;
    const int pos = (int)((gid / d4) % L);
    const int b = (int)(gid / ((long long)d4 * L));
    const int ne = off ? Ne + off[b] : Ne;  // this row's enrollment frames
    const float* src;
    int p = pos;
    if (p == 0) {
        src = task_vec;
    } else {
        p -= 1;
        if (enroll_emb && p == 0) {
            src = enroll_sos;
        } else {
            if (enroll_emb) p -= 1;
            if (enroll_emb && p < ne) {
                src = enroll_emb + ((long long)b * Ne + p) * d;
            } else {
                if (enroll_emb) p -= ne;
                src = (p == 0) ? mix_sos : (p <= Nm) ? mix_emb + ((long long)b * Nm + (p - 1)) * d : nullptr;
            }
        }
    }
    *reinterpret_cast<float4*>(x + ((long long)b * L + pos) * d + c) =
        src ? *reinterpret_cast<const float4*>(src + c) : make_float4(0.f, 0.f, 0.f, 0.f);
}

int launch_assemble_prompt(float* x, const float* task_vec, const float* enroll_sos, const float* enroll_emb,
                           const float* mix_sos, const float* mix_emb, int B, int Ne, int Nm, int d, hipStream_t s, const int* off) {
    QA_REQUIRE(!off || enroll_emb, "assemble_prompt: per-row lengths need an enrollment");
    const int L = 1 + (enroll_emb ? 1 + Ne : 0) + 1 + Nm;
    const long long total = (long long)B * L * (d / 4);
    hipLaunchKernelGGL(assemble_prompt_kernel, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, s, x, task_vec,
                       enroll_sos, enroll_emb, mix_sos, mix_emb, B, Ne, Nm, d, off);
    QA_LAUNCH_CHECK();
    return QA_OK;
}

// ------------------------------------------------------------------------------------------------
// Skinny-M GEMM for the decode steps: y[M <= 16*MT, N] = epi(x[M, K] W[N, K]^T).  Weight streaming is the whole cost
// (226 MB of fp32 weights per step, SURVEY.md hard part 2), so: one workgroup per 16 output columns, its 8 waves split K,
// every lane streams 32 B-contiguous pieces of its weight row straight from HBM into v_mfma_f32_16x16x4_f32 (the batch
// rows are the M side), partial tiles are reduced through LDS in a fixed order (deterministic, no atomics) and the same
// fused epilogue as conv_gemm is applied.
// Two fusions remove launches from the decode step:
//   rms_eps > 0: the input is the un-normalised residual stream; RMSNorm's weight has been folded into W on the host
//                (W' = W diag(w)), so y = rstd[m] * (x W'^T) and only the per-row rstd is computed here (every workgroup
//                recomputes it from the 16 x K input it reads anyway);
//   DUAL:        W holds, per 16-column group, 16 "gate" rows followed by 16 "up" rows; y = silu(gate) * up (SwiGLU).
template <int MT, bool DUAL>
__global__ __launch_bounds__(512) void skinny_gemm_kernel(const float* __restrict__ x, long long ldx,
                                                          const float* __restrict__ w, const float* __restrict__ bias,
                                                          const float* __restrict__ gate, long long ldg,
                                                          const float* __restrict__ res, long long ldr,
                                                          float* __restrict__ y, long long ldy, int M, int N, int K,
                                                          int act, float rms_eps) {
    constexpr int NA = DUAL ? 2 : 1;
    __shared__ float part[8][NA][MT][16][17];
    __shared__ float s_rstd[MT * 16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, kq = lane >> 4;
    const int n0 = blockIdx.x * 16;
    const int kw = K / 8, k0 = wave * kw;
    if (rms_eps > 0.f) {
        for (int r = wave; r < MT * 16; r += 8) {
            const float* xr = x + (long long)min(r, M - 1) * ldx;
            float sq = 0.f;
            for (int c = lane * 4; c < K; c += 256) {
                const float4 t = *reinterpret_cast<const float4*>(xr + c);
                sq += t.x * t.x + t.y * t.y + t.z * t.z + t.w * t.w;
            }
            sq = wave_sum(sq);
            if (lane == 0) s_rstd[r] = rsqrtf(sq / K + rms_eps);
        }
    }
    const int nrow = min(n0 + li, N - 1);
    const float* wp[NA];
    wp[0] = w + (long long)(DUAL ? (blockIdx.x * 32 + li) : nrow) * K + k0 + 8 * kq;
    if (DUAL) wp[NA - 1] = w + (long long)(blockIdx.x * 32 + 16 + li) * K + k0 + 8 * kq;
    const float* xp[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) xp[m] = x + (long long)min(m * 16 + li, M - 1) * ldx + k0 + 8 * kq;
    f32x4 acc[NA][MT];
#pragma unroll
    for (int a = 0; a < NA; ++a)
#pragma unroll
        for (int m = 0; m < MT; ++m) acc[a][m] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
    for (int g = 0; g < kw; g += 32) {
        float4 w0[NA], w1[NA];
#pragma unroll
        for (int a = 0; a < NA; ++a) {
            w0[a] = *reinterpret_cast<const float4*>(wp[a] + g);
            w1[a] = *reinterpret_cast<const float4*>(wp[a] + g + 4);
        }
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            const float4 a0 = *reinterpret_cast<const float4*>(xp[m] + g);
            const float4 a1 = *reinterpret_cast<const float4*>(xp[m] + g + 4);
#pragma unroll
            for (int a = 0; a < NA; ++a) {
                acc[a][m] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.x, w0[a].x, acc[a][m], 0, 0, 0);
                acc[a][m] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.y, w0[a].y, acc[a][m], 0, 0, 0);
                acc[a][m] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.z, w0[a].z, acc[a][m], 0, 0, 0);
                acc[a][m] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.w, w0[a].w, acc[a][m], 0, 0, 0);
                acc[a][m] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.x, w1[a].x, acc[a][m], 0, 0, 0);
                acc[a][m] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.y, w1[a].y, acc[a][m], 0, 0, 0);
                acc[a][m] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.z, w1[a].z, acc[a][m], 0, 0, 0);
                acc[a][m] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.w, w1[a].w, acc[a][m], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int a = 0; a < NA; ++a)
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r) part[wave][a][m][4 * kq + r][li] = acc[a][m][r];
    __syncthreads();
    for (int i = tid; i < MT * 256; i += 512) {
        const int row = i >> 4, col = i & 15;
        const int n = n0 + col;
        if (row >= M || n >= N) continue;
        float v = 0.f, u = 0.f;
#pragma unroll
        for (int wv = 0; wv < 8; ++wv) {
            v += part[wv][0][row >> 4][row & 15][col];
            if (DUAL) u += part[wv][NA - 1][row >> 4][row & 15][col];
        }
        if (rms_eps > 0.f) {
            v *= s_rstd[row];
            u *= s_rstd[row];
        }
        if (bias) v += bias[n];
        if (DUAL) v = silu_f(v) * u;
        if (gate) v = silu_f(gate[(long long)row * ldg + n]) * v;
        v = apply_act(v, act);
        if (res) v += res[(long long)row * ldr + n];
        y[(long long)row * ldy + n] = v;
    }
}

int launch_skinny_gemm(const float* x, long long ldx, const float* w, const float* bias, const float* gate,
                       long long ldg, const float* res, long long ldr, float* y, long long ldy, int M, int N, int K,
                       int act, hipStream_t s, float rms_eps, int dual) {
    QA_REQUIRE(M >= 1 && M <= 32, "skinny_gemm: M=%d must be in [1, 32]", M);
    QA_REQUIRE(K % 256 == 0 && (ldx % 4) == 0, "skinny_gemm: K=%d must be a multiple of 256", K);
    QA_REQUIRE(!dual || N % 16 == 0, "skinny_gemm: dual mode needs N %% 16 == 0");
    const dim3 grid((unsigned)ceil_div(N, 16));
#define QA_SK(MT, DUAL)                                                                                                  \
    hipLaunchKernelGGL((skinny_gemm_kernel<MT, DUAL>), grid, dim3(512), 0, s, x, ldx, w, bias, gate, ldg, res, ldr, y, ldy, M, N, \
                       K, act, rms_eps)
    if (M <= 16) {
        if (dual) QA_SK(1, true); else QA_SK(1, false);
    } else {
        if (dual) QA_SK(2, true); else QA_SK(2, false);
    }
#undef QA_SK
    QA_LAUNCH_CHECK();
    return QA_OK;
}

// RoPE (rotate-half, position pos0 + t) on the q and k parts of a fused [B*n, 3d] buffer in place, and append k, v to the caches
// RAGGED (a session chunk with per-row lengths): item b's rows start at position row_pos0[b] and only its first
// row_n[b] rows exist - the others are neither rotated nor appended, so a row that ends at max_len writes nothing into its neighbour
template <bool RAGGED>
__global__ __launch_bounds__(256) void rope_kv_kernel(float* __restrict__ qkv, const float* __restrict__ cs,
                                                      float* __restrict__ kc, float* __restrict__ vc, int B, int n, int H,
                                                      int hd, int pos0, int max_len, const int* __restrict__ row_pos0,
                                                      const int* __restrict__ row_n) {
    const int half = hd >> 1, d = H * hd;
    const long long total = (long long)B * n * H * half;
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= total) return;
    const int i = (int)(gid % half);
    const int h = (int)((gid / half) % H);
    const long long row = gid / ((long long)half * H);
    const int b = (int)(row / n), t = (int)(row % n);
    if (RAGGED) {
        if (t >= row_n[b]) return;
        pos0 = row_pos0[b];
    }
    const int pos = pos0 + t;
    const float c = cs[((long long)pos * half + i) * 2], sn = cs[((long long)pos * half + i) * 2 + 1];
    float* q = qkv + row * 3 * d + h * hd;
    const float q1 = q[i], q2 = q[i + half];
    q[i] = q1 * c - q2 * sn;
    q[i + half] = q2 * c + q1 * sn;
    const float* k = q + d;
    const float* v = q + 2 * d;
    const long long dst = ((long long)b * max_len + pos) * d + h * hd;
    const float k1 = k[i], k2 = k[i + half];
    kc[dst + i] = k1 * c - k2 * sn;
    kc[dst + i + half] = k2 * c + k1 * sn;
    vc[dst + i] = v[i];
    vc[dst + i + half] = v[i + half];
}
int launch_rope_kv(float* qkv, const float* cs, float* kc, float* vc, int B, int n, int H, int hd, int pos0, int max_len,
                   hipStream_t s, const int* row_pos0, const int* row_n) {
    QA_REQUIRE((row_pos0 == nullptr) == (row_n == nullptr), "rope_kv: per-row positions and counts come together");
    const long long total = (long long)B * n * H * (hd / 2);
    const dim3 grid((unsigned)ceil_div(total, 256));
    if (row_n) hipLaunchKernelGGL(rope_kv_kernel<true>, grid, dim3(256), 0, s, qkv, cs, kc, vc, B, n, H, hd, pos0, max_len, row_pos0, row_n);
    else hipLaunchKernelGGL(rope_kv_kernel<false>, grid, dim3(256), 0, s, qkv, cs, kc, vc, B, n, H, hd, pos0, max_len, row_pos0, row_n);
    QA_LAUNCH_CHECK();
    return QA_OK;
}

// ------------------------------------------------------------------------------------------------
// Per-row lengths of a session call.  The lengths are host data: launch_row_ints (ew.hip) writes them into a device
// array the cache owns, in stream order.
//
// The input of a ragged chunk: rows t < row_n[b] are copied, the others become exact zeros WITHOUT being read.  A zero row stays a zero
// row through the whole body (no projection of the Llama layers has a bias, RMSNorm and SwiGLU map 0 to 0, and the ragged attention
// writes 0 for such a query), so the padded rows of every hidden state and of the final norm come out as 0 with no launch of their own.
__global__ __launch_bounds__(256) void lm_rows_masked_copy_kernel(float4* __restrict__ y, const float4* __restrict__ x, int B, int n, int d4,
                                                                  const int* __restrict__ row_n) {
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (long long)B * n * d4) return;
    const long long row = gid / d4;
    const int b = (int)(row / n), t = (int)(row % n);
    y[gid] = t < row_n[b] ? x[gid] : make_float4(0.f, 0.f, 0.f, 0.f);
}
int launch_lm_rows_masked_copy(float* y, const float* x, int B, int n, int d, const int* row_n, hipStream_t s) {
    QA_REQUIRE(d % 4 == 0 && row_n, "lm_rows_masked_copy: bad launch");
    const long long total = (long long)B * n * (d / 4);
    hipLaunchKernelGGL(lm_rows_masked_copy_kernel, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, s, reinterpret_cast<float4*>(y),
                       reinterpret_cast<const float4*>(x), B, n, d / 4, row_n);
    QA_LAUNCH_CHECK();
    return QA_OK;
}

// The outputs of a ragged n = 1 step: the fused step computes every row of its group, so the idle rows' outputs (and their copies in
// all_hidden) are overwritten with exact zeros here, one launch for all entries.  Grid: x covers an entry, y = entry.
__global__ __launch_bounds__(256) void lm_rows_zero_pad_kernel(float4* __restrict__ y, long long entry_stride4, int B, int n, int d4,
                                                               const int* __restrict__ row_n) {
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (long long)B * n * d4) return;
    const long long row = gid / d4;
    const int b = (int)(row / n), t = (int)(row % n);
    if (t >= row_n[b]) y[(long long)blockIdx.y * entry_stride4 + gid] = make_float4(0.f, 0.f, 0.f, 0.f);
}
int launch_lm_rows_zero_pad(float* y, long long entry_stride, int entries, int B, int n, int d, const int* row_n, hipStream_t s) {
    QA_REQUIRE(d % 4 == 0 && entry_stride % 4 == 0 && entries >= 1 && entries <= 65535 && row_n, "lm_rows_zero_pad: bad launch");
    const long long total = (long long)B * n * (d / 4);
    hipLaunchKernelGGL(lm_rows_zero_pad_kernel, dim3((unsigned)ceil_div(total, 256), (unsigned)entries), dim3(256), 0, s,
                       reinterpret_cast<float4*>(y), entry_stride / 4, B, n, d / 4, row_n);
    QA_LAUNCH_CHECK();
    return QA_OK;
}

// ------------------------------------------------------------------------------------------------
// Teacher-forced scoring (LLM_SFT.forward, llm_sft.py:37-90).  With Lt = G + T + 2 target positions per sequence:
//   input_ids  = [0, g + 3, 1, s + soff]      -> codec_embedding rows at x[b, t, :] (x: rows of ldx_seq floats per sequence)
//   target_ids = [g + 3, 1, s + soff, 2]      -> tgt[b * Lt + t]
// Ids are clamped into [0, V) so that no read leaves the table; the caller range-checks them first (qa_codes_check: IndexError).
__device__ __forceinline__ long long clamp_id(long long v, int V) { return v < 0 ? 0 : (v >= V ? V - 1 : v); }

__global__ __launch_bounds__(256) void lm_targets_kernel(float* __restrict__ x, long long ldx_seq, const float* __restrict__ table,
                                                         const long long* __restrict__ gids, int G, const long long* __restrict__ sids,
                                                         int T, int V, int goff, int soff, long long* __restrict__ tgt, int B, int d, int drop) {
    const int Lt = G + T + 2 - drop, d4 = d >> 2;  // drop = 1: CustomLlamaModel.forward leaves the last position out (llm.py:126-127)
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (long long)B * Lt * d4) return;
    const int c = (int)(gid % d4) * 4;
    const int t = (int)((gid / d4) % Lt);
    const int b = (int)(gid / ((long long)d4 * Lt));
    long long in_id, tg;
    if (t == 0) in_id = 0;
    else if (t <= G) in_id = gids[(long long)b * G + t - 1] + goff;
    else if (t == G + 1) in_id = 1;
    else in_id = sids[(long long)b * T + t - G - 2] + soff;
    if (t < G) tg = gids[(long long)b * G + t] + goff;
    else if (t == G) tg = 1;
    else if (t < G + T + 1) tg = sids[(long long)b * T + t - G - 1] + soff;
    else tg = 2;
    in_id = clamp_id(in_id, V);
    *reinterpret_cast<float4*>(x + b * ldx_seq + (long long)t * d + c) = *reinterpret_cast<const float4*>(table + in_id * d + c);
    if (c == 0) tgt[(long long)b * Lt + t] = clamp_id(tg, V);
}

int launch_lm_targets(float* x, long long ldx_seq, const float* table, const long long* gids, int G, const long long* sids, int T, int V,
                      int goff, int soff, long long* tgt, int B, int d, hipStream_t s, int drop) {
    QA_REQUIRE(d % 4 == 0 && ldx_seq % 4 == 0 && (drop == 0 || drop == 1), "lm_targets: d %d / row stride must be multiples of 4", d);
    const long long total = (long long)B * (G + T + 2 - drop) * (d / 4);
    hipLaunchKernelGGL(lm_targets_kernel, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, s, x, ldx_seq, table, gids, G, sids, T, V,
                       goff, soff, tgt, B, d, drop);
    QA_LAUNCH_CHECK();
    return QA_OK;
}

// Row loss: one workgroup per row of the head's logits z [rows, V] (row stride ldl), ONE pass over the row.  Every thread keeps
// (running max m, sum of exp(z - m), sum of z, first arg-max) over the columns it owns (j = tid + 256 i, increasing), the four waves
// merge theirs with a fixed butterfly and thread 0 merges the four waves in order: no atomics, the same bits in any batch.
// Label-smoothed KL against true_dist = c at the target, s elsewhere (llm.py:87-104), in closed form (0 log 0 = 0, as xlogy):
//   kl = c log c + (V - 1) s log s - c (z_y - lse) - s (sum z - z_y - (V - 1) lse)
struct RowStat {
    float m, s, sz, bv;
    int bi;
};
__device__ __forceinline__ RowStat row_merge(RowStat a, const RowStat& b) {
    const float M = fmaxf(a.m, b.m);  // a part with s = 0 owns no column (m = -inf): it adds nothing, and no exp(-inf - -inf) is formed
    a.s = (a.s > 0.f ? a.s * expf(a.m - M) : 0.f) + (b.s > 0.f ? b.s * expf(b.m - M) : 0.f);
    a.m = M;
    a.sz += b.sz;
    if (b.bv > a.bv || (b.bv == a.bv && b.bi < a.bi)) {
        a.bv = b.bv;
        a.bi = b.bi;
    }
    return a;
}

__global__ __launch_bounds__(256) void lm_row_loss_kernel(const float* __restrict__ z, long long ldl, int V, const long long* __restrict__ tgt,
                                                          float c, float sm, float* __restrict__ row_kl, int* __restrict__ row_ok) {
    __shared__ RowStat s_w[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* zr = z + (long long)blockIdx.x * ldl;
    RowStat st{-INFINITY, 0.f, 0.f, -INFINITY, V};
    int j = tid;
    for (; j + 768 < V; j += 1024) {  // four independent loads in flight per thread
        const float v0 = zr[j], v1 = zr[j + 256], v2 = zr[j + 512], v3 = zr[j + 768];
        const float vm = fmaxf(fmaxf(v0, v1), fmaxf(v2, v3));
        const float M = fmaxf(st.m, vm);
        st.s = st.s * expf(st.m - M) + (expf(v0 - M) + expf(v1 - M)) + (expf(v2 - M) + expf(v3 - M));
        st.m = M;
        st.sz += (v0 + v1) + (v2 + v3);
        if (v0 > st.bv) { st.bv = v0; st.bi = j; }
        if (v1 > st.bv) { st.bv = v1; st.bi = j + 256; }
        if (v2 > st.bv) { st.bv = v2; st.bi = j + 512; }
        if (v3 > st.bv) { st.bv = v3; st.bi = j + 768; }
    }
    for (; j < V; j += 256) {
        const float v = zr[j];
        const float M = fmaxf(st.m, v);
        st.s = st.s * expf(st.m - M) + expf(v - M);
        st.m = M;
        st.sz += v;
        if (v > st.bv) { st.bv = v; st.bi = j; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        RowStat p;
        p.m = __shfl_xor(st.m, o, 64);
        p.s = __shfl_xor(st.s, o, 64);
        p.sz = __shfl_xor(st.sz, o, 64);
        p.bv = __shfl_xor(st.bv, o, 64);
        p.bi = __shfl_xor(st.bi, o, 64);
        st = (lane & o) ? row_merge(p, st) : row_merge(st, p);  // lower lanes' columns first: the same expression in every lane pair
    }
    if (lane == 0) s_w[wave] = st;
    __syncthreads();
    if (tid == 0) {
        RowStat a = s_w[0];
        for (int w = 1; w < 4; ++w) a = row_merge(a, s_w[w]);
        const long long y = tgt[blockIdx.x];
        const double lse = (double)a.m + log((double)a.s);
        const double zy = zr[y], Vm1 = (double)(V - 1), cd = c, sd = sm;
        double kl = (cd > 0.0 ? cd * log(cd) : 0.0) - cd * (zy - lse);
        if (sd > 0.0) kl += Vm1 * sd * log(sd) - sd * ((double)a.sz - zy - Vm1 * lse);
        row_kl[blockIdx.x] = (float)kl;
        row_ok[blockIdx.x] = a.bi == (int)y;
    }
}

int launch_lm_row_loss(const float* z, long long ldl, int V, long long rows, const long long* tgt, float c, float sm, float* row_kl,
                       int* row_ok, hipStream_t s) {
    if (rows <= 0) return QA_OK;
    hipLaunchKernelGGL(lm_row_loss_kernel, dim3((unsigned)rows), dim3(256), 0, s, z, ldl, V, tgt, c, sm, row_kl, row_ok);
    QA_LAUNCH_CHECK();
    return QA_OK;
}

// Per sequence (one workgroup each): seq_sum[b] = sum of its Lt row KLs in double, loss_seq[b] = seq_sum[b] / Lt, correct_seq[b] = its
// correct rows; thread i owns rows i, i + 256, ..., merged by a fixed LDS tree.
__global__ __launch_bounds__(256) void lm_seq_reduce_kernel(const float* __restrict__ row_kl, const int* __restrict__ row_ok, int Lt,
                                                            double* __restrict__ seq_sum, float* __restrict__ loss_seq,
                                                            long long* __restrict__ correct_seq) {
    __shared__ double s_kl[256];
    __shared__ long long s_ok[256];
    const int tid = threadIdx.x, b = blockIdx.x;
    double kl = 0.0;
    long long ok = 0;
    for (int t = tid; t < Lt; t += 256) {
        kl += (double)row_kl[(long long)b * Lt + t];
        ok += row_ok[(long long)b * Lt + t];
    }
    s_kl[tid] = kl;
    s_ok[tid] = ok;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h) {
            s_kl[tid] += s_kl[tid + h];
            s_ok[tid] += s_ok[tid + h];
        }
        __syncthreads();
    }
    if (tid == 0) {
        seq_sum[b] = s_kl[0];
        loss_seq[b] = (float)(s_kl[0] / Lt);
        correct_seq[b] = s_ok[0];
    }
}

int launch_lm_seq_reduce(const float* row_kl, const int* row_ok, int B, int Lt, double* seq_sum, float* loss_seq, long long* correct_seq,
                         hipStream_t s) {
    hipLaunchKernelGGL(lm_seq_reduce_kernel, dim3((unsigned)B), dim3(256), 0, s, row_kl, row_ok, Lt, seq_sum, loss_seq, correct_seq);
    QA_LAUNCH_CHECK();
    return QA_OK;
}

// The batch scalars (F.kl_div 'batchmean' over B * Lt rows, accuracy over the same rows): sequences in index order, one thread.
__global__ void lm_batch_reduce_kernel(const double* __restrict__ seq_sum, const long long* __restrict__ correct_seq, int B, int Lt,
                                       float* __restrict__ loss, float* __restrict__ acc) {
    double kl = 0.0;
    long long ok = 0;
    for (int b = 0; b < B; ++b) {
        kl += seq_sum[b];
        ok += correct_seq[b];
    }
    const double n = (double)B * Lt;
    *loss = (float)(kl / n);
    *acc = (float)((double)ok / n);
}

int launch_lm_batch_reduce(const double* seq_sum, const long long* correct_seq, int B, int Lt, float* loss, float* acc, hipStream_t s) {
    hipLaunchKernelGGL(lm_batch_reduce_kernel, dim3(1), dim3(1), 0, s, seq_sum, correct_seq, B, Lt, loss, acc);
    QA_LAUNCH_CHECK();
    return QA_OK;
}

// ------------------------------------------------------------------------------------------------
// Teacher-forced scoring with per-row lengths (qa_lm_score_ragged / qa_lm_prompt_ragged).  Row b of a group holds
// ne[b] of the Ne enrollment frames, nm[b] of the Nm mixture frames and T[b] of the T_max semantic ids (device int [B] each, written by
// launch_row_ints).  The rectangular kernels above keep their code: these are launched by the ragged entry points alone.
//
// One assembly pass: x [B, n, d] row b <- [task, (enroll_sos, enroll_emb[b, :ne])?, mix_sos, mix_emb[b, :nm], codec_embedding(input_ids_b)]
// left-aligned over L_b = Lp_b + Lt_b positions, exact zeros behind; target_ids_b -> tgt[off[b] ..] (PACKED: Lt_b = G + T[b] + 2 entries).
// The eos target sits right behind the row's own last semantic id.  Frames and ids at or behind a row's counts are never read.
// table == nullptr: a prompt-only pass (no target positions, gids / sids / tgt unused).
// task_vec == nullptr: CustomLlamaModel's form - the prompt is [mix_sos, mix_emb[b, :nm]] with mix_emb the condition
// embeddings, already in the LM's width, or nothing at all (mix_emb null too).  drop = 1 (that model's forward, llm.py:126-127): the last
// position of the row's OWN stream is left out, Lt_b = G + T[b] + 1, and with it the eos target.
__global__ __launch_bounds__(256) void lm_score_assemble_kernel(float* __restrict__ x, int n, const float* __restrict__ task_vec,
                                                                const float* __restrict__ enroll_sos, const float* __restrict__ enroll_emb,
                                                                const float* __restrict__ mix_sos, const float* __restrict__ mix_emb, int Ne,
                                                                int Nm, const float* __restrict__ table, const long long* __restrict__ gids,
                                                                int G, const long long* __restrict__ sids, int T_max, int V, int goff, int soff,
                                                                long long* __restrict__ tgt, const int* __restrict__ ne_r,
                                                                const int* __restrict__ nm_r, const int* __restrict__ T_r,
                                                                const int* __restrict__ off_r, int B, int d, int drop) {
    const int d4 = d >> 2;
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (long long)B * n * d4) return;
    const int c = (int)(gid % d4) * 4;
    const int pos = (int)((gid / d4) % n);
    const int b = (int)(gid / ((long long)d4 * n));
    const int ne = enroll_emb ? ne_r[b] : 0, nm = mix_emb ? nm_r[b] : 0;
    const int Lp = task_vec ? 1 + (enroll_emb ? 1 + ne : 0) + 1 + nm : (mix_emb ? 1 + nm : 0);
    const float* src = nullptr;
    if (pos < Lp) {
        int p = pos;
        if (!task_vec) {
            src = (p == 0) ? mix_sos : mix_emb + ((long long)b * Nm + (p - 1)) * d;  // p - 1 < nm: pos < Lp
        } else if (p == 0) {
            src = task_vec;
        } else {
            p -= 1;
            if (enroll_emb && p == 0) {
                src = enroll_sos;
            } else {
                if (enroll_emb) p -= 1;
                if (enroll_emb && p < ne) {
                    src = enroll_emb + ((long long)b * Ne + p) * d;
                } else {
                    if (enroll_emb) p -= ne;
                    src = (p == 0) ? mix_sos : mix_emb + ((long long)b * Nm + (p - 1)) * d;  // p - 1 < nm: pos < Lp
                }
            }
        }
    } else if (table) {
        const int T = T_r[b], t = pos - Lp;
        if (t < G + T + 2 - drop) {
            long long in_id, tg;
            if (t == 0) in_id = 0;
            else if (t <= G) in_id = gids[(long long)b * G + t - 1] + goff;
            else if (t == G + 1) in_id = 1;
            else in_id = sids[(long long)b * T_max + t - G - 2] + soff;
            if (t < G) tg = gids[(long long)b * G + t] + goff;
            else if (t == G) tg = 1;
            else if (t < G + T + 1) tg = sids[(long long)b * T_max + t - G - 1] + soff;
            else tg = 2;
            src = table + clamp_id(in_id, V) * d;
            if (c == 0) tgt[off_r[b] + t] = clamp_id(tg, V);
        }
    }
    *reinterpret_cast<float4*>(x + ((long long)b * n + pos) * d + c) =
        src ? *reinterpret_cast<const float4*>(src + c) : make_float4(0.f, 0.f, 0.f, 0.f);
}

int launch_lm_score_assemble(const ScoreAssembleArgs& a, hipStream_t s) {
    QA_REQUIRE(a.d % 4 == 0 && a.n >= 1 && a.B >= 1 && (!a.mix_emb || a.nm_r) && (a.task_vec || !a.enroll_emb) &&
                   (a.task_vec || a.mix_emb || a.table) && (!a.enroll_emb || a.ne_r) && (!a.table || (a.tgt && a.T_r && a.off_r)) &&
                   (a.drop == 0 || a.drop == 1), "lm_score_assemble: bad launch");
    const long long total = (long long)a.B * a.n * (a.d / 4);
    hipLaunchKernelGGL(lm_score_assemble_kernel, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, s, a.x, a.n, a.task_vec, a.enroll_sos,
                       a.enroll_emb, a.mix_sos, a.mix_emb, a.Ne, a.Nm, a.table, a.gids, a.G, a.sids, a.T_max, a.V, a.goff, a.soff, a.tgt, a.ne_r,
                       a.nm_r, a.T_r, a.off_r, a.B, a.d, a.drop);
    QA_LAUNCH_CHECK();
    return QA_OK;
}

// The packed tail: y [sum Lt_b, d] <- each row's last Lt_b = G + T[b] + 2 - drop live positions x[b, lp[b] + t, :], sequences in order.  Grid: x
// covers Lt_max rows of one sequence, y = sequence.
__global__ __launch_bounds__(256) void lm_score_gather_kernel(float4* __restrict__ y, const float4* __restrict__ x, int n, int d4, int G,
                                                              int Lt_max, const int* __restrict__ lp_r, const int* __restrict__ T_r,
                                                              const int* __restrict__ off_r, int drop) {
    const int b = blockIdx.y;
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (long long)Lt_max * d4) return;
    const int t = (int)(gid / d4), c = (int)(gid % d4);
    if (t >= G + T_r[b] + 2 - drop) return;
    y[((long long)off_r[b] + t) * d4 + c] = x[((long long)b * n + lp_r[b] + t) * d4 + c];
}

int launch_lm_score_gather(float* y, const float* x, int B, int n, int d, int G, int Lt_max, const int* lp_r, const int* T_r, const int* off_r,
                           hipStream_t s, int drop) {
    QA_REQUIRE(d % 4 == 0 && B >= 1 && B <= 65535 && Lt_max >= 1 && lp_r && T_r && off_r, "lm_score_gather: bad launch");
    const long long total = (long long)Lt_max * (d / 4);
    hipLaunchKernelGGL(lm_score_gather_kernel, dim3((unsigned)ceil_div(total, 256), (unsigned)B), dim3(256), 0, s, reinterpret_cast<float4*>(y),
                       reinterpret_cast<const float4*>(x), n, d / 4, G, Lt_max, lp_r, T_r, off_r, drop);
    QA_LAUNCH_CHECK();
    return QA_OK;
}

// lm_seq_reduce_kernel over packed rows: sequence b owns rows off[b] .. off[b] + Lt_b - 1, Lt_b = G + T[b] + 2 - drop.  The same thread
// ownership and the same fixed LDS tree in double, so a sequence's values equal the rectangular kernel's on its own rows.
__global__ __launch_bounds__(256) void lm_seq_reduce_rows_kernel(const float* __restrict__ row_kl, const int* __restrict__ row_ok, int G,
                                                                 const int* __restrict__ T_r, const int* __restrict__ off_r,
                                                                 double* __restrict__ seq_sum, float* __restrict__ loss_seq,
                                                                 long long* __restrict__ correct_seq, int drop) {
    __shared__ double s_kl[256];
    __shared__ long long s_ok[256];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int Lt = G + T_r[b] + 2 - drop;
    const long long base = off_r[b];
    double kl = 0.0;
    long long ok = 0;
    for (int t = tid; t < Lt; t += 256) {
        kl += (double)row_kl[base + t];
        ok += row_ok[base + t];
    }
    s_kl[tid] = kl;
    s_ok[tid] = ok;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h) {
            s_kl[tid] += s_kl[tid + h];
            s_ok[tid] += s_ok[tid + h];
        }
        __syncthreads();
    }
    if (tid == 0) {
        seq_sum[b] = s_kl[0];
        loss_seq[b] = (float)(s_kl[0] / Lt);
        correct_seq[b] = s_ok[0];
    }
}

int launch_lm_seq_reduce_rows(const float* row_kl, const int* row_ok, int B, int G, const int* T_r, const int* off_r, double* seq_sum,
                              float* loss_seq, long long* correct_seq, hipStream_t s, int drop) {
    QA_REQUIRE(B >= 1 && T_r && off_r, "lm_seq_reduce_rows: bad launch");
    hipLaunchKernelGGL(lm_seq_reduce_rows_kernel, dim3((unsigned)B), dim3(256), 0, s, row_kl, row_ok, G, T_r, off_r, seq_sum, loss_seq,
                       correct_seq, drop);
    QA_LAUNCH_CHECK();
    return QA_OK;
}

// The batch scalars over rows of different lengths: the pooled mean over all `total` = sum Lt_b target rows, sequences in index order.
__global__ void lm_batch_reduce_rows_kernel(const double* __restrict__ seq_sum, const long long* __restrict__ correct_seq, int B,
                                            long long total, float* __restrict__ loss, float* __restrict__ acc) {
    double kl = 0.0;
    long long ok = 0;
    for (int b = 0; b < B; ++b) {
        kl += seq_sum[b];
        ok += correct_seq[b];
    }
    const double n = (double)total;
    *loss = (float)(kl / n);
    *acc = (float)((double)ok / n);
}

int launch_lm_batch_reduce_rows(const double* seq_sum, const long long* correct_seq, int B, long long total, float* loss, float* acc,
                                hipStream_t s) {
    QA_REQUIRE(B >= 1 && total >= 1, "lm_batch_reduce_rows: bad launch");
    hipLaunchKernelGGL(lm_batch_reduce_rows_kernel, dim3(1), dim3(1), 0, s, seq_sum, correct_seq, B, total, loss, acc);
    QA_LAUNCH_CHECK();
    return QA_OK;
}

// ------------------------------------------------------------------------------------------------
// qa_lm_cache_select: one WAVE of row moves of a KV cache [layer][max_batch][max_len][d] (K and V).  Move i copies the first mv.len[i]
// positions of its row (the length of the row it carries rides with the move: stale positions behind it are never copied, and rows of
// different lengths share a launch).  Grid: x covers the longest row of the wave, y = move, z = layer * 2 + {K, V}.
// Row -1 is the cache's spare row [layer][K / V][max_len][d] (lm.cpp plan_cache_moves: it breaks a permutation cycle).  The moves of one
// launch never read a row another move of the launch writes, so the launch is in-place safe; the host orders the waves on the stream.
// Rows are whole 16-byte multiples (d % 32 == 0) and 16-byte aligned.
__global__ __launch_bounds__(256) void kv_row_moves_kernel(float4* __restrict__ kc, float4* __restrict__ vc, float4* __restrict__ spare,
                                                           long long layer4, long long row4, int d4, const KvMoves mv) {
    const int layer = blockIdx.z >> 1, kv = blockIdx.z & 1;
    const int dst = mv.dst[blockIdx.y], src = mv.src[blockIdx.y];
    const long long n4 = (long long)mv.len[blockIdx.y] * d4;
    float4* base = (kv ? vc : kc) + layer * layer4;
    float4* sp = spare + (long long)blockIdx.z * row4;
    const float4* from = src < 0 ? sp : base + src * row4;
    float4* to = dst < 0 ? sp : base + dst * row4;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) to[i] = from[i];
}
int launch_kv_row_moves(float* kc, float* vc, float* spare, int n_layers, int max_batch, int max_len, int d, const KvMoves& mv, hipStream_t s) {
    QA_REQUIRE(mv.n >= 1 && mv.n <= KV_MOVES_MAX && d % 4 == 0, "kv_row_moves: bad launch");
    int longest = 0;
    for (int i = 0; i < mv.n; ++i) {
        QA_REQUIRE(mv.dst[i] >= -1 && mv.dst[i] < max_batch && mv.src[i] >= -1 && mv.src[i] < max_batch && mv.dst[i] != mv.src[i],
                   "kv_row_moves: move %d -> %d outside the cache's %d rows", mv.src[i], mv.dst[i], max_batch);
        QA_REQUIRE(mv.len[i] >= 0 && mv.len[i] <= max_len, "kv_row_moves: move %d -> %d of %d positions, the cache holds %d", mv.src[i], mv.dst[i],
                   mv.len[i], max_len);
        longest = std::max(longest, mv.len[i]);
    }
    if (longest == 0) return QA_OK;
    const long long row4 = (long long)max_len * d / 4, n4 = (long long)longest * d / 4;
    // ~8 float4 per thread: enough workgroups to fill the device at one move, few enough that the tail is short
    const unsigned gx = (unsigned)std::min<long long>(ceil_div(n4, 256 * 8), 1024);
    hipLaunchKernelGGL(kv_row_moves_kernel, dim3(gx, (unsigned)mv.n, (unsigned)(2 * n_layers)), dim3(256), 0, s, reinterpret_cast<float4*>(kc),
                       reinterpret_cast<float4*>(vc), reinterpret_cast<float4*>(spare), (long long)max_batch * row4, row4, d / 4, mv);
    QA_LAUNCH_CHECK();
    return QA_OK;
}

}  // namespace qa
