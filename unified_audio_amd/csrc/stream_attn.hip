// stream_attn.hip - the two kernels a streaming step of the codec Transformer adds in front of / in place of attention.hip
// (DESIGN.md section 42): RoPE fused with the K/V cache append, and a split-key attention for short chunks over a long key history.
//
// The cache is LINEAR by default (row = position, [B, cap, d] fp32 per layer): the codec Transformer has no bounded context unless
// `left_context` is given, and a window is then a mask over the same rows.  Under a window the same caches can be a RING (the RING
// template forms; arithmetic in ring_geometry.h): position p sits in row p mod cap, row s holds position p(s),
// and the stream has no end.  Splits and tiles stay fixed ranges of PHYSICAL rows, so the property below holds for the ring as well.
//
// attn_short_kernel: a stream step has n = 1 .. 16 queries per (row, head) and up to `cap` keys.  attention_kernel gives such a step
// ONE workgroup per (row, head) with one busy wave that walks every key tile in turn - tens of dependent L2 round trips.  Here the
// keys of a (row, head) are split over workgroups that own FIXED ranges [s L, (s + 1) L), L = attn_short_split_keys(cap) derived
// from the cache capacity and never from the key count (lm_attn_kernel's rule, lm_decode.hip): a key sits in the same split, the
// same 32-key tile and the same lane whatever the offset of the step is, so a step's bits depend on the cache contents and the
// offset alone, not on how the stream was chunked before.  Each split runs a base-2 online softmax over its tiles in fp32 (plain
// FMAs: at M <= 16 the step is bound by launch and memory latency, not by arithmetic) and writes one partial record
// [n][hd | m | l | pad] ; attn_short_merge_kernel combines the records in split order.  A split (or tile) that lies wholly outside
// the window / causal range is skipped; such a split writes the identity record (m = -inf, l = 0, o = 0), which the merge adds as
// exact zeros.
#include <vector>

#include "kernels.h"
#include "ring_geometry.h"

namespace qa {

// ------------------------------------------------------------------------------------------------ RoPE + append
// one thread: one (row, head, pair i < hd / 2) - the rotate-half pairs (i, i + hd / 2) of q and k, and the same two elements of v
// ROWS: item b's t-th row sits at position row_pos0[b] + t and only its first row_nq[b] rows exist - the others
// touch neither q nor the caches, so no row of a cache is written that a later step of that item has not yet replaced, and none at or
// behind `cap` (the host has checked row_pos0[b] + row_nq[b] <= cap)
// RING: position p goes to row p mod cap.  Positions inside the static table (p < table_rows) read it, so a ring
// that has not wrapped gives the bits of the linear form; beyond it the angle is the table builder's own formula (transformer_rope_table):
// fr = (float)p * inv_freq[i] in fp32, cos / sin in double, rounded to float.  Rows of one step may lie millions of positions apart,
// so no rolling window of the table covers them; the double-precision evaluation costs this small kernel little (section 46).
template <bool ROWS, bool RING = false>
__global__ __launch_bounds__(256) void rope_append_kernel(float* __restrict__ qkv, const float* __restrict__ cs, float* __restrict__ kc,
                                                          float* __restrict__ vc, int B, int n, int H, int hd, int pos0, int cap,
                                                          const int* __restrict__ row_pos0, const int* __restrict__ row_nq,
                                                          const float* __restrict__ inv_freq, int table_rows) {
    const int half = hd >> 1;
    const long long total = (long long)B * n * H * half;
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= total) return;
    const int i = (int)(gid % half);
    const int h = (int)((gid / half) % H);
    const long long row = gid / ((long long)half * H);
    const int b = (int)(row / n);
    const int ti = (int)(row - (long long)b * n);
    if (ROWS) {
        pos0 = row_pos0[b];
        if (ti >= row_nq[b] || pos0 < 0 || (!RING && pos0 + ti >= cap)) return;
    }
    const int pos = pos0 + ti;
    float c, s;
    if (!RING || pos < table_rows) {
        c = cs[((long long)pos * half + i) * 2];
        s = cs[((long long)pos * half + i) * 2 + 1];
    } else {
        const float fr = (float)pos * inv_freq[i];
        c = (float)cos((double)fr);
        s = (float)sin((double)fr);
    }
    const int crow = RING ? ring::row_of(pos, cap) : pos;
    const int d = H * hd;
    float* q = qkv + row * 3 * d + h * hd;
    const float* k = q + d;
    const float* v = q + 2 * d;
    const float q1 = q[i], q2 = q[i + half];
    q[i] = q1 * c - q2 * s;
    q[i + half] = q2 * c + q1 * s;
    const float k1 = k[i], k2 = k[i + half];
    const long long dst = ((long long)b * cap + crow) * d + h * hd;
    kc[dst + i] = k1 * c - k2 * s;
    kc[dst + i + half] = k2 * c + k1 * s;
    vc[dst + i] = v[i];
    vc[dst + i + half] = v[i + half];
}

int launch_rope_append(float* qkv, const float* cs, float* kc, float* vc, int B, int n, int H, int hd, int pos0, int cap, hipStream_t s,
                       const int* row_pos0, const int* row_nq, const float* ring_inv_freq) {
    const bool ring = ring_inv_freq != nullptr;
    QA_REQUIRE((row_pos0 == nullptr) == (row_nq == nullptr), "rope_append: per-row positions and counts come together");
    QA_REQUIRE(B >= 1 && n >= 1 && H >= 1 && hd >= 2 && hd % 2 == 0 && pos0 >= 0 && (row_nq || ring || (long long)pos0 + n <= cap),
               "rope_append: rows %d .. %d of a cache of %d rows", pos0, pos0 + n - 1, cap);
    QA_REQUIRE(!ring || (cap >= n && (row_nq || ring::positions_fit(pos0, n))), "rope_append: %d frames at position %d of a ring of %d rows "
               "(positions stay below 2^24)", n, pos0, cap);
    const long long total = (long long)B * n * H * (hd / 2);
    const dim3 grid((unsigned)ceil_div(total, 256));
    const int T = TR_ROPE_POSITIONS;
    if (ring) {
        if (row_nq) hipLaunchKernelGGL((rope_append_kernel<true, true>), grid, dim3(256), 0, s, qkv, cs, kc, vc, B, n, H, hd, 0, cap, row_pos0,
                                       row_nq, ring_inv_freq, T);
        else hipLaunchKernelGGL((rope_append_kernel<false, true>), grid, dim3(256), 0, s, qkv, cs, kc, vc, B, n, H, hd, pos0, cap, row_pos0,
                                row_nq, ring_inv_freq, T);
    } else if (row_nq) {
        hipLaunchKernelGGL((rope_append_kernel<true>), grid, dim3(256), 0, s, qkv, cs, kc, vc, B, n, H, hd, 0, cap, row_pos0, row_nq,
                           ring_inv_freq, T);
    } else {
        hipLaunchKernelGGL((rope_append_kernel<false>), grid, dim3(256), 0, s, qkv, cs, kc, vc, B, n, H, hd, pos0, cap, row_pos0, row_nq,
                           ring_inv_freq, T);
    }
    QA_LAUNCH_CHECK();
    return QA_OK;
}

// ------------------------------------------------------------------------------------------------ short-chunk attention
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int AS_Q = ATTN_SHORT_MAX_Q;  // query slots of a workgroup
constexpr int AS_KT = 32;               // keys per tile
__host__ __device__ constexpr int as_rec(int hd) { return hd + 4; }  // floats of one query's record: o [hd], m, l, 2 pad (16-byte rows)

// Grid (splits, H, B), 256 threads.  Score phase: wave w owns queries 4 w .. 4 w + 3 - lane (key = lane & 31, half = lane >> 5) holds
// key `key` of the tile for queries 4 w + half and 4 w + 2 + half; the softmax statistics are reduced over the 32 lanes of a half.
// PV phase: thread (q = tid >> 4, ct = tid & 15) owns the float4 columns ct and ct + 16 of query q - the same four queries per wave,
// so a wave without a live query (4 w >= n) skips both phases of every tile.
// ROWS: item b = blockIdx.z - workgroup-uniform, two scalar loads - sits at pos0 = row_pos0[b] with nq = row_nq[b]
// live queries of the n query slots of the layout; n_keys = pos0 + nq.  The grid's split count comes from the longest item, so a split
// wholly behind THIS item's keys (every split when n_keys = 0) leaves through the identity-record exit in front of the first barrier.
// Dead queries are never loaded (zeros in sQ) and the merge writes them as 0 without reading a record.
// RING: the caches are rings of `cap` rows and the grid covers all of them.  Row s holds position p(s)
// (ring_geometry.h) of THIS item, whose end is e = pos0 + nq; the rows some query can see form at most two physical intervals, and a
// split or a tile without one is skipped.  A fresh ring is never cleared and after a per-row reset it holds another sequence's rows, so a
// row with p(s) < 0 may hold NaN: its load is redirected to the row of position e - 1, which this step has written.
template <int HD, bool ROWS, bool RING = false>
__global__ __launch_bounds__(256) void attn_short_kernel(const float* __restrict__ q, long long ldq, const float* __restrict__ kc,
                                                         const float* __restrict__ vc, float* __restrict__ part, int n, int pos0, int cap,
                                                         int context, int split_keys, float qscale, const int* __restrict__ row_pos0,
                                                         const int* __restrict__ row_nq) {
    constexpr int LDK = HD + 4;   // K / V rows an odd number of 16-byte slots apart: the ds_read_b128 of 32 keys covers all banks
    constexpr int C4 = HD / 4;    // float4 columns of a head
    constexpr int NLD = HD / 32;  // float4 per thread per operand and tile: 32 keys x HD floats over 256 threads
    constexpr int NC = (C4 + 15) / 16;
    constexpr int RS = as_rec(HD);
    __shared__ __attribute__((aligned(16))) float sK[AS_KT][LDK];
    __shared__ __attribute__((aligned(16))) float sV[AS_KT][LDK];
    __shared__ __attribute__((aligned(16))) float sQ[AS_Q][HD];
    __shared__ float sP[AS_Q][AS_KT + 1];
    __shared__ float sA[AS_Q];

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int sp = blockIdx.x, ns = gridDim.x, head = blockIdx.y, H = gridDim.y, b = blockIdx.z;
    const int d = H * HD;
    int nq = n;  // live queries of this item; n stays the row count of the q / record / out layouts
    if (ROWS) {
        pos0 = max(row_pos0[b], 0);
        nq = min(max(row_nq[b], 0), RING ? n : min(n, cap - pos0));
    }
    const int n_keys = pos0 + nq;  // the item's end e: keys of a linear cache, positions seen of a ring
    // keys some query of the chunk can see, cut to this split's range
    const int lo = context > 0 ? max(0, pos0 - context + 1) : 0;
    int k_begin = max(sp * split_keys, lo), k_end = min((sp + 1) * split_keys, n_keys);
    ring::Intervals iv = {0, {0, 0}, {0, 0}};
    int last_row = 0;  // the row of position e - 1
    if (RING) {
        iv = ring::visible_rows(pos0, nq, context, cap);
        last_row = nq > 0 ? ring::row_of(n_keys - 1, cap) : 0;
        k_begin = sp * split_keys;
        k_end = min((sp + 1) * split_keys, cap);
        if (!ring::intersects(iv, k_begin, k_end)) k_end = k_begin;
    }
    float* rec = part + (((long long)(b * H + head) * ns + sp) * n) * RS;
    if (k_begin >= k_end || (ROWS && nq == 0)) {  // workgroup-uniform, before the first barrier: the identity record
        for (int i = tid; i < n * RS; i += 256) rec[i] = (i % RS == HD) ? -INFINITY : 0.f;
        return;
    }
    int kt0 = k_begin / AS_KT, kt1 = (k_end - 1) / AS_KT;  // tiles sit on multiples of 32 keys and never straddle a split
    auto tile_live = [&](int kt) { return !RING || ring::intersects(iv, kt * AS_KT, kt * AS_KT + AS_KT); };
    if (RING) {  // the split holds a visible row, so both walks end
        while (!tile_live(kt0)) ++kt0;
        while (!tile_live(kt1)) --kt1;
    }

    for (int f = tid; f < AS_Q * C4; f += 256) {
        const int qi = f / C4, c4 = f - qi * C4;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (qi < nq) v = *reinterpret_cast<const f32x4*>(q + ((long long)b * n + qi) * ldq + head * HD + 4 * c4) * qscale;
        *reinterpret_cast<f32x4*>(&sQ[qi][4 * c4]) = v;
    }

    const float* kb = kc + (long long)b * cap * d + head * HD;
    const float* vb = vc + (long long)b * cap * d + head * HD;
    // register-staged tiles, every load unconditional: rows past the last key re-read it (it is written and finite; whatever lies behind
    // it in the cache is not) and are masked below
    f32x4 kreg[NLD], vreg[NLD];
    auto fetch = [&](int kt) {
#pragma unroll
        for (int j = 0; j < NLD; ++j) {
            const int i = tid + 256 * j;
            const int row = i / C4, c4 = i - row * C4;
            long long key = min(kt * AS_KT + row, n_keys - 1);
            if (RING) {
                const int r = min(kt * AS_KT + row, cap - 1);
                key = ring::pos_at(r, n_keys - 1, last_row, cap) >= 0 ? r : last_row;
            }
            kreg[j] = *reinterpret_cast<const f32x4*>(kb + key * d + 4 * c4);
            vreg[j] = *reinterpret_cast<const f32x4*>(vb + key * d + 4 * c4);
        }
    };

    const bool live = 4 * wave < nq;  // wave-uniform
    const int key_l = lane & 31, hh = lane >> 5;
    const int qs[2] = {4 * wave + hh, 4 * wave + 2 + hh};
    float m_run[2] = {-INFINITY, -INFINITY}, l_run[2] = {0.f, 0.f};
    const int pq = tid >> 4, ct = tid & 15;
    f32x4 o[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) o[c] = (f32x4){0.f, 0.f, 0.f, 0.f};

    fetch(kt0);
    for (int kt = kt0, kn; kt <= kt1; kt = kn) {
        kn = kt + 1;  // the next tile with a visible row
        if (RING)
            while (kn <= kt1 && !tile_live(kn)) ++kn;
        __syncthreads();  // the previous tile (and, the first time, nothing) is no longer read
#pragma unroll
        for (int j = 0; j < NLD; ++j) {
            const int i = tid + 256 * j;
            const int row = i / C4, c4 = i - row * C4;
            *reinterpret_cast<f32x4*>(&sK[row][4 * c4]) = kreg[j];
            *reinterpret_cast<f32x4*>(&sV[row][4 * c4]) = vreg[j];
        }
        __syncthreads();
        if (kn <= kt1) fetch(kn);
        if (live) {
            float s[2] = {0.f, 0.f};
#pragma unroll 4  // (fully unrolled hipcc hoists every LDS read in front of the first FMA: 256 VGPRs, one workgroup per CU)
            for (int c4 = 0; c4 < C4; ++c4) {
                const f32x4 kv = *reinterpret_cast<const f32x4*>(&sK[key_l][4 * c4]);
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    const f32x4 qv = *reinterpret_cast<const f32x4*>(&sQ[qs[e]][4 * c4]);
                    s[e] += kv.x * qv.x;
                    s[e] += kv.y * qv.y;
                    s[e] += kv.z * qv.z;
                    s[e] += kv.w * qv.w;
                }
            }
            const int key = kt * AS_KT + key_l;
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int p = pos0 + qs[e];  // the query's position; key <= p implies key < n_keys
                bool ok = qs[e] < nq && key <= p && (context <= 0 || p - key < context);
                if (RING) ok = qs[e] < nq && key < cap && ring::visible(ring::pos_at(min(key, cap - 1), n_keys - 1, last_row, cap), p, context);
                const float sc = ok ? s[e] : -INFINITY;
                float tmax = sc;
#pragma unroll
                for (int x = 16; x > 0; x >>= 1) tmax = fmaxf(tmax, __shfl_xor(tmax, x, 64));
                const float m_new = fmaxf(m_run[e], tmax);
                const float m_use = (m_new == -INFINITY) ? 0.f : m_new;
                const float alpha = __builtin_amdgcn_exp2f(m_run[e] - m_use);  // m_run = -inf -> 0
                const float pr = __builtin_amdgcn_exp2f(sc - m_use);
                float psum = pr;
#pragma unroll
                for (int x = 16; x > 0; x >>= 1) psum += __shfl_xor(psum, x, 64);
                l_run[e] = l_run[e] * alpha + psum;
                m_run[e] = m_new;
                sP[qs[e]][key_l] = pr;
                if (key_l == 0) sA[qs[e]] = alpha;
            }
        }
        __syncthreads();
        if (live) {
            const float a = sA[pq];
#pragma unroll
            for (int c = 0; c < NC; ++c) o[c] *= a;
#pragma unroll 8
            for (int key = 0; key < AS_KT; ++key) {
                const float pr = sP[pq][key];
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    const int col = ct + 16 * c;
                    if (col < C4) o[c] += pr * *reinterpret_cast<const f32x4*>(&sV[key][4 * col]);
                }
            }
        }
    }
    if (live) {
        if (pq < nq) {
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const int col = ct + 16 * c;
                if (col < C4) *reinterpret_cast<f32x4*>(rec + (long long)pq * RS + 4 * col) = o[c];
            }
        }
        if (key_l == 0) {
#pragma unroll
            for (int e = 0; e < 2; ++e)
                if (qs[e] < nq) {
                    rec[(long long)qs[e] * RS + HD] = m_run[e];
                    rec[(long long)qs[e] * RS + HD + 1] = l_run[e];
                }
        }
    }
}

// Grid (H, B), 256 threads: out[b, i, head, :] = sum_s o_s 2^(m_s - M) / sum_s l_s 2^(m_s - M), splits in order
// ROWS: the queries i >= row_nq[b] of item b are written as 0 and their records, which no split has written, are not read
template <int HD, bool ROWS>
__global__ __launch_bounds__(256) void attn_short_merge_kernel(const float* __restrict__ part, float* __restrict__ out, int n, int ns,
                                                               const int* __restrict__ row_nq) {
    constexpr int RS = as_rec(HD);
    const int head = blockIdx.x, H = gridDim.x, b = blockIdx.y;
    const float* rec = part + ((long long)(b * H + head) * ns) * n * RS;
    const int nq = ROWS ? row_nq[b] : n;
    for (int e = threadIdx.x; e < n * HD; e += 256) {
        const int i = e / HD, c = e - i * HD;
        if (ROWS && i >= nq) {
            out[((long long)b * n + i) * H * HD + head * HD + c] = 0.f;
            continue;
        }
        const float* r = rec + (long long)i * RS;
        float M = -INFINITY;
        for (int s = 0; s < ns; ++s) M = fmaxf(M, r[(long long)s * n * RS + HD]);
        const float m_use = (M == -INFINITY) ? 0.f : M;
        float L = 0.f, acc = 0.f;
        for (int s = 0; s < ns; ++s) {
            const float* rs = r + (long long)s * n * RS;
            const float w = __builtin_amdgcn_exp2f(rs[HD] - m_use);
            L += rs[HD + 1] * w;
            acc += rs[c] * w;
        }
        out[((long long)b * n + i) * H * HD + head * HD + c] = L > 0.f ? acc / L : 0.f;
    }
}

// 16 splits of a cache, in whole 64-key steps, between 64 and 256 keys each
int attn_short_split_keys(int cap) { return (int)std::min<int64_t>(256, std::max<int64_t>(64, round_up(ceil_div(cap, 16), 64))); }

size_t attn_short_part_floats(int B, int H, int hd, int n, int cap) {
    return (size_t)B * H * (size_t)ceil_div(cap, attn_short_split_keys(cap)) * n * as_rec(hd);
}

int launch_attention_short(const float* q, long long ldq, const float* kc, const float* vc, float* out, float* part, int B, int n, int H,
                           int hd, int pos0, int cap, int context, hipStream_t s, const int* row_pos0, const int* row_nq, int max_keys,
                           bool ring) {
    QA_REQUIRE((row_pos0 == nullptr) == (row_nq == nullptr) && (!row_nq || ring || (max_keys >= 1 && max_keys <= cap)),
               "attention_short: per-row positions and counts come together, with the key count of the longest row (1 .. %d)", cap);
    if (row_nq) pos0 = ring ? 0 : max_keys - n;  // unused by the kernels; the split count below covers the longest row
    QA_REQUIRE(B >= 1 && H >= 1 && n >= 1 && n <= ATTN_SHORT_MAX_Q && (row_nq || (pos0 >= 0 && (ring || (long long)pos0 + n <= cap))) &&
                   context >= 0 && ldq % 4 == 0,
               "attention_short: %d queries at offset %d of a cache of %d rows (at most %d queries)", n, pos0, cap, ATTN_SHORT_MAX_Q);
    QA_REQUIRE(!ring || (context >= 1 && cap >= ring::min_rows(context, n) && ring::positions_fit(pos0, n)),
               "attention_short: a ring of %d rows under a window of %d keys holds steps of at most %d frames (this one has %d, at position %d; "
               "positions stay below 2^24)", cap, context, cap - context + 1, n, pos0);
    const int L = attn_short_split_keys(cap), ns = (int)ceil_div(ring ? cap : pos0 + n, L);  // a ring: every split, visible rows lie anywhere
    constexpr float LOG2E = 1.4426950408889634f;
    const float qscale = LOG2E / std::sqrt((float)hd);
    const dim3 grid((unsigned)ns, (unsigned)H, (unsigned)B), mgrid((unsigned)H, (unsigned)B);
#define QA_AS_RING(HD_)                                                                                                                   \
    if (row_nq) {                                                                                                                         \
        hipLaunchKernelGGL((attn_short_kernel<HD_, true, true>), grid, dim3(256), 0, s, q, ldq, kc, vc, part, n, 0, cap, context, L,      \
                           qscale, row_pos0, row_nq);                                                                                     \
        hipLaunchKernelGGL((attn_short_merge_kernel<HD_, true>), mgrid, dim3(256), 0, s, part, out, n, ns, row_nq);                       \
    } else {                                                                                                                              \
        hipLaunchKernelGGL((attn_short_kernel<HD_, false, true>), grid, dim3(256), 0, s, q, ldq, kc, vc, part, n, pos0, cap, context, L,  \
                           qscale, row_pos0, row_nq);                                                                                     \
        hipLaunchKernelGGL((attn_short_merge_kernel<HD_, false>), mgrid, dim3(256), 0, s, part, out, n, ns, row_nq);                      \
    }
#define QA_AS(HD_)                                                                                                                        \
    if (ring) {                                                                                                                           \
        QA_AS_RING(HD_)                                                                                                                   \
    } else if (row_nq) {                                                                                                                  \
        hipLaunchKernelGGL((attn_short_kernel<HD_, true>), grid, dim3(256), 0, s, q, ldq, kc, vc, part, n, 0, cap, context, L, qscale,    \
                           row_pos0, row_nq);                                                                                             \
        hipLaunchKernelGGL((attn_short_merge_kernel<HD_, true>), mgrid, dim3(256), 0, s, part, out, n, ns, row_nq);                       \
    } else {                                                                                                                              \
        hipLaunchKernelGGL((attn_short_kernel<HD_, false>), grid, dim3(256), 0, s, q, ldq, kc, vc, part, n, pos0, cap, context, L,        \
                           qscale, row_pos0, row_nq);                                                                                     \
        hipLaunchKernelGGL((attn_short_merge_kernel<HD_, false>), mgrid, dim3(256), 0, s, part, out, n, ns, row_nq);                      \
    }
    switch (hd) {
        case 64: QA_AS(64); break;
        case 96: QA_AS(96); break;
        case 128: QA_AS(128); break;
        default: set_error("attention_short: head_dim=%d unsupported (64/96/128)", hd); return QA_ERR_UNSUPPORTED;
    }
#undef QA_AS
#undef QA_AS_RING
    QA_LAUNCH_CHECK();
    return QA_OK;
}

// RotaryEmbedding of transformer.py:8-74 evaluated in fp32 like the reference: inv [hd / 2] and the (cos, sin) pairs of positions
// 0 .. TR_ROPE_POSITIONS - 1 as [position][hd / 2][2].  rope_append_kernel's RING form restates the inner two lines for later positions.
void transformer_rope_table(int hd, std::vector<float>* cs, std::vector<float>* inv_freq) {
    const int half = hd / 2;
    cs->resize((size_t)TR_ROPE_POSITIONS * half * 2);
    inv_freq->resize((size_t)half);
    for (int i = 0; i < half; ++i) {
        const float expo = (float)(2 * i) / (float)hd;
        const float inv = 1.0f / std::pow(10000.0f, expo);
        (*inv_freq)[(size_t)i] = inv;
        for (int t = 0; t < TR_ROPE_POSITIONS; ++t) {
            const float fr = (float)t * inv;
            (*cs)[((size_t)t * half + i) * 2] = (float)std::cos((double)fr);
            (*cs)[((size_t)t * half + i) * 2 + 1] = (float)std::sin((double)fr);
        }
    }
}

}  // namespace qa

// test hook (tests/test_stream_ring_gpu.py): one rope-append plus attention of n frames per item over caches [B, cap, H hd] the caller
// owns, at positions the caller chooses - pos0 for every item, or device int [B] row_pos0 / row_nq.  ring = 0: the linear forms.
// long_form: attention_kernel instead of the short kernel (rows moving together only; its ring mode wants cap > context - 1 + n and
// every row of the ring finite).  qkv [B n, 3 H hd] is roped in place (q), out [B n, H hd].  Synchronous.
extern "C" int qa_debug_stream_attn(float* qkv, float* kc, float* vc, float* out, int B, int n, int H, int hd, int cap, int context, int ring,
                                    int pos0, const int* row_pos0_dev, const int* row_nq_dev, int long_form, void* stream) {
    using namespace qa;
    QA_REQUIRE(qkv && kc && vc && out, "qa_debug_stream_attn: null argument");
    QA_REQUIRE(B >= 1 && n >= 1 && H >= 1 && (hd == 64 || hd == 96 || hd == 128) && cap >= 1 && cap <= TR_ROPE_POSITIONS && context >= 0 &&
                   pos0 >= 0 && (long long)B * n * H * hd < (1LL << 28),
               "qa_debug_stream_attn: B %d n %d H %d hd %d cap %d context %d pos0 %d", B, n, H, hd, cap, context, pos0);
    QA_REQUIRE((row_pos0_dev == nullptr) == (row_nq_dev == nullptr) && !(long_form && row_nq_dev),
               "qa_debug_stream_attn: per-row positions and counts come together, on the short kernel");
    QA_REQUIRE(!ring || (context >= 1 && cap >= ring::min_rows(context, n) + (long_form ? 1 : 0) && (row_nq_dev || ring::positions_fit(pos0, n))),
               "qa_debug_stream_attn: a ring of %d rows, window %d, %d frames at position %d", cap, context, n, pos0);
    QA_REQUIRE(ring || row_nq_dev || (long long)pos0 + n <= cap, "qa_debug_stream_attn: rows %d .. %d of a linear cache of %d", pos0, pos0 + n - 1, cap);
    QA_REQUIRE(long_form || n <= ATTN_SHORT_MAX_Q, "qa_debug_stream_attn: the short kernel takes at most %d frames", ATTN_SHORT_MAX_Q);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    std::vector<float> cs, inv;
    transformer_rope_table(hd, &cs, &inv);
    const int d = H * hd;
    float *table = nullptr, *part = nullptr;
    QA_HIP(hipMalloc(reinterpret_cast<void**>(&table), sizeof(float) * (cs.size() + inv.size())));
    int rc = long_form ? QA_OK
                       : (hipMalloc(reinterpret_cast<void**>(&part), sizeof(float) * attn_short_part_floats(B, H, hd, n, cap)) == hipSuccess
                              ? QA_OK : QA_ERR_HIP);
    if (rc == QA_OK && (hipMemcpy(table, cs.data(), sizeof(float) * cs.size(), hipMemcpyHostToDevice) != hipSuccess ||
                        hipMemcpy(table + cs.size(), inv.data(), sizeof(float) * inv.size(), hipMemcpyHostToDevice) != hipSuccess))
        rc = QA_ERR_HIP;
    const float* inv_dev = ring ? table + cs.size() : nullptr;
    if (rc == QA_OK) rc = launch_rope_append(qkv, table, kc, vc, B, n, H, hd, pos0, cap, s, row_pos0_dev, row_nq_dev, inv_dev);
    if (rc == QA_OK && long_form) {
        AttnArgs at = attn_packed_qkv(qkv, out, B, n, H, hd);
        at.k = kc; at.v = vc; at.ldkv = d; at.kv_batch_stride = (long long)cap * d;
        at.causal = 1; at.context = context;
        at.n_keys = ring ? cap : pos0 + n;
        if (ring) { at.q_pos0 = pos0; at.ring_end = pos0 + n; }
        rc = launch_attention(at, s);
    } else if (rc == QA_OK) {
        rc = launch_attention_short(qkv, 3 * d, kc, vc, out, part, B, n, H, hd, pos0, cap, context, s, row_pos0_dev, row_nq_dev, cap, ring != 0);
    }
    const hipError_t se = hipStreamSynchronize(s);
    (void)hipFree(table);
    (void)hipFree(part);
    QA_HIP(se);
    return rc;
}
