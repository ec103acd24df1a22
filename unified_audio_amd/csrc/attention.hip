// attention.hip - flash-style attention with fp32-class results: one kernel body, attention_kernel, in two
// arithmetic forms (AttForm) - the fp32 chain on the f32 matrix cores and split-6 bf16 planes on the bf16 ones.
//
// Reference semantics: softmax(Q K^T * head_dim^-0.5, fp32) V, no mask for the codec transformers
// (QuarkAudio-HCodec/HCodec-1.0/vq/encoder_modules/transformer.py:158-180) and a causal mask over a KV cache for the
// UniSE Llama layers (QuarkAudio-UniSE/model/llm/llm.py:182-211).  RoPE has already been applied to q / k.
//
// Causal windows and the streaming ring (mimi/transformer.py:212-281,403-413; encoder_modules/transformer.py:437-447):
//   causal = 1            key j visible to query i iff j <= i + off                       (off = n_keys - n_q)
//   context > 0           ... and (i + off) - j < context   (StreamingMultiheadAttention `context`, Transformer `left_context`)
//   ring_end > 0          the keys are the slots of a RingKVCache of capacity n_keys whose write cursor stands at ring_end
//                         (= tokens seen so far, this chunk included): slot s holds position p(s) as RingKVCache.complete()
//                         computes it (-1 = never written), query i sits at q_pos0 + i, visible iff p >= 0 and
//                         0 <= pos_q - p < context.  Slots overwritten by later tokens of the same chunk are gone, as in the
//                         reference (it writes the whole chunk before it attends).
//
// One wave64 owns 32 queries and walks the keys 32 at a time; both products run TRANSPOSED (written here for the fp32 form's
// v_mfma_f32_32x32x2_f32; the split-6 form's operand maps are at AttForm<HD, true>) so that every softmax statistic is per lane (no cross-lane row reductions):
//   S^T[key, q] = sum_d K[key, d] Q[q, d]     A = K tile (LDS, ds_read_b128), B = Q (registers)
//   O^T[d,  q] += sum_key V[key, d] P[q, key] A = V tile (LDS),               B = P = exp(S - m) (registers)
// The 32x32 accumulator layout gives lane (q = lane & 31, h = lane >> 5) the keys (r&3) + 8*(r>>2) + 4*h for r = 0..15,
// which is exactly the k-slot order used for the second product, so P never leaves the registers.
#include "kernels.h"
#include "split_planes.h"

#include <atomic>

#ifdef QA_ATT_TIMING  // tuning builds only (tools/variants.py -DQA_ATT_TIMING=1, read by tools/att_timing.py): shader cycles per phase of the key-tile loop
__device__ unsigned long long g_qa_att_timing[8];  // [0] barriers + LDS stores (incl. the wait for the prefetched tile), [1] S = K Q^T, [2] softmax, [3] O += V P, [4] whole kernel, [5] waves, [6] tiles
#define QA_ATT_TICK(i)                                      \
    {                                                       \
        const long long now_ = __builtin_readcyclecounter(); \
        tacc[i] += now_ - tlast;                            \
        tlast = now_;                                       \
    }
extern "C" int qa_debug_att_timing(unsigned long long* out, int reset) {
    if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(g_qa_att_timing), sizeof(g_qa_att_timing)) != hipSuccess) return -1;  // out[8]
    if (reset) {
        unsigned long long z[8] = {0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_qa_att_timing), z, sizeof(z)) != hipSuccess) return -1;
    }
    return 0;
}
#else
#define QA_ATT_TICK(i)
#endif

namespace qa {

typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));

// The two arithmetic forms.  An AttForm owns everything that depends on the number format: the LDS image of a key tile, the Q fragment,
// the staging store of a fetched tile, and the two products.  attention_kernel below owns the rest and is the same text for both.
// The kernel declares the K and the V image as two __shared__ arrays of K_BYTES / V_BYTES and hands them over: carved out of one array
// the split HD 64 instances spill (profiles/r09_attention_resource_usage.md).
template <int HD, bool SPLIT>
struct AttForm;

// fp32 chain (QA_ATT_MATH = 0, and every UniSE LM launch): v_mfma_f32_32x32x2_f32 on two [32 keys][HD + 4] float tiles.  A tile's
// KMASK validity floats sit in the four padding floats behind each K row, so the other instantiations keep their code and their LDS size.
template <int HD>
struct AttForm<HD, false> {
    static constexpr int MIN_WG = 2;
    static constexpr int LD = HD + 4, DT = HD / 32, NG = HD / 8, NLD = HD / 32;
    static constexpr int K_BYTES = 32 * LD * 4, V_BYTES = 32 * LD * 4;
    float *sK, *sV;
    int ql, hh;
    float qreg[HD / 2];

    __device__ __forceinline__ AttForm(char* k_tile, char* v_tile, int lane, int) : sK((float*)k_tile), sV((float*)v_tile), ql(lane & 31), hh(lane >> 5) {}
    // Q fragment: lane (q, h) keeps d = 8g + 4h + e  ->  qreg[4g + e], scaled by qs
    __device__ __forceinline__ void load_q(const float* qrow, float qs) {
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            const float4 t = *reinterpret_cast<const float4*>(qrow + 4 * hh + 8 * g);
            qreg[4 * g + 0] = t.x * qs; qreg[4 * g + 1] = t.y * qs; qreg[4 * g + 2] = t.z * qs; qreg[4 * g + 3] = t.w * qs;
        }
    }
    __device__ __forceinline__ void stage(const f32x4 (&kreg)[NLD], const f32x4 (&vreg)[NLD], int tid) {
#pragma unroll
        for (int j = 0; j < NLD; ++j) {
            const int i = tid + 256 * j;
            const int row = i / (HD / 4), c4 = (i % (HD / 4)) * 4;
            *reinterpret_cast<f32x4*>(sK + row * LD + c4) = kreg[j];
            *reinterpret_cast<f32x4*>(sV + row * LD + c4) = vreg[j];
        }
    }
    __device__ __forceinline__ float& key_valid(int row) { return sK[row * LD + HD]; }
    // S^T = K Q^T
    __device__ __forceinline__ void scores(f32x16& s) const {
        const float* kp = sK + ql * LD + 4 * hh;
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            const float4 a = *reinterpret_cast<const float4*>(kp + 8 * g);
            s = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, qreg[4 * g + 0], s, 0, 0, 0);
            s = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, qreg[4 * g + 1], s, 0, 0, 0);
            s = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, qreg[4 * g + 2], s, 0, 0, 0);
            s = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, qreg[4 * g + 3], s, 0, 0, 0);
        }
    }
    // O^T += V^T P^T ; k-slot (step st, half h) <-> key (st&3) + 8*(st>>2) + 4*h
    __device__ __forceinline__ void accumulate(f32x16 (&o)[DT], const f32x16& p) const {
#pragma unroll
        for (int st = 0; st < 16; ++st) {
            const int key = (st & 3) + 8 * (st >> 2) + 4 * hh;
            const float* vp = sV + key * LD + ql;
#pragma unroll
            for (int t = 0; t < DT; ++t) o[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(vp[32 * t], p[st], o[t], 0, 0, 0);
        }
    }
};

// Split-6 form (QA_ATT_MATH = 1): the same decomposition with every matrix operand as three exact bf16 planes x = h + m + l
// (split_planes.h) and six v_mfma_f32_32x32x16_bf16 per 16-wide k group, smallest terms first (PAIR_A / PAIR_B, the LDS operand's plane
// first), into one fp32 accumulator: 48 MFMAs of 32 cycles per tile at head dim 64 where the fp32 chain issues 64 of 64 cycles.
//   Q   split once per wave after scale * log2(e) is folded in; lane (q, h) holds d = 16g + 8h + j of k group g (the B operand map).
//   K/V the staging threads split each f32x4 right before the LDS store: per operand three planes of [32 keys][HD] bf16.
//       K rows are HD * 2 + 16 bytes apart (an odd number of 16-byte slots: the ds_read_b128 of a 16-lane group covers all 64 banks);
//       the KMASK validity float sits in the pad of the h plane's row.
//       V rows are 64 bytes (mod 256) apart, so the four rows x 64 bytes a 32-lane half takes with one ds_read_b64_tr_b16 tile the 64
//       banks; V stays row-major [key][d], the transposed read delivers the column-wise A operand (8-byte aligned addresses, EXEC full:
//       the tile skip is a scalar branch).
//   P   accumulator registers 8s .. 8s+7 of S^T are, for lane (q, h), the keys 16s + 8(j >> 2) + 4h + (j & 3), j = 0..7: used as the
//       B fragment of k step s they never leave the registers; the V reads take the same key order (two 4-key blocks per fragment).
//       p lies in [0, 1] (or is NaN): the residuals are finite without split4_rne's tests.
// The summation order is fixed by (tile, k group, plane pair) alone.  dbg bits 32 / 64 / 128 (tests) zero the h / m / l plane of the
// operands selected by bits 256 (Q), 512 (K), 1024 (V), 2048 (P); with none of those four set, of every operand.
template <int HD>
struct AttForm<HD, true> {
    // three workgroups per CU up to HD 64, as the fp32 form gets there (168 VGPRs, no scratch; 768 workgroups of the 32 x 283 x 8 launch
    // are one round of 256 CUs), two above
    static constexpr int MIN_WG = HD <= 64 ? 3 : 2;
    static constexpr int DT = HD / 32, NLD = HD / 32;
    static constexpr int NKG = HD / 16;                                    // 16-wide k groups of S^T = K Q^T
    static constexpr int KS = HD * 2 + 16;                                 // bytes per K row of one plane
    static constexpr int VS = (HD % 64 == 0) ? HD * 2 + 64 : HD * 2;       // bytes per V row of one plane: 64 (mod 256)
    static constexpr int KPLANE = 32 * KS, VPLANE = 32 * VS;
    static constexpr int K_BYTES = 3 * KPLANE, V_BYTES = 3 * VPLANE;
    static_assert(VS % 256 == 64 || VS % 256 == 192, "V rows must be 16 banks apart (mod 64)");
    char *sK, *sV;
    // read addresses.  K fragment of k group g, plane pl: 16 bytes at kread + pl * KPLANE + 32 g.  V fragment of k step s, d tile t:
    // lane 4r + p of a 16-lane group supplies row r, columns 4p .. 4p + 3 of the group's 4-key x 16-d block; blocks at keys
    // 16 s + 8 jh + 4 hh (jh = 0, 1: elements 0..3 and 4..7), d = 32 t + 16 * (group & 1)
    const char *kread, *vread;
    int hh;
    int zq, zk, zv, zp;  // planes to zero (tests), per operand
    bf16x8 qf[3][NKG];

    __device__ __forceinline__ AttForm(char* k_tile, char* v_tile, int lane, int dbg) : sK(k_tile), sV(v_tile), hh(lane >> 5) {
        kread = sK + (lane & 31) * KS + 16 * hh;
        vread = sV + (4 * hh + ((lane & 15) >> 2)) * VS + 32 * ((lane >> 4) & 1) + 8 * (lane & 3);
        const int zpl = (dbg >> 5) & 7, zsel = (dbg >> 8) & 15;  // planes to zero, and of which operands (0: all)
        zq = (zsel == 0 || (zsel & 1)) ? zpl : 0, zk = (zsel == 0 || (zsel & 2)) ? zpl : 0;
        zv = (zsel == 0 || (zsel & 4)) ? zpl : 0, zp = (zsel == 0 || (zsel & 8)) ? zpl : 0;
    }
    __device__ __forceinline__ void load_q(const float* qrow, float qs) {
        const float* qp = qrow + 8 * hh;
#pragma unroll
        for (int g = 0; g < NKG; ++g) {
            u32x2 p0[3], p1[3];
            split4_rne(*reinterpret_cast<const f32x4*>(qp + 16 * g) * qs, p0[0], p0[1], p0[2]);
            split4_rne(*reinterpret_cast<const f32x4*>(qp + 16 * g + 4) * qs, p1[0], p1[1], p1[2]);
#pragma unroll
            for (int pl = 0; pl < 3; ++pl) {
                if (zq & (1 << pl)) p0[pl] = p1[pl] = u32x2{0u, 0u};
                qf[pl][g] = frag8(p0[pl], p1[pl]);
            }
        }
    }
    __device__ __forceinline__ void stage(const f32x4 (&kreg)[NLD], const f32x4 (&vreg)[NLD], int tid) {
#pragma unroll
        for (int j = 0; j < NLD; ++j) {
            const int i = tid + 256 * j;
            const int row = i / (HD / 4), c4 = (i % (HD / 4)) * 4;
            u32x2 pk[3], pv[3];
            split4_rne(kreg[j], pk[0], pk[1], pk[2]);
            split4_rne(vreg[j], pv[0], pv[1], pv[2]);
            if (zk | zv) {
#pragma unroll
                for (int pl = 0; pl < 3; ++pl) {
                    if (zk & (1 << pl)) pk[pl] = u32x2{0u, 0u};
                    if (zv & (1 << pl)) pv[pl] = u32x2{0u, 0u};
                }
            }
#pragma unroll
            for (int pl = 0; pl < 3; ++pl) {
                *reinterpret_cast<u32x2*>(sK + pl * KPLANE + row * KS + c4 * 2) = pk[pl];
                *reinterpret_cast<u32x2*>(sV + pl * VPLANE + row * VS + c4 * 2) = pv[pl];
            }
            if (HD >= 96) __builtin_amdgcn_sched_barrier(0);  // one split's temporaries at a time (HD 96: 253 -> 233 VGPRs; HD 128 still spills)
        }
    }
    __device__ __forceinline__ float& key_valid(int row) { return *reinterpret_cast<float*>(sK + row * KS + HD * 2); }
    // S^T = K Q^T
    __device__ __forceinline__ void scores(f32x16& s) const {
#pragma unroll
        for (int g = 0; g < NKG; ++g) {
            bf16x8 kf[3];
#pragma unroll
            for (int pl = 0; pl < 3; ++pl) kf[pl] = *reinterpret_cast<const bf16x8*>(kread + pl * KPLANE + 32 * g);
#pragma unroll
            for (int i = 0; i < 6; ++i) s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[PAIR_A[i]], qf[PAIR_B[i]][g], s, 0, 0, 0);
            if (HD >= 96) __builtin_amdgcn_sched_barrier(0);  // one group's fragments live at a time (register pressure, as above)
        }
    }
    // O^T += V^T P^T, the P planes of each 16-key step split in registers right before its MFMAs
    __device__ __forceinline__ void accumulate(f32x16 (&o)[DT], const f32x16& p) const {
#pragma unroll
        for (int st = 0; st < 2; ++st) {
            bf16x8 pf[3];
            {
                u32x2 p0[3], p1[3];
                const f32x4 x0 = {p[8 * st + 0], p[8 * st + 1], p[8 * st + 2], p[8 * st + 3]};
                const f32x4 x1 = {p[8 * st + 4], p[8 * st + 5], p[8 * st + 6], p[8 * st + 7]};
                split4_unit(x0, p0[0], p0[1], p0[2]);
                split4_unit(x1, p1[0], p1[1], p1[2]);
                if (zp) {
#pragma unroll
                    for (int pl = 0; pl < 3; ++pl)
                        if (zp & (1 << pl)) p0[pl] = p1[pl] = u32x2{0u, 0u};
                }
#pragma unroll
                for (int pl = 0; pl < 3; ++pl) pf[pl] = frag8(p0[pl], p1[pl]);
            }
#pragma unroll
            for (int t = 0; t < DT; ++t) {
                bf16x8 vf[3];
#pragma unroll
                for (int pl = 0; pl < 3; ++pl) {
                    const char* a = vread + pl * VPLANE + 16 * st * VS + 64 * t;
                    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(a));
                    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(a + 8 * VS));
                    const s16x8 w = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                    vf[pl] = __builtin_bit_cast(bf16x8, w);
                }
#pragma unroll
                for (int i = 0; i < 6; ++i) o[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf[PAIR_A[i]], pf[PAIR_B[i]], o[t], 0, 0, 0);
                if (HD >= 96) __builtin_amdgcn_sched_barrier(0);  // as above
            }
        }
    }
};

// One wave per 32 queries, 32-key tiles, both products transposed, base-2 online softmax (file header); SPLIT selects the AttForm.
// BIAS: WavLM's gated relative position bias (transformers WavLMAttention.forward): score(i, j) += gate[b, head, i] *
// relbias[head][clamp(j - i, -R, R) + R]; the bucket function saturates below R, so the clamp is exact.
// KMASK: key-padding mask (Conformer condition encoder, conformer.py:165-174): kvalid [B, n_keys] bytes, 0 = the key is invisible to
// every query of its batch item.  A tile's validity bytes travel with its K rows (register-staged, unconditional loads) and sit in
// the padding behind each K row in LDS (AttForm::key_valid).
// gate / relbias / R are read only with BIAS, kvalid only with KMASK.
// RAGGED: a causal chunk over a KV cache whose items differ in length (a qa_lm_cache session).  Item b holds
// row_pos0[b] cached keys and row_nq[b] <= n_q live query rows: its counts nq / nk replace the launch's in every test below, while n_q
// stays the row count of the q / out layout.  A (sequence, head) belongs to one workgroup column that starts at key 0, so an item's walk
// never depends on its neighbours; query rows behind nq are written as exact zeros, and a workgroup with no live query only does that.
// row_pos0 / row_nq are read only with RAGGED: every other instantiation keeps its code.
template <int HD, bool BIAS, bool KMASK, bool SPLIT, bool RAGGED = false>
__global__ __launch_bounds__(256, (AttForm<HD, SPLIT>::MIN_WG)) void attention_kernel(const float* __restrict__ q, long long ldq,
                                                        const float* __restrict__ k, const float* __restrict__ v,
                                                        long long ldkv, long long kv_bstride, float* __restrict__ out,
                                                        long long ldo, int n_q, int n_keys, float scale, int causal,
                                                        const float* __restrict__ gate, const float* __restrict__ relbias, int R,
                                                        int context, int q_pos0, int ring_end, int dbg_arg,
                                                        const unsigned char* __restrict__ kvalid,
                                                        const int* __restrict__ row_pos0, const int* __restrict__ row_nq) {
#if defined(QA_ATT_DBG) && QA_ATT_DBG == 0
    constexpr int dbg = 0;
    (void)dbg_arg;
#else
    const int dbg = dbg_arg;
#endif
    using Form = AttForm<HD, SPLIT>;
    constexpr int DT = HD / 32;
    __shared__ __attribute__((aligned(16))) char sK[Form::K_BYTES];
    __shared__ __attribute__((aligned(16))) char sV[Form::V_BYTES];

    // `wave` through readfirstlane: every wave-level test below (tile skips, mask tests) is then a SCALAR branch.  As a VGPR value
    // hipcc lowers them to exec-masked regions, and exec-masked VMEM next to register-staged prefetches is where ROCm 7.2 mis-tracks
    // outstanding loads (see fetch()).
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ql = lane & 31, hh = lane >> 5;
    const int b = blockIdx.z, head = blockIdx.y;
    const int q_blk0 = blockIdx.x * 128;
    const int qi = q_blk0 + wave * 32 + ql;
    const int nq = RAGGED ? row_nq[b] : n_q;              // live queries and keys of this item
    const int nk = RAGGED ? row_pos0[b] + nq : n_keys;
    if (RAGGED && q_blk0 >= nq) {  // workgroup-uniform, before the first barrier: no live query here (an idle item, or a block behind nq)
        if (qi < n_q) {
            float* op = out + ((long long)b * n_q + qi) * ldo + head * HD + 4 * hh;
#pragma unroll
            for (int t = 0; t < HD / 32; ++t)
#pragma unroll
                for (int c = 0; c < 4; ++c) *reinterpret_cast<float4*>(op + 32 * t + 8 * c) = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        return;
    }
    const int off = nk - nq;  // causal: key j visible iff j <= qi + off

    // The softmax runs in base 2: scale * log2(e) is folded into Q once, so that a score needs no multiply and an exponential is the
    // single v_exp_f32 instruction (ocml's expf is ~10 instructions, and a vector instruction issued beside the other waves' MFMAs
    // costs ~30 cycles, conv_gemm.hip)
    constexpr float LOG2E = 1.4426950408889634f;
    Form form(sK, sV, lane, dbg);
    form.load_q(q + ((long long)b * n_q + (qi < nq ? qi : nq - 1)) * ldq + head * HD, scale * LOG2E);

    float gate_q = 0.f;
    const float* rb = nullptr;
    if (BIAS) {
        gate_q = LOG2E * gate[((long long)b * gridDim.y + head) * n_q + (qi < n_q ? qi : n_q - 1)];
        rb = relbias + (long long)head * (2 * R + 1) + R;
    }

    f32x16 o[DT];
#pragma unroll
    for (int t = 0; t < DT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[t][r] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;

    const float* kb = k + (long long)b * kv_bstride + head * HD;
    const float* vb = v + (long long)b * kv_bstride + head * HD;

    const bool ring = ring_end > 0;
    const bool lin_causal = causal && !ring;
    int last_key = nk - 1, first_key = 0;
    if (lin_causal) {
        const int q_last = min(q_blk0 + 127, nq - 1);
        last_key = min(last_key, q_last + off);
        if (context > 0) first_key = max(0, q_blk0 + off - context + 1);
    }
    const int n_tiles = last_key / 32 + 1, kt0 = first_key / 32;
    const int wave_last_key = lin_causal ? min(nk - 1, min(q_blk0 + wave * 32 + 31, nq - 1) + off) : nk - 1;
    const int wave_first_key = (lin_causal && context > 0) ? max(0, q_blk0 + wave * 32 + off - context + 1) : 0;
    const int ring_idx = ring ? ring_end % n_keys : 0;  // RingKVCache.complete(): end_index

    // K / V tiles go global -> registers -> (split ->) LDS; the loads of tile kt + 1 are issued right after tile kt is in LDS and stay
    // in flight under its MFMAs (the first version loaded synchronously: one exposed L2 / HBM round trip per 32 keys)
    // Rows past n_keys re-read the last valid row instead of being predicated off: their scores are masked to -inf below (need_mask
    // is set on any tile that reaches n_keys) and their probability is exactly 0, so a finite stand-in row changes nothing - and
    // every load of the kernel is UNCONDITIONAL.  The round-2 form (`if (key < n_keys) load; else zeros`) put the prefetch into an
    // exec-masked region; with it hipcc (ROCm 7.2) re-used the staging registers while the loads were still in flight for
    // HD = 64 at n_keys = 1500: half of all outputs differed from run to run (tools/diag_attention.py on a build of that form,
    // profiles/r03_attention_determinism.txt).  Caught by the at-size parity test of H-Codec 2.0 (tests/test_at_size_gpu.py).
    constexpr int NLD = HD / 32;  // float4 per thread per operand: 32 keys x HD floats over 256 threads
    // native vector type, NOT float4: with float4 staging arrays hipcc funnels the unconditional loads through ONE temporary register
    // quad into AGPRs for HD >= 96 (global_load; s_waitcnt vmcnt(0); v_accvgpr_write - eight serialized round trips per tile: 110 -> 177 us
    // per launch at HD = 128); ext_vector_type values stay in VGPRs and the loads stay in flight
    f32x4 kreg[NLD], vreg[NLD];
    float mreg = 1.f;
    const unsigned char* kvb = KMASK ? kvalid + (long long)b * n_keys : nullptr;
    auto fetch = [&](int kt) {
        if (KMASK) mreg = kvb[min(kt * 32 + (tid & 31), nk - 1)] ? 1.f : 0.f;
#pragma unroll
        for (int j = 0; j < NLD; ++j) {
            const int i = tid + 256 * j;
            const int row = i / (HD / 4), c4 = (i % (HD / 4)) * 4;
            const int key = min(kt * 32 + row, nk - 1);
            kreg[j] = *reinterpret_cast<const f32x4*>(kb + (long long)key * ldkv + c4);
            vreg[j] = *reinterpret_cast<const f32x4*>(vb + (long long)key * ldkv + c4);
        }
    };
#ifdef QA_ATT_TIMING
    long long tacc[4] = {0, 0, 0, 0};
    long long tlast = __builtin_readcyclecounter();
    const long long tbegin = tlast;
    long long n_done = 0;
#endif
    fetch(kt0);
    for (int kt = kt0; kt < n_tiles; ++kt) {
        QA_ATT_TICK(3)  // (the tail of the previous tile's PV phase; the first time: the Q prologue, negligible)
        __syncthreads();  // the previous tile is no longer read
        form.stage(kreg, vreg, tid);
        if (KMASK && tid < 32) form.key_valid(tid) = mreg;
        __syncthreads();
        if (kt + 1 < n_tiles) fetch(kt + 1);
        if (dbg & 4) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        // the extra barrier stands before the tile skip: every wave of the workgroup reaches it on every tile (after the PV phase, a wave
        // that skipped the tile missed it, so the workgroup's barriers paired up across tiles and LDS tiles were overwritten under readers)
        if (dbg & 2) __syncthreads();
        QA_ATT_TICK(0)
        // wave-uniform skips: the whole tile is masked for this wave, or the wave owns no query at all (the last query block of a
        // sequence that is not a multiple of 128: at N = 283 three of the four waves of block 3 would multiply clamped rows)
        if (!(dbg & 8) && (kt * 32 > wave_last_key || kt * 32 + 31 < wave_first_key || q_blk0 + wave * 32 >= nq)) continue;

        f32x16 s;
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = 0.f;
        form.scores(s);
        QA_ATT_TICK(1)
        // online softmax in base 2 (per lane = per query; the two halves of the wave hold interleaved key groups).  Masks are
        // evaluated only on tiles that can contain a hidden key for some query of this wave (wave-uniform test).
        const int q_first = q_blk0 + wave * 32, q_last = q_first + 31;
        const bool need_mask = KMASK || (dbg & 16) || ring || kt * 32 + 31 >= nk ||
                               (lin_causal && (kt * 32 + 31 > q_first + off || (context > 0 && kt * 32 < q_last + off - context + 1)));
        float tmax = -INFINITY;
        if (BIAS || need_mask) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int key = kt * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
                bool ok = key < nk;
                if (KMASK) ok = ok && form.key_valid((r & 3) + 8 * (r >> 2) + 4 * hh) != 0.f;
                if (ring) {
                    const int delta = key - ring_idx;
                    const int pos = key >= ring_end ? -1 : (delta <= 0 ? ring_end + delta : ring_end + delta - n_keys);
                    const int dq = q_pos0 + qi - pos;
                    ok = ok && pos >= 0 && dq >= 0 && dq < context;
                } else if (causal) {
                    ok = ok && key <= qi + off && (context <= 0 || qi + off - key < context);
                }
                float sc = s[r];
                if (BIAS) sc += gate_q * rb[max(-R, min(R, key - qi))];
                s[r] = ok ? sc : -INFINITY;
            }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) tmax = fmaxf(tmax, s[r]);
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
        const float m_new = fmaxf(m_run, tmax);
        const float m_use = (m_new == -INFINITY) ? 0.f : m_new;
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_use);  // m_run = -inf -> 0
        float psum = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            s[r] = __builtin_amdgcn_exp2f(s[r] - m_use);
            psum += s[r];
        }
        psum += __shfl_xor(psum, 32, 64);
        l_run = l_run * alpha + psum;
        m_run = m_new;
        if ((dbg & 1) || __any(alpha != 1.f)) {  // the running maximum moved for some query of the wave: rescale (rare after the first tiles)
#pragma unroll
            for (int t = 0; t < DT; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) o[t][r] *= alpha;
        }
        QA_ATT_TICK(2)
        form.accumulate(o, s);
#ifdef QA_ATT_TIMING
        ++n_done;
#endif
    }
#ifdef QA_ATT_TIMING
    QA_ATT_TICK(3)
    if (lane == 0) {
        for (int i = 0; i < 4; ++i) atomicAdd(&g_qa_att_timing[i], (unsigned long long)tacc[i]);
        atomicAdd(&g_qa_att_timing[4], (unsigned long long)(tlast - tbegin));
        atomicAdd(&g_qa_att_timing[5], 1ULL);
        atomicAdd(&g_qa_att_timing[6], (unsigned long long)n_done);
    }
#endif

    if (qi < n_q) {
        // a query with no visible key (possible in the ring mode: a chunk as long as the ring overwrites everything its first query
        // could see, and the slot at the write cursor is masked) yields 0, as torch >= 2.5's scaled_dot_product_attention does for
        // a fully masked row - the convention the oracle and the reference-generated golden were produced under
        const float inv = l_run > 0.f ? 1.f / l_run : 0.f;
        float* op = out + ((long long)b * n_q + qi) * ldo + head * HD + 4 * hh;
#pragma unroll
        for (int t = 0; t < DT; ++t)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                float4 w;
                w.x = o[t][4 * c + 0] * inv; w.y = o[t][4 * c + 1] * inv;
                w.z = o[t][4 * c + 2] * inv; w.w = o[t][4 * c + 3] * inv;
                if (RAGGED && qi >= nq) w = make_float4(0.f, 0.f, 0.f, 0.f);  // a row of the layout behind the item's count
                *reinterpret_cast<float4*>(op + 32 * t + 8 * c) = w;
            }
    }
}

template <int HD, bool SPLIT>
static auto attention_instance(bool bias, bool kmask) {
    // BIAS and KMASK together: WavLM under a key-padding mask (a ragged qa_ssl_forward_ragged call)
    return kmask ? (bias ? attention_kernel<HD, true, true, SPLIT> : attention_kernel<HD, false, true, SPLIT>)
                 : bias ? attention_kernel<HD, true, false, SPLIT> : attention_kernel<HD, false, false, SPLIT>;
}

static std::atomic<long long> g_att_launches[2];  // by kernel form: [0] fp32 chain, [1] split-6 (qa_debug_att_stats)
static std::atomic<long long> g_att_kmask_launches;  // launches of a KMASK instantiation (qa_debug_att_kmask_launches)

// gate [B, H, n_q] and relbias [H, 2R+1] (both optional, together): gated relative position bias, see attention_kernel.
// Arithmetic: split-6 (SPLIT) unless QA_ATT_MATH = 0 or the caller asks for the fp32 chain (math_fp32: the UniSE LM, whose prefill
// stays consistent with its fp32 decode kernels)
int launch_attention(const AttnArgs& a, hipStream_t s) {
    const bool ragged = a.row_nq != nullptr;  // the items' own counts decide; n_keys is then only the longest item's
    QA_REQUIRE(a.n_q > 0 && a.n_keys > 0 && (!a.causal || a.ring_end > 0 || ragged || a.n_keys >= a.n_q), "attention: n_q=%d n_keys=%d", a.n_q,
               a.n_keys);
    QA_REQUIRE((a.row_pos0 == nullptr) == (a.row_nq == nullptr) &&
                   (!ragged || (a.causal && a.math_fp32 && !a.gate && !a.kvalid && a.context == 0 && a.ring_end <= 0)),
               "attention: per-item lengths are for the plain causal fp32 form (no bias, key mask, window or ring)");
    QA_REQUIRE(a.context >= 0 && (a.context == 0 || a.causal) && (a.ring_end <= 0 || (a.causal && a.context > 0 && !a.gate)),
               "attention: a context window needs causal=1; the ring mode needs causal=1 and context > 0");
    QA_REQUIRE((a.ldq % 4) == 0 && (a.ldkv % 4) == 0 && (a.ldo % 4) == 0, "attention: strides must be multiples of 4");
    QA_REQUIRE((a.gate == nullptr) == (a.relbias == nullptr) && (!a.gate || (a.R >= 0 && !a.causal && a.n_q == a.n_keys)),
               "attention: gate and relbias come together, for non-causal self-attention");
    // the kernel indexes the mask by (item, key) alone and a non-causal query carries no position, so compact queries (n_q != n_keys: the
    // aggregators' read-out layer) take it as self-attention does
    QA_REQUIRE(!a.kvalid || !a.causal, "attention: the key-padding mask is for non-causal attention");
    const bool split = knob(K_ATT_MATH) != 0 && !a.math_fp32;
    const bool bias = a.gate != nullptr, kmask = a.kvalid != nullptr;
    decltype(attention_instance<32, false>(bias, kmask)) kernel;
    switch (a.hd) {
        case 32: kernel = split ? attention_instance<32, true>(bias, kmask) : attention_instance<32, false>(bias, kmask); break;
        case 64: kernel = split ? attention_instance<64, true>(bias, kmask) : attention_instance<64, false>(bias, kmask); break;
        case 96: kernel = split ? attention_instance<96, true>(bias, kmask) : attention_instance<96, false>(bias, kmask); break;
        case 128: kernel = split ? attention_instance<128, true>(bias, kmask) : attention_instance<128, false>(bias, kmask); break;
        default: qa::set_error("attention: head_dim=%d unsupported (32/64/96/128)", a.hd); return QA_ERR_UNSUPPORTED;
    }
    if (ragged) {  // the fp32 form alone, one more flag on the same body
        switch (a.hd) {
            case 32: kernel = attention_kernel<32, false, false, false, true>; break;
            case 64: kernel = attention_kernel<64, false, false, false, true>; break;
            case 96: kernel = attention_kernel<96, false, false, false, true>; break;
            default: kernel = attention_kernel<128, false, false, false, true>; break;
        }
    }
    hipLaunchKernelGGL(kernel, dim3((unsigned)ceil_div(a.n_q, 128), a.H, a.B), dim3(256), 0, s, a.q, a.ldq, a.k, a.v, a.ldkv, a.kv_batch_stride,
                       a.out, a.ldo, a.n_q, a.n_keys, a.scale, a.causal, a.gate, a.relbias, a.R, a.context, a.q_pos0, a.ring_end,
                       (int)knob(K_ATT_DEBUG), a.kvalid, a.row_pos0, a.row_nq);
    QA_LAUNCH_CHECK();
    g_att_launches[split ? 1 : 0].fetch_add(1, std::memory_order_relaxed);
    if (kmask) g_att_kmask_launches.fetch_add(1, std::memory_order_relaxed);
    return QA_OK;
}

}  // namespace qa

// test hook (declared in quarkaudio.h): host-side launches since load by kernel form - out2[0] the fp32 chain, out2[1] split-6; launches
// replayed from a captured graph are not counted
extern "C" int qa_debug_att_stats(int64_t* out2) {
    if (!out2) {
        qa::set_error("qa_debug_att_stats: bad argument");
        return QA_ERR_INVALID;
    }
    for (int i = 0; i < 2; ++i) out2[i] = qa::g_att_launches[i].load(std::memory_order_relaxed);
    return QA_OK;
}

// test hook (not part of the public header): of those launches, the ones that took a key-padding-mask (KMASK) instantiation - the Conformer
// condition encoder's, and the transformers of a ragged H-Codec or SSL front-end call
extern "C" long long qa_debug_att_kmask_launches(void) { return qa::g_att_kmask_launches.load(std::memory_order_relaxed); }

namespace qa {
// split4_unit against split4_rne on caller-provided values: counts the floats whose three planes differ
__global__ void split_unit_check_kernel(const float* __restrict__ x, long long n4, unsigned long long* __restrict__ bad) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    const f32x4 v = *reinterpret_cast<const f32x4*>(x + 4 * i);
    u32x2 a[3], b[3];
    split4_rne(v, a[0], a[1], a[2]);
    split4_unit(v, b[0], b[1], b[2]);
    unsigned diff = 0;
    for (int pl = 0; pl < 3; ++pl)
        for (int e = 0; e < 2; ++e) diff += a[pl][e] != b[pl][e];
    if (diff) atomicAdd(bad, 1ULL);
}
}  // namespace qa

// test hook (not part of the public header): the number of f32x4 groups of x[0 .. n), n % 4 == 0, on which the probability split of the
// split-6 kernel (split4_unit, no finite tests) and split4_rne give different planes; `bad` is one device word, zeroed by the caller
extern "C" int qa_debug_att_split_unit(const float* x, long long n, unsigned long long* bad, void* stream) {
    if (!x || !bad || n <= 0 || (n % 4) != 0) {
        qa::set_error("qa_debug_att_split_unit: bad argument");
        return QA_ERR_INVALID;
    }
    const long long n4 = n / 4;
    hipLaunchKernelGGL(qa::split_unit_check_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), x, n4, bad);
    QA_LAUNCH_CHECK();
    return QA_OK;
}

// what the four hooks below share: the operands, the shape, the scale and the mask mode, as the C ABI spells them
static qa::AttnArgs debug_attn_args(const float* q, long long ldq, const float* k, const float* v, long long ldkv, float* out, long long ldo,
                                    int B, int n_q, int n_keys, long long kv_bstride, int H, int hd, float scale, int causal) {
    qa::AttnArgs a;
    a.q = q; a.ldq = ldq; a.out = out; a.ldo = ldo;
    a.k = k; a.v = v; a.ldkv = ldkv; a.kv_batch_stride = kv_bstride;
    a.B = B; a.n_q = n_q; a.n_keys = n_keys; a.H = H; a.hd = hd;
    a.scale = scale; a.causal = causal;
    return a;
}

// test hook (not part of the public header): non-causal self-attention under a key-padding mask, kvalid [B, n_keys] bytes (the KMASK
// instantiations the Conformer condition encoder launches)
extern "C" int qa_debug_attention_kmask(const float* q, long long ldq, const float* k, const float* v, long long ldkv, float* out, long long ldo,
                                        int B, int n_q, int n_keys, long long kv_bstride, int H, int hd, float scale,
                                        const unsigned char* kvalid, void* stream) {
    qa::AttnArgs a = debug_attn_args(q, ldq, k, v, ldkv, out, ldo, B, n_q, n_keys, kv_bstride, H, hd, scale, 0);
    a.kvalid = kvalid;
    return qa::launch_attention(a, static_cast<hipStream_t>(stream));
}

// test hook (not part of the public header): the gated relative position bias (gate [B, H, n_q], relbias [H, 2R + 1]) under a key-padding
// mask - the BIAS + KMASK instantiations a ragged WavLM call launches
extern "C" int qa_debug_attention_bias_kmask(const float* q, long long ldq, const float* k, const float* v, long long ldkv, float* out,
                                             long long ldo, int B, int n_q, int n_keys, long long kv_bstride, int H, int hd, float scale,
                                             const float* gate, const float* relbias, int R, const unsigned char* kvalid, void* stream) {
    qa::AttnArgs a = debug_attn_args(q, ldq, k, v, ldkv, out, ldo, B, n_q, n_keys, kv_bstride, H, hd, scale, 0);
    a.gate = gate; a.relbias = relbias; a.R = R;
    a.kvalid = kvalid;
    return qa::launch_attention(a, static_cast<hipStream_t>(stream));
}

// test / diagnostic hook (not part of the public header): the attention kernel alone on caller-provided buffers
extern "C" int qa_debug_attention(const float* q, long long ldq, const float* k, const float* v, long long ldkv, float* out, long long ldo,
                                  int B, int n_q, int n_keys, long long kv_bstride, int H, int hd, float scale, int causal, void* stream) {
    return qa::launch_attention(debug_attn_args(q, ldq, k, v, ldkv, out, ldo, B, n_q, n_keys, kv_bstride, H, hd, scale, causal),
                                static_cast<hipStream_t>(stream));
}

// test hook (not part of the public header): the same, with every launch_attention parameter - the WavLM gated relative position
// bias (gate [B, H, n_q], relbias [H, 2R + 1]), the causal window `context` and the ring mode (q_pos0, ring_end)
extern "C" int qa_debug_attention_ex(const float* q, long long ldq, const float* k, const float* v, long long ldkv, float* out,
                                     long long ldo, int B, int n_q, int n_keys, long long kv_bstride, int H, int hd, float scale,
                                     int causal, const float* gate, const float* relbias, int R, int context, int q_pos0, int ring_end,
                                     void* stream) {
    qa::AttnArgs a = debug_attn_args(q, ldq, k, v, ldkv, out, ldo, B, n_q, n_keys, kv_bstride, H, hd, scale, causal);
    a.gate = gate; a.relbias = relbias; a.R = R;
    a.context = context; a.q_pos0 = q_pos0; a.ring_end = ring_end;
    return qa::launch_attention(a, static_cast<hipStream_t>(stream));
}
