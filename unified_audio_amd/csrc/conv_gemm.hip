// conv_gemm.hip - implicit-GEMM Conv1d / Linear over channel-last activations on the fp32 matrix cores.
//
// Replaces every Conv1d / Linear of the reference's codec and LM graphs (SURVEY.md 2.2 K1,K2,K5-K7,K10-K13,K17):
//   y[m, n] = post( res[m,n] + gamma[n] * act( silu(gate[m,n]) * (bias[n] + sum_k A[m,k] * W[n,k]) ) )
// where row m = (b, t) of a [B, T_out] grid and A[m, (j, c)] = pro(x[b, src(t, j), c]) is gathered on the fly:
// in channel-last layout the im2col row of a 1-D convolution is `ksize` contiguous C_in-long segments, so no
// im2col buffer and no padded copy ever exist in HBM (reflect / zero padding are resolved per segment).
//
// gfx950 mapping: 256-thread workgroups (4 wave64), block tile BM x BN x 32, each wave owns a grid of 32x32
// accumulators fed by v_mfma_f32_32x32x2_f32 (exact fp32 FMA chain, 157 TFLOP/s peak).  Operands are staged
// global -> registers -> LDS (double buffered, one barrier per K step, next tile's global loads issued before
// the current tile's MFMAs).  LDS rows are padded to 36 floats so that the ds_read_b128 fragment loads are
// bank-conflict free; each lane fetches 4 consecutive k per read and the (lane>>5) halves take k-groups
// {0..3},{4..7}: the K order inside a step is permuted identically for A and B, which leaves the sum unchanged.
// That is the fp32 chain (QA_GEMM_MATH = 0).  The default, split-6 (QA_GEMM_MATH = 1, split4_rne in split_planes.h), runs the same tiles
// on the bf16 matrix pipe: three bf16 planes per operand in LDS and, per 16 x 16 output tile, six v_mfma_f32_16x16x32_bf16 per 32-wide k group.  Two opt-in reduced
// forms keep fewer planes of the same split: split-3 (QA_GEMM_MATH = 2, two planes, three MFMAs) and bf16 (3, one plane, one MFMA).
// Host side: launch_conv_gemm validates and derives the kernel's parameters, choose_tile is the tile cost model, launch_cfg /
// launch_instance map a tile to a kernel instance.  The pre-split weight images the PRE instances read live in weight_planes.hip.
#include <algorithm>
#include <cstdlib>
#include <type_traits>

#include "common.h"
#include "conv_offsets.h"
#include "split_planes.h"

// tuning knobs of tools/variants.py
#ifndef QA_LOAD_AT  // MFMA group of a K chunk that carries the next chunk's global loads
#define QA_LOAD_AT 0
#endif

#ifdef QA_TIMING  // tuning builds only (tools/variants.py, read by tools/gemm_timing.py): shader-cycle totals of the kernel, summed over waves
__device__ unsigned long long g_qa_timing[10];  // [4] epilogue, [5] main loop + epilogue, [6] waves, [7] chunks, [8] the interval of [5] in 100 MHz ticks; the rest unused
extern "C" int qa_debug_timing(unsigned long long* out, int reset) {
    if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(g_qa_timing), sizeof(g_qa_timing)) != hipSuccess) return -1;  // out[10]
    if (reset) {
        unsigned long long z[10] = {0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_qa_timing), z, sizeof(z)) != hipSuccess) return -1;
    }
    return 0;
}
#endif

namespace qa {

// LDS bytes of one conv_gemm configuration (fp32 image with 4-float row padding, or three bf16 planes) and the workgroups per CU that
// the register budget is tuned for.  Split forms: BK = 32 is two buffers of 32 k, BK = 16 one buffer of 32 k - the bytes of two 16-k buffers,
// which is what the formula says
__host__ __device__ constexpr int conv_gemm_lds_bytes(int BM, int BN, int BK, bool split) {
    return (split ? 2 * (BM + BN) * 3 * BK * 2 : 2 * (BM + BN) * (BK + 4) * 4) + BM * 8 * 4;
}
__host__ __device__ constexpr int conv_gemm_min_wg(int BM, int BN, int BK, bool split) {
    const int regs = BM == 256 ? (BK == 16 ? 2 : 1) : (BM == 64 && (BK == 16 || BN == 64) ? 4 : (BK == 16 ? 3 : 2));
    const int lds = 160 * 1024 / conv_gemm_lds_bytes(BM, BN, BK, split);
    return regs < lds ? regs : (lds < 1 ? 1 : lds);
}

template <int N, int I = 0, class F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<N, I + 1>(f);
    }
}

constexpr int TAP_WIN = 8;  // taps per LDS source-frame table window (ksize <= 8: built once per tile)

__device__ __forceinline__ float snake_f(float x, float a) {
    const float s = sinf(a * x);
    return x + s * s / (a + 1e-9f);
}
__device__ __forceinline__ f32x4 snake4(f32x4 v, const float* alpha, int n) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(alpha + n);
    const f32x4 r = {snake_f(v.x, a.x), snake_f(v.y, a.y), snake_f(v.z, a.z), snake_f(v.w, a.w)};
    return r;
}

// epilogue of 4 consecutive output channels of one row: v = acc + bias -> gate -> act -> gamma -> residual -> post_act
__device__ __forceinline__ f32x4 epilogue4(f32x4 v, const ConvParams& p, long long m, int n, f32x4 bias, f32x4 gamma) {
    v += bias;
    if (p.gate) {
        const f32x4 g = *reinterpret_cast<const f32x4*>(p.gate + m * p.ldg + n);
        v.x *= silu_f(g.x); v.y *= silu_f(g.y); v.z *= silu_f(g.z); v.w *= silu_f(g.w);
    }
    if (p.act == ACT_SNAKE) {
        v = snake4(v, p.alpha, n);
    } else if (p.act != ACT_NONE) {
        v.x = apply_act(v.x, p.act); v.y = apply_act(v.y, p.act); v.z = apply_act(v.z, p.act); v.w = apply_act(v.w, p.act);
    }
    if (p.gamma) v *= gamma;
    if (p.res) v += *reinterpret_cast<const f32x4*>(p.res + m * p.ldr + n);
    if (p.post_act == ACT_SNAKE) {
        v = snake4(v, p.alpha, n);
    } else if (p.post_act != ACT_NONE) {
        v.x = apply_act(v.x, p.post_act); v.y = apply_act(v.y, p.post_act); v.z = apply_act(v.z, p.post_act);
        v.w = apply_act(v.w, p.post_act);
    }
    if (p.y2) *reinterpret_cast<f32x4*>(p.y2 + m * p.ldy2 + n) = snake4(v, p.alpha2, n);
    if (p.rope && n < p.rope_n) {  // interleaved pairs (2i, 2i+1): both members of a pair sit in this float4 (n % 4 == 0)
        const int t = p.rope_pos0 + (int)(m % p.rope_T), i = (n % p.rope_hd) >> 1;
        const f32x4 cs = *reinterpret_cast<const f32x4*>(p.rope + ((long long)t * (p.rope_hd >> 1) + i) * 2);  // c_i, s_i, c_i+1, s_i+1
        const f32x4 r = {v.x * cs.x - v.y * cs.y, v.y * cs.x + v.x * cs.y, v.z * cs.z - v.w * cs.w, v.w * cs.z + v.z * cs.w};
        v = r;
    }
    return v;
}

// LINEAR: ksize 1, stride 1, no padding, no input repetition (every Linear / 1x1 of the graphs: most of the FLOPs).  Row m of A is
// x + m * ldx, so the per-chunk source-frame lookup (LDS read, clamp, select, 64-bit address build) and the padding multiply
// disappear from the main loop - about 20 of its ~50 non-MFMA instructions, each of which costs ~30 cycles beside the co-resident
// workgroup's MFMAs.
//
// SPLIT: split-6 math (above).  The staging threads split their activation / weight float4 after the zero-padding mask and the ELU
// prologue and store three bf16 planes.  A staged chunk is always one 32-wide k group (CK = 32): a plane row is 32 bf16 = four 16-byte
// slots, and slot s of row r sits at s ^ (-(r >> 2) & 3).  A fragment read is one ds_read_b128: lane l takes slot l >> 4 of row l & 15 of a
// 16-row tile.  The instruction serves the lane groups {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32; in each, the 16 lanes'
// (row & 3, swizzled slot) pairs are all different - rows 0-3 and 12-15 at slot s, rows 4-11 at slot s ^ 1, XORed with 0, 1 and 3, 2 - so
// they cover all 64 banks (with the 32x32x16 form's s ^ (r >> 2) the same read was 2-way).  Per output element the order is fixed: 32-wide
// k groups ascending, the kept plane pairs of a group in the order above, one MFMA each into one fp32 accumulator - independent of BM, BN,
// BK, LINEAR, PRE, M and the tile order, like the fp32 chain.  K = 16 mod 32: the last group's upper 16 k are stored as zeros in both
// operands (the staging threads re-read the lower half, so no load leaves the operands), which keeps K % 16 == 0 as the contract; in the
// table form the two halves of a group look up their own taps, so C_in % 16 == 0 is enough as well.
// BK names the buffering of a split instance: 32 = two LDS buffers and one barrier per chunk, 16 = one buffer - the LDS bytes of the former
// two 16-k buffers, so the occupancy stays - and two barriers per chunk, the split + stores of the next chunk between them.
//
// PRE (SPLIT only): the weight comes from a pre-split image (p.wp, split_planes.h).  The B tile of a chunk is BN / 4 blocks of
// 48 image units: 4 rows x 4 slots x 3 planes.  A staging thread owns the same unit of every chunk - one 16-byte global
// load, one ds_write_b128, both addresses fixed before the loop - and 16 consecutive lanes write the 256 contiguous (XOR-permuted)
// bytes that one plane of a block occupies in LDS.  The LDS image is byte for byte the one the in-loop split builds.  Instantiated
// for the 128-column tiles only (launch_instance).
//
// NPL: the arithmetic form as a plane count.  0 = the fp32 chain; 3 = split-6; 2 = split-3 and 1 = bf16 (QA_GEMM_MATH = 2 / 3,
// split_planes.h): the staging threads compute and store the first NPL planes only, the fragment reads load those, and a k group issues
// the table's pairs that pair_kept names (3: all six; 2: hm, mh, hh; 1: hh), in the table's order - so the per-element order, and with it the independence of
// BM, BN, BK, LINEAR and the tile order, is the same in every form.  The LDS image keeps the three-plane stride in every form (the l, or
// m and l, rows are simply never touched): the occupancy of these instances is set by registers, and one layout keeps the image path, the
// epilogue staging and conv_gemm_min_wg as they are.  PRE instances read the same image and move only the units of the kept planes.
template <int BM, int BN, int WM, int WN, bool PRO_ELU, int BK = 32, bool LINEAR = false, int NPL = 0, bool PRE = false>
__global__ __launch_bounds__(256, conv_gemm_min_wg(BM, BN, BK, NPL > 0)) void conv_gemm_kernel(const ConvParams p_in) {
    constexpr bool SPLIT = NPL > 0;
    constexpr int NP = SPLIT ? NPL : 3;  // planes moved and read
    static_assert(NPL >= 0 && NPL <= 3, "0 = fp32 chain, else the number of bf16 planes");
    static_assert(SPLIT || !PRE, "a pre-split weight image feeds the bf16-plane instances only");
    ConvParams p = p_in;
    // Split forms stage and consume 32-wide k groups whatever BK says: CK is the k width of a staged chunk.  For them BK names the buffering:
    // 32 = two LDS buffers of 32 k (one barrier per chunk), 16 = ONE buffer of 32 k (the LDS bytes of two 16-k buffers; two barriers per chunk,
    // the co-resident workgroups cover the store phase).
    constexpr int CK = SPLIT ? 32 : BK;
    constexpr bool ONE_BUF = SPLIT && BK == 16;
    constexpr int LDS = BK + 4;
    constexpr int RPP = 256 / (CK / 4);  // rows staged per pass: 8 (32 k) or 4 (16 k) threads cover one row chunk
    constexpr int WTM = BM / WM, WTN = BN / WN;
    constexpr int TM = WTM / 32, TN = WTN / 32;
    constexpr int A_IT = BM / RPP, B_IT = BN / RPP;
    static_assert(WM * WN == 4, "4 waves per workgroup");
    static_assert(TM >= 1 && TN >= 1, "wave tile must hold at least one 32x32 MFMA tile");

    constexpr int SMEM_FLOATS = SPLIT ? (ONE_BUF ? 1 : 2) * (BM + BN) * 3 * CK / 2 : 2 * (BM + BN) * LDS;
    __shared__ __attribute__((aligned(16))) float smem[SMEM_FLOATS];
    __shared__ int s_tap[BM * TAP_WIN];  // source-frame offset (floats, relative to the tile's first clip) of (row, tap); -1 = zero padding
    float* sA = smem;
    float* sB = smem + 2 * BM * LDS;
    // SPLIT image: [buffer][operand A rows, then B rows][plane h, m, l] rows of CK = 32 bf16
    constexpr int PLANE_A = BM * CK * 2, PLANE_B = BN * CK * 2;       // bytes of one plane of one buffer
    constexpr int BUF_BYTES = 3 * (PLANE_A + PLANE_B);
    char* const sbytes = reinterpret_cast<char*>(smem);
    auto swz = [](int row, int slot) { return slot ^ ((0 - (row >> 2)) & 3); };

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int tiles_n = (p.N + BN - 1) / BN;
    // XCD-aware tile order: workgroup b is dispatched to XCD b % 8 (observed, used for speed only).  Give every XCD a
    // contiguous run of tile ids (n fastest inside it) so the A rows an XCD works on stay private to its L2 and the
    // column tiles of W are re-read from that same L2.  Bijective for any grid size.
    int tile = blockIdx.x;
    if (p.xcd_swizzle) {
        const int nwg = gridDim.x, q = nwg >> 3, r = nwg & 7;
        const int xcd = tile & 7, local = tile >> 3;
        tile = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + local;
    }
    int tm_i = tile / tiles_n, tn_i = tile % tiles_n;
    if (p.panel > 0 && tiles_n > p.panel) {
        // 2-D blocking of the tile order (QA_GEMM_PANEL = PW): column panels of PW tiles, row tiles fastest inside a panel, so that the
        // ~96 tiles an XCD has in flight form a ~(96 / PW) x PW block - the bytes they pull through the XCD's L2 scale with
        // rows + columns of the block instead of with one of them
        const int tiles_m = (p.M + BM - 1) / BM;
        const int per_panel = tiles_m * p.panel;
        const int panel = tile / per_panel, r = tile - panel * per_panel;
        const int pw = min(p.panel, tiles_n - panel * p.panel);
        tm_i = r / pw;
        tn_i = panel * p.panel + (r - tm_i * pw);
    }
    const int m0 = tm_i * BM;
    const int n0 = tn_i * BN;

    const int ld_row = tid / (CK / 4);          // 0..RPP-1
    const int ld_c4 = (tid % (CK / 4)) * 4;     // float offset inside the CK-wide K chunk
    // K = 16 mod 32 (split forms): the last chunk's upper 16 k do not exist.  The threads that stage them (ld_hi; bp_hi for the image units,
    // whose slot is tid & 3 in every unit) re-read the lower half instead - always inside the operand - and store zeros, in BOTH operands.
    const bool ld_hi = SPLIT && ld_c4 >= 16, bp_hi = (tid & 2) != 0;
    const bool k_tail = SPLIT && (p.K & 16) != 0;

    // Source-frame table.  The im2col row of output frame t is the ksize frames src(t, j); padding (reflect with the
    // short-input rule of pad1d, or zeros) and repeat_interleave are resolved HERE, once per (row, tap), so that the main
    // loop's address arithmetic is one LDS read per staged row: vector ALU instructions issued beside the other wave's
    // MFMAs cost ~30 cycles each (measured), and the per-chunk resolve used to take as long as the MFMA phase itself.
    // Rows past M are clamped to row M-1 and columns past N to column N-1 (their results are never stored), so every
    // load in the main loop is unconditional.
    // An entry is relative to the FIRST clip of the tile (clip0): (clip - clip0) * T_in * ldx + frame * ldx, below 2^31 by the host's check
    // (conv_offsets.h), so the main loop adds it to ONE base pointer per thread - no pointer per staged row.
    const bool reflect = p.pad_mode == PAD_REFLECT;
    const int ldx_i = (int)p.ldx;
    const int t_virtual = p.T_in * (p.in_rep > 1 ? p.in_rep : 1);
    const int dil = p.dilation > 1 ? p.dilation : 1;
    const int clip0 = m0 / p.T_out;  // m0 < M: every tile has a row
    const unsigned clip_stride = (unsigned)p.T_in * (unsigned)ldx_i;
    auto build_taps = [&](int jbase) {
        for (int e = tid; e < BM * TAP_WIN; e += 256) {
            const int row = e / TAP_WIN, j = jbase + (e % TAP_WIN);
            const int m = min(m0 + row, p.M - 1);
            const int clip = m / p.T_out, t = m - clip * p.T_out;
            int len = t_virtual, lp = p.Lp;
            if (p.lens) {  // launch-uniform: a ragged call, the clip ends at its own length (never past the T_in its rows are laid out for)
                len = min(p.lens[clip] * p.len_mul, t_virtual);
                lp = len <= p.max_pad ? p.max_pad + 1 : len;
            }
            int r = t * p.stride - p.pad_left + j * dil;
            const int rr = r < 0 ? -r : (r >= lp ? 2 * (lp - 1) - r : r);  // = resolve_frame()
            r = reflect ? rr : r;
            const bool ok = r >= 0 && r < len && j < p.ksize;
            const unsigned ru = ok ? (unsigned)r : 0u;
            const unsigned src = __umulhi(ru, p.rep_magic) + ru * p.rep_one;  // = r / in_rep
            s_tap[e] = ok ? (int)((unsigned)(clip - clip0) * clip_stride + src * (unsigned)ldx_i) : -1;
        }
    };
    if (!LINEAR) build_taps(0);
    int jbase = 0;

    // LINEAR: row base + this thread's column offset inside a chunk, per staged row.  Table form: ONE pointer, the tile's first clip + the
    // column offset; staged row i reads line a_tab0 + i * RPP * TAP_WIN of the table (a compile-time stride: the ds_read's immediate)
    const float* a_ptr[LINEAR ? A_IT : 1];
    const int a_tab0 = ld_row * TAP_WIN;
    if constexpr (LINEAR) {
#pragma unroll
        for (int i = 0; i < A_IT; ++i) a_ptr[i] = p.x + (long long)min(m0 + ld_row + RPP * i, p.M - 1) * p.ldx + ld_c4;
    } else {
        a_ptr[0] = p.x + (long long)clip0 * p.T_in * p.ldx + ld_c4;
    }
    const float* b_ptr[B_IT];
    if constexpr (!PRE) {
#pragma unroll
        for (int i = 0; i < B_IT; ++i) {
            const int n = min(n0 + ld_row + RPP * i, p.N - 1);
            b_ptr[i] = p.w + (long long)n * p.K + ld_c4;
        }
    }
    // PRE: unit u = tid + 256 i of the B tile -> (block of 128 / BK rows, plane, row in block, slot)
    constexpr int BP_BLOCK = 16 * NP;  // units of one block that this form moves: its first NP planes
    constexpr int BP_UNITS = BN * CK / 128 * BP_BLOCK, BP_IT = PRE ? BP_UNITS / 256 : 1;
    static_assert(!PRE || (BN == 128 && BP_UNITS % 256 == 0), "the image path exists for the 128-column tiles: every thread moves BP_IT whole units");
    const char* bp_ptr[BP_IT];  // this thread's unit of chunk 0 in the image
    int bp_lds[BP_IT];          // ... and its byte offset in an LDS buffer
    if constexpr (PRE) {
#pragma unroll
        for (int i = 0; i < BP_IT; ++i) {
            const int u = tid + 256 * i, v = u % BP_BLOCK;
            const int pl = v >> 4, slot = v % (CK / 8);
            const int row = u / BP_BLOCK * (128 / CK) + (v & 15) / (CK / 8);
            const int n = min(n0 + row, p.N - 1);
            bp_ptr[i] = static_cast<const char*>(p.wp) + plane_byte_offset((long long)n * p.K + slot * 8, pl);
            bp_lds[i] = 3 * PLANE_A + pl * PLANE_B + row * CK * 2 + swz(row, slot) * 16;
        }
    }
    const int nk = (p.K + CK - 1) / CK;

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    // 32-wide k groups: 16 x 16 accumulators of v_mfma_f32_16x16x32_bf16, the same 64 registers per wave tile
    constexpr int TM16 = WTM / 16, TN16 = WTN / 16;
    f32x4 acc4[SPLIT ? TM16 : 1][SPLIT ? TN16 : 1];
    if constexpr (SPLIT) {
#pragma unroll
        for (int i = 0; i < TM16; ++i)
#pragma unroll
            for (int j = 0; j < TN16; ++j) acc4[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

    // Staging registers of the NEXT K chunk (native vector type: float4 arrays were left as scratch allocas).  Every
    // iteration loads (the last one re-loads chunk nk-1, harmlessly).
    f32x4 a_reg[A_IT], b_reg[B_IT];
    u32x4 bp_reg[BP_IT];  // PRE: plane units instead of b_reg
    // table form: bit A_IT - 1 - i is set when staged row i falls into zero padding - the sign bits of its table entries, shifted in row by
    // row.  The staged value is then SELECTED to +0 at LDS-store time (the load itself is unconditional, from frame 0 of clip0): no inf or
    // NaN in that frame can reach a padded position
    static_assert(A_IT <= 32, "one mask register for the staged rows");
    unsigned a_pad = 0u;

#define QA_LOAD_GLOBAL(KC)                                                                                     \
    {                                                                                                          \
        const int k0_ = (KC) * CK;                                                                             \
        const bool tl_ = k_tail && (KC) == nk - 1;            /* block-uniform: the half chunk of K = 16 mod 32 */ \
        const int kt_ = k0_ - (tl_ && ld_hi ? 16 : 0);        /* its upper-half threads re-read the lower half */  \
        if (LINEAR) {                                                                                          \
            _Pragma("unroll") for (int i = 0; i < A_IT; ++i) a_reg[i] = *reinterpret_cast<const f32x4*>(a_ptr[i] + kt_); \
        } else {                                                                                               \
            const int j0_ = k0_ / p.C_in;                                                                      \
            const int c0_ = k0_ - j0_ * p.C_in;                                                                \
            int j1_ = j0_, c1_ = c0_;                                                                          \
            if (SPLIT && (p.C_in & 16)) { /* block-uniform: the upper 16 k may belong to the next tap */       \
                const int kh_ = tl_ ? k0_ : k0_ + 16;                                                          \
                j1_ = kh_ / p.C_in;                                                                            \
                c1_ = kh_ - j1_ * p.C_in - 16;                                                                 \
            }                                                                                                  \
            if (j1_ >= jbase + TAP_WIN) { /* block-uniform; only for ksize > TAP_WIN */                        \
                jbase = j0_;                                                                                   \
                build_taps(jbase);                                                                             \
                __syncthreads();                                                                               \
            }                                                                                                  \
            const int j_ = ld_hi ? j1_ : j0_, c_ = ld_hi ? c1_ : c0_;                                          \
            const int* tab_ = s_tap + (a_tab0 + (j_ - jbase));                                                 \
            const float* ac_ = a_ptr[0] + c_;                                                                  \
            _Pragma("unroll") for (int i = 0; i < A_IT; ++i) {                                                 \
                const int off_ = tab_[i * RPP * TAP_WIN];                                                      \
                a_pad = __builtin_amdgcn_alignbit(a_pad, (unsigned)off_, 31); /* (a_pad << 1) | sign */        \
                a_reg[i] = *reinterpret_cast<const f32x4*>(ac_ + (unsigned)max(off_, 0));                      \
            }                                                                                                  \
        }                                                                                                      \
        if constexpr (PRE) {                                                                                   \
            const long long bo_ = (long long)(KC) * (CK * 6) - (tl_ && bp_hi ? 2 * PLANE_GROUP_BYTES : 0);     \
            _Pragma("unroll") for (int i = 0; i < BP_IT; ++i)                                                  \
                bp_reg[i] = *reinterpret_cast<const u32x4*>(bp_ptr[i] + bo_);                                  \
        } else {                                                                                               \
            _Pragma("unroll") for (int i = 0; i < B_IT; ++i) b_reg[i] = *reinterpret_cast<const f32x4*>(b_ptr[i] + kt_); \
        }                                                                                                      \
    }
#define QA_STORE_LDS(BUF, KC)                                                                                  \
    { if constexpr (SPLIT) {                                                                                   \
        char* a_ = sbytes + (BUF) * BUF_BYTES;                                                                 \
        const int sl_ = ld_c4 >> 3, in_ = (ld_c4 & 7) * 2;                                                     \
        if (k_tail && (KC) == nk - 1) { /* block-uniform: zeros into the upper 16 k of the half chunk */       \
            const f32x4 z4_ = {0.f, 0.f, 0.f, 0.f};                                                            \
            const u32x4 zu_ = {0u, 0u, 0u, 0u};                                                                \
            _Pragma("unroll") for (int i = 0; i < A_IT; ++i) a_reg[i] = ld_hi ? z4_ : a_reg[i];                \
            if constexpr (PRE) {                                                                               \
                _Pragma("unroll") for (int i = 0; i < BP_IT; ++i) bp_reg[i] = bp_hi ? zu_ : bp_reg[i];         \
            } else {                                                                                           \
                _Pragma("unroll") for (int i = 0; i < B_IT; ++i) b_reg[i] = ld_hi ? z4_ : b_reg[i];            \
            }                                                                                                  \
        }                                                                                                      \
        _Pragma("unroll") for (int i = 0; i < A_IT; ++i) {                                                     \
            f32x4 v = a_reg[i];                                                                                \
            if (!LINEAR && (a_pad >> (A_IT - 1 - i) & 1u)) v = f32x4{0.f, 0.f, 0.f, 0.f};                      \
            if (PRO_ELU) {                                                                                     \
                v.x = elu_f(v.x); v.y = elu_f(v.y); v.z = elu_f(v.z); v.w = elu_f(v.w);                        \
            }                                                                                                  \
            u32x2 h_, m_, l_;                                                                                  \
            split4_planes<NP>(v, h_, m_, l_);                                                                  \
            const int r_ = ld_row + RPP * i, o_ = r_ * CK * 2 + swz(r_, sl_) * 16 + in_;                       \
            *reinterpret_cast<u32x2*>(a_ + o_) = h_;                                                           \
            if constexpr (NP >= 2) *reinterpret_cast<u32x2*>(a_ + PLANE_A + o_) = m_;                          \
            if constexpr (NP == 3) *reinterpret_cast<u32x2*>(a_ + 2 * PLANE_A + o_) = l_;                      \
        }                                                                                                      \
        if constexpr (PRE) {                                                                                   \
            _Pragma("unroll") for (int i = 0; i < BP_IT; ++i)                                                  \
                *reinterpret_cast<u32x4*>(a_ + bp_lds[i]) = bp_reg[i];                                         \
        } else {                                                                                               \
        char* b_ = a_ + 3 * PLANE_A;                                                                           \
        _Pragma("unroll") for (int i = 0; i < B_IT; ++i) {                                                     \
            u32x2 h_, m_, l_;                                                                                  \
            split4_planes<NP>(b_reg[i], h_, m_, l_);                                                           \
            const int r_ = ld_row + RPP * i, o_ = r_ * CK * 2 + swz(r_, sl_) * 16 + in_;                       \
            *reinterpret_cast<u32x2*>(b_ + o_) = h_;                                                           \
            if constexpr (NP >= 2) *reinterpret_cast<u32x2*>(b_ + PLANE_B + o_) = m_;                          \
            if constexpr (NP == 3) *reinterpret_cast<u32x2*>(b_ + 2 * PLANE_B + o_) = l_;                      \
        } }                                                                                                    \
    } else {                                                                                                   \
        float* a_ = sA + (BUF) * BM * LDS;                                                                     \
        float* b_ = sB + (BUF) * BN * LDS;                                                                     \
        _Pragma("unroll") for (int i = 0; i < A_IT; ++i) {                                                     \
            f32x4 v = a_reg[i];                                                                                \
            if (!LINEAR && (a_pad >> (A_IT - 1 - i) & 1u)) v = f32x4{0.f, 0.f, 0.f, 0.f};                      \
            if (PRO_ELU) {                                                                                     \
                v.x = elu_f(v.x); v.y = elu_f(v.y); v.z = elu_f(v.z); v.w = elu_f(v.w);                        \
            }                                                                                                  \
            *reinterpret_cast<f32x4*>(a_ + (ld_row + RPP * i) * LDS + ld_c4) = v;                              \
        }                                                                                                      \
        _Pragma("unroll") for (int i = 0; i < B_IT; ++i)                                                       \
            *reinterpret_cast<f32x4*>(b_ + (ld_row + RPP * i) * LDS + ld_c4) = b_reg[i];                       \
    } }

    __syncthreads();  // tap table visible
    QA_LOAD_GLOBAL(0)
    QA_STORE_LDS(0, 0)
    __syncthreads();

    const int frag_row = lane & 31;
    const int frag_k = (lane >> 5) * 4;
#ifdef QA_TIMING
    const long long tbegin = __builtin_readcyclecounter();
    const unsigned long long rbegin = __builtin_amdgcn_s_memrealtime();  // constant 100 MHz
#endif
    // One K chunk = BK/8 groups of 4*TM*TN MFMAs.  The next chunk's address arithmetic + global loads ride in group 0 and
    // its LDS stores in the last group, pinned there by sched_barriers: a wave's non-MFMA instructions must sit BETWEEN ITS
    // OWN MFMAs.  Bunched before / after the MFMA phase they have to issue while the co-resident workgroup's wave owns the
    // SIMD with back-to-back 64-cycle MFMAs, and then get roughly one issue slot per MFMA (measured: ~55 cycles per
    // instruction, the "address phase" lasted as long as the whole MFMA phase).
    constexpr int NKK = BK / 8;
    if constexpr (SPLIT) {
        // one K chunk = one 32-wide k group: the fragment of a 16-row tile is one ds_read_b128 per plane - lane l reads slot l >> 4 (k 8 (l >> 4) ..
        // + 7) of row l & 15 - and a 16 x 16 accumulator takes the kept plane pairs in the table's order, one v_mfma_f32_16x16x32_bf16 each.
        // The activation fragments of the wave's rows stay for the whole group; the weight fragments come column tile by column tile.  The next
        // chunk's global loads ride in front of the MFMAs.  Two buffers: its split + LDS stores go under the MFMAs from column tile STORE_J on, one barrier
        // per chunk.  ONE_BUF: they wait behind a second barrier - everybody has read the buffer - and the co-resident workgroups cover them.
        // the 256-row tile (8 row tiles per wave) reads its activation fragments in four blocks: all of them beside the staging registers would not
        // fit two workgroups per CU
        constexpr int RB = BM == 256 ? 4 : 1;
        // two buffers: the column tile whose MFMAs carry the next chunk's split + LDS stores.  A 16-cycle MFMA leaves the VALU 8 cycles, so the
        // ~500 issue cycles of a 128 x 128 chunk's split need most of the chunk's 96 MFMAs: under the last of four column tiles the instance ran
        // 10 % behind the 32x32x16 form, from the second on 10 % ahead of it
        constexpr int STORE_J = TN16 > 1 ? 1 : 0;
        const int fr = lane & 15, sl = lane >> 4;
        int a_off[TM16], b_off[TN16];  // byte offsets of this lane's fragments (plane h of buffer 0)
#pragma unroll
        for (int i = 0; i < TM16; ++i) {
            const int r = wm * WTM + i * 16 + fr;
            a_off[i] = r * CK * 2 + swz(r, sl) * 16;
        }
#pragma unroll
        for (int j = 0; j < TN16; ++j) {
            const int r = wn * WTN + j * 16 + fr;
            b_off[j] = 3 * PLANE_A + r * CK * 2 + swz(r, sl) * 16;
        }
        for (int kc = 0; kc < nk; ++kc) {
            const int cur = ONE_BUF ? 0 : kc & 1;
            const int nxt = min(kc + 1, nk - 1);
            const char* base = sbytes + cur * BUF_BYTES;
            QA_LOAD_GLOBAL(nxt)
            // RB row blocks: the activation fragments of TM16 / RB row tiles at a time, the weight fragments read once per block
            static_for<RB>([&](auto rb_c) {
                constexpr int i0 = decltype(rb_c)::value * (TM16 / RB);
                bf16x8 af[NP][TM16 / RB];
#pragma unroll
                for (int pl = 0; pl < NP; ++pl)
#pragma unroll
                    for (int i = 0; i < TM16 / RB; ++i) af[pl][i] = *reinterpret_cast<const bf16x8*>(base + pl * PLANE_A + a_off[i0 + i]);
#pragma unroll
                for (int j = 0; j < TN16; ++j) {
                    bf16x8 bf[NP];
#pragma unroll
                    for (int pl = 0; pl < NP; ++pl) bf[pl] = *reinterpret_cast<const bf16x8*>(base + pl * PLANE_B + b_off[j]);
                    if (!ONE_BUF && i0 + TM16 / RB == TM16 && j == STORE_J) QA_STORE_LDS(cur ^ 1, nxt)
                    // operands swapped as in the fp32 loop below; plane pairs in the order of split_planes.h (PAIR_A: activation, PAIR_B: weight)
                    static_for<6>([&](auto q_c) {
                        constexpr int q = decltype(q_c)::value;
                        if constexpr (pair_kept(q, NP)) {
#pragma unroll
                            for (int i = 0; i < TM16 / RB; ++i)
                                acc4[i0 + i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf[PAIR_B[q]], af[PAIR_A[q]][i], acc4[i0 + i][j], 0, 0, 0);
                        }
                    });
                }
            });
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (ONE_BUF) {
                if (kc + 1 < nk) {  // block-uniform
                    __syncthreads();  // every wave has read chunk kc
                    QA_STORE_LDS(0, nxt)
                    __syncthreads();
                }
            } else {
                __syncthreads();
            }
        }
    } else
    for (int kc = 0; kc < nk; ++kc) {
        const int cur = kc & 1;
        const int nxt = min(kc + 1, nk - 1);
        const float* a = sA + cur * BM * LDS + (wm * WTM + frag_row) * LDS + frag_k;
        const float* b = sB + cur * BN * LDS + (wn * WTN + frag_row) * LDS + frag_k;
        // fragment double buffering: the ds_read_b128 of k-group kk+1 are issued before the MFMAs of group kk
        f32x4 af[2][TM], bf[2][TN];
#pragma unroll
        for (int i = 0; i < TM; ++i) af[0][i] = *reinterpret_cast<const f32x4*>(a + i * 32 * LDS);
#pragma unroll
        for (int j = 0; j < TN; ++j) bf[0][j] = *reinterpret_cast<const f32x4*>(b + j * 32 * LDS);
#pragma unroll
        for (int kk = 0; kk < NKK; ++kk) {
            const int cb = kk & 1, nb = cb ^ 1;
            if (kk < NKK - 1) {
#pragma unroll
                for (int i = 0; i < TM; ++i) af[nb][i] = *reinterpret_cast<const f32x4*>(a + i * 32 * LDS + (kk + 1) * 8);
#pragma unroll
                for (int j = 0; j < TN; ++j) bf[nb][j] = *reinterpret_cast<const f32x4*>(b + j * 32 * LDS + (kk + 1) * 8);
            }
            if (kk == QA_LOAD_AT) QA_LOAD_GLOBAL(nxt)
            if (kk == NKK - 1) QA_STORE_LDS(cur ^ 1, nxt)
            // operands swapped on purpose: the W fragment is the MFMA's row operand and the activation fragment its
            // column operand, so D = (A W^T)^T and every lane ends up with 4 CONSECUTIVE output channels of one output
            // row per register quad -> the epilogue moves float4, not scalars
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(bf[cb][j].x, af[cb][i].x, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(bf[cb][j].y, af[cb][i].y, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(bf[cb][j].z, af[cb][i].z, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(bf[cb][j].w, af[cb][i].w, acc[i][j], 0, 0, 0);
                }
            __builtin_amdgcn_sched_barrier(0);
        }
        __syncthreads();
    }
#ifdef QA_TIMING
    const long long tloop = __builtin_readcyclecounter();
#endif
#undef QA_LOAD_GLOBAL
#undef QA_STORE_LDS

    // Epilogue.  D layout of the 32x32 MFMA with swapped operands: output row m <- lane & 31, output channel
    // n <- (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5): registers 4g..4g+3 are channels 8g + 4h .. +3 of row m.
    // The accumulators take one trip through LDS (the operand buffers are free now) so that (a) global traffic is whole
    // 512-byte row segments per wave, float4 per lane, for the store AND for the fused residual / gate loads, and (b) the
    // bias / gate / activation / gamma / residual code exists once, in a rolled loop - fully unrolled over the 64
    // accumulator registers it was ~20k instructions per kernel and the epilogue alone cost 20 K-chunks of time.
    constexpr int EP_LD = BN + 4;          // staging row stride (floats)
    constexpr int EP_ROWS = WM * 32;       // rows staged per pass
    constexpr int EP_C4 = BN / 4;          // float4 per row
    static_assert(EP_ROWS * EP_LD <= 2 * (BM + BN) * LDS, "epilogue staging must fit in the operand buffers");
    static_assert(256 % EP_C4 == 0, "a thread keeps its column group across iterations");
    static_assert(EP_C4 % 8 == 0, "arg-min epilogue: the 8 lanes of a 32-column group are consecutive lanes of one wave");
    float* stage = smem;
    const int row_l = lane & 31, col_h = 4 * (lane >> 5);
    const int ep_c4 = tid % EP_C4, ep_r0 = tid / EP_C4;
    const int ep_n = n0 + 4 * ep_c4;
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f}, one4 = {1.f, 1.f, 1.f, 1.f};
    f32x4 bias4 = zero4, gamma4 = one4;
    if (p.vec_epi && ep_n < p.N) {
        if (p.bias) bias4 = *reinterpret_cast<const f32x4*>(p.bias + ep_n);
        if (p.gamma) gamma4 = *reinterpret_cast<const f32x4*>(p.gamma + ep_n);
    }
    // compile-time row-tile index: with four row tiles per wave (the 256 x 128 block) hipcc no longer unrolls this loop by pragma and the
    // accumulators - indexed by a run-time i - fell back to scratch memory for the whole kernel
    static_for<TM>([&](auto i_c) {
        constexpr int i = decltype(i_c)::value;
        __syncthreads();  // operand buffers (i = 0) / previous pass (i > 0) no longer read
        if constexpr (SPLIT) {  // 16 x 16 accumulators: row <- lane & 15, channels 4 (lane >> 4) .. + 3
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int j = 0; j < TN16; ++j)
                    *reinterpret_cast<f32x4*>(stage + (wm * 32 + h * 16 + (lane & 15)) * EP_LD + wn * WTN + j * 16 + 4 * (lane >> 4)) = acc4[2 * i + h][j];
        } else {
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 v = {acc[i][j][4 * g], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]};
                *reinterpret_cast<f32x4*>(stage + (wm * 32 + row_l) * EP_LD + wn * WTN + j * 32 + 8 * g + col_h) = v;
            }
        }
        __syncthreads();
#pragma unroll 1
        for (int r = ep_r0; r < EP_ROWS; r += 256 / EP_C4) {
            const long long m = m0 + (r >> 5) * WTM + i * 32 + (r & 31);
            if (p.am_dist) {  // launch-uniform: the RVQ arg-min epilogue (ConvParams::am_*); every lane takes part in the shuffles
                float best = INFINITY;
                int bi = 0x7fffffff;
                if (m < p.M && ep_n < p.N) {
                    const f32x4 sv = *reinterpret_cast<const f32x4*>(stage + r * EP_LD + 4 * ep_c4);
                    const f32x4 e4 = *reinterpret_cast<const f32x4*>(p.am_e2 + ep_n);
                    const float xx = p.am_x2[m];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {  // codes ascend: strict '<' keeps the first minimum
                        const float dist = (xx - 2.f * sv[e]) + e4[e];
                        if (dist < best) {
                            best = dist;
                            bi = ep_n + e;
                        }
                    }
                }
#pragma unroll
                for (int o = 1; o < 8; o <<= 1) {  // the 8 lanes of a 32-column group are consecutive lanes of one wave (EP_C4 % 8 == 0)
                    const float d2 = __shfl_xor(best, o, 64);
                    const int i2 = __shfl_xor(bi, o, 64);
                    if (d2 < best || (d2 == best && i2 < bi)) {
                        best = d2;
                        bi = i2;
                    }
                }
                if ((ep_c4 & 7) == 0 && m < p.M && ep_n < p.N) {
                    p.am_dist[m * p.am_ld + (ep_n >> 5)] = best;
                    p.am_idx[m * p.am_ld + (ep_n >> 5)] = bi;
                }
                continue;
            }
            if (m >= p.M || ep_n >= p.N) continue;
            f32x4 v = *reinterpret_cast<const f32x4*>(stage + r * EP_LD + 4 * ep_c4);
            if (p.vec_epi) {  // N % 4 == 0, every leading dimension and pointer 16-byte aligned
                v = epilogue4(v, p, m, ep_n, bias4, gamma4);
                *reinterpret_cast<f32x4*>(p.y + m * p.ldy + ep_n) = v;
            } else {
                for (int e = 0; e < 4 && ep_n + e < p.N; ++e) {
                    const int n = ep_n + e;
                    float u = v[e] + (p.bias ? p.bias[n] : 0.f);
                    if (p.gate) u = silu_f(p.gate[m * p.ldg + n]) * u;
                    u = apply_act(u, p.act);
                    if (p.gamma) u *= p.gamma[n];
                    if (p.res) u += p.res[m * p.ldr + n];
                    u = apply_act(u, p.post_act);
                    p.y[m * p.ldy + n] = u;
                }
            }
        }
    });
#ifdef QA_TIMING
    if (lane == 0) {
        const long long tend = __builtin_readcyclecounter();
        atomicAdd(&g_qa_timing[4], (unsigned long long)(tend - tloop));   // epilogue
        atomicAdd(&g_qa_timing[5], (unsigned long long)(tend - tbegin));  // main loop + epilogue
        atomicAdd(&g_qa_timing[6], 1ULL);                                 // waves
        atomicAdd(&g_qa_timing[7], (unsigned long long)nk);               // chunks
        atomicAdd(&g_qa_timing[8], __builtin_amdgcn_s_memrealtime() - rbegin);  // same interval as [5] in 100 MHz ticks
    }
#endif
}

// the geometry of a Linear / 1x1 layer (the LINEAR instances), QA_GEMM_LINEAR on; the ELU prologue term stays with each user
static bool is_linear(const ConvParams& p) {
    return knob(K_GEMM_LINEAR) != 0 && p.ksize == 1 && p.stride == 1 && p.pad_left == 0 && p.in_rep <= 1 && p.T_in == p.T_out && p.dilation <= 1;
}

constexpr int prof_cfg(int bm, int bn) {  // PROF_CFG_* of a tile
    return bm == 256 ? PROF_CFG_256x128 : bm == 64 ? (bn == 64 ? PROF_CFG_64x64 : PROF_CFG_64x128) : bn == 32 ? PROF_CFG_128x32 : bn == 64 ? PROF_CFG_128x64 : PROF_CFG_128x128;
}

// QA_GEMM_MATH as the kernel's plane count: 0 = the fp32 chain (also every launch with math_fp32, whatever the knob says), 2 = split-3 (two
// planes), 3 = bf16 (one plane), any other value = split-6 (three planes, the default); the same for every launch whatever its M
static int gemm_planes(const ConvParams& p) {
    const long long math = knob(K_GEMM_MATH);
    return math == 0 || p.math_fp32 ? 0 : math == 2 ? 2 : math == 3 ? 1 : 3;
}

// one (tile, prologue, chunk, addressing) choice in its arithmetic instances
template <int BM, int BN, int WM, int WN, bool ELU, int BK, bool LIN>
static int launch_instance(const ConvParams& p, long long tiles, hipStream_t stream) {
    constexpr bool IMAGE = BN == 128;  // narrower tiles keep the in-loop split: measured slower from an image
    const bool image = IMAGE && p.wp;
    void (*kernel)(const ConvParams) = nullptr;
    switch (gemm_planes(p)) {
        case 0:  // the fp32 chain has no one-buffer ELU instance (takes_bk16 never sends it one)
            if constexpr (!(ELU && BK == 16)) kernel = conv_gemm_kernel<BM, BN, WM, WN, ELU, BK, LIN, 0, false>;
            break;
        case 1: kernel = image ? conv_gemm_kernel<BM, BN, WM, WN, ELU, BK, LIN, 1, IMAGE> : conv_gemm_kernel<BM, BN, WM, WN, ELU, BK, LIN, 1, false>; break;
        case 2: kernel = image ? conv_gemm_kernel<BM, BN, WM, WN, ELU, BK, LIN, 2, IMAGE> : conv_gemm_kernel<BM, BN, WM, WN, ELU, BK, LIN, 2, false>; break;
        default: kernel = image ? conv_gemm_kernel<BM, BN, WM, WN, ELU, BK, LIN, 3, IMAGE> : conv_gemm_kernel<BM, BN, WM, WN, ELU, BK, LIN, 3, false>; break;
    }
    QA_REQUIRE(kernel != nullptr, "conv_gemm: no %dx%d kernel instance for this launch (ELU %d, BK %d)", BM, BN, (int)ELU, BK);
    hipLaunchKernelGGL(kernel, dim3((unsigned)tiles), dim3(256), 0, stream, p);
    return QA_OK;
}

// The K-chunk width of a launch (launch_cfg; choose_tile prices the instance this picks).  For the split forms "BK = 16" is the one-buffer
// instance (32-wide chunks, two barriers each) and "BK = 32" the two-buffer one: same LDS bytes, occupancy and trade-off as the widths below.
// BK = 16 chunks need 45 KB / 35 KB of LDS, so 3-4 workgroups are co-resident per CU (BK = 32: 2) and cover each other's barriers, prologues and
// epilogues: +10..25 % on the K = 512 layers of the aggregator stacks, +3..5 % on K = 768..3072 (per-shape sweep, tools/gemm_bench.py with
// QA_GEMM_BK16=0 / default).  QA_GEMM_BK16 = largest K that takes the BK = 16 variant.
// ... but only when the launch has enough tiles for that co-residency: with about one workgroup per CU nobody covers the exposed latency of the
// next chunk's global loads, which a BK = 16 chunk's 0.45 us of MFMAs is too short to hide (measured: the 144-tile RVQ distance GEMM 1056 x 1024
// x 512 ran 37 us, 2.5 x its MFMA time).  QA_GEMM_BK16_MIN_TILES = fewest tiles that take BK = 16.
// The 256-row tile (r06 experiment, QA_GEMM_256) exists with BK = 16 only: 61 KB of LDS, two workgroups per CU.
// Launches of a two-stream region (GemmLanes, common.h) run beside a sibling of the same shape on the other stream, so the workgroups of the
// two cover each other's loads: the threshold counts the tiles of both.  A half-batch lane of the H-Codec 1.5 bottleneck at 32 x 10 s has 256
// tiles in out_proj and lin2; on the BK = 32 instance (one workgroup per CU) the split gained 0.1 ms per step, on BK = 16 1.3 ms (DESIGN.md
// section 30).  Same bits either way: every instance accumulates an output element over k in the same order.
static thread_local int t_gemm_lanes = 1;
GemmLanes::GemmLanes(int n) : prev(t_gemm_lanes) { t_gemm_lanes = n > 1 ? n : 1; }
GemmLanes::~GemmLanes() { t_gemm_lanes = prev; }
// The ELU prologue has one-buffer instances for the split forms of the 128 x 128 tile only (the 64 x 128 one from the image
// would need scratch); elsewhere it keeps BK = 32.
static bool takes_bk16(int bm, int bn, long long tiles, int K, int C_in, bool elu, bool split) {
    return bm == 256 || (bn >= 64 && (!elu || (bm == 128 && bn == 128 && split)) &&
                         ((K <= knob(K_GEMM_BK16) && tiles * t_gemm_lanes >= knob(K_GEMM_BK16_MIN_TILES)) || C_in % 32 != 0));
}

template <int BM, int BN, int WM, int WN>
static int launch_cfg(const ConvParams& p, hipStream_t stream) {
    QA_REQUIRE(p.prologue == ACT_NONE || p.prologue == ACT_ELU, "conv_gemm: prologue %d unsupported", p.prologue);
    const long long tiles = ceil_div(p.M, BM) * ceil_div(p.N, BN);
    const bool linear = is_linear(p), elu = p.prologue == ACT_ELU;
    const bool bk16 = takes_bk16(BM, BN, tiles, p.K, p.C_in, elu, gemm_planes(p) > 0);
    // the fp32 chain's K loop runs K / BK whole chunks and its table form reads each chunk from ONE tap: a BK that does not divide K (and, with
    // the table, C_in) would drop the tail of K or read past a tap's C_in channels - into the next frame or the next channel group.  The split
    // forms stage 32-wide groups as two 16-wide halves, each from its own tap, and zero-fill the missing half of K = 16 mod 32: multiples of 16
    const int bk = bk16 || gemm_planes(p) > 0 ? 16 : 32;
    const bool table = BM != 256 && (!linear || elu);  // the ELU prologue exists in the table form only
    QA_REQUIRE(p.K % bk == 0 && (!table || p.C_in % bk == 0),
               "conv_gemm: the %dx%d tile's K chunk needs K=%d / C_in=%d to be multiples of %d", BM, BN, p.K, p.C_in, bk);
    // the table's entries are 32-bit offsets from the first clip of a row tile (conv_offsets.h)
    int64_t span = 0;
    QA_REQUIRE(!table || conv_tile_offsets_fit(BM, p.T_out, p.T_in, p.ldx, &span),
               "conv_gemm: a %d-row tile spans %lld floats of x (%lld clips of T_in=%d x ldx=%lld; T_out=%d), limit 2^31", BM, (long long)span,
               (long long)ceil_div(BM, p.T_out) + 1, p.T_in, (long long)p.ldx, p.T_out);
    const bool prof = profile_enabled();
    if (prof) {
        const double n = p.algo_n ? p.algo_n : p.N, k = p.algo_k ? p.algo_k : p.K;
        // algorithmic bytes: every input frame, weight and output element once (+ fused residual / gate reads)
        const double out_elems = p.am_dist ? 2.0 * (double)p.M * p.am_ld + p.M + n  // arg-min epilogue: (dist, idx) per 32 columns + |r|^2 + |e|^2
                                            : (double)p.M * n * (1.0 + (p.res ? 1.0 : 0.0) + (p.gate ? 1.0 : 0.0));
        const double elems = (double)p.B * p.T_in * p.C_in + n * k + out_elems;
        profile_record_begin(prof_cfg(BM, BN), 2.0 * (double)p.M * n * k, 4.0 * elems, stream, &p);
    }
    if constexpr (BM == 256) QA_REQUIRE(linear && !elu, "conv_gemm: the 256 x 128 tile exists for LINEAR layers only");
    constexpr int BK16 = BN >= 64 ? 16 : 32;  // the 32-column tile has no BK = 16 instance (bk16 is false for it)
    int rc = QA_OK;
    if (bk16 && linear && !elu) rc = launch_instance<BM, BN, WM, WN, false, BK16, true>(p, tiles, stream);
    else if constexpr (BM != 256) {  // the 256-row tile has the instance above only
        if (bk16 && elu) {
            QA_REQUIRE(BM == 128 && BN == 128, "conv_gemm: the one-buffer ELU instances exist for the 128 x 128 tile only");  // takes_bk16 agrees
            if constexpr (BM == 128 && BN == 128) rc = launch_instance<BM, BN, WM, WN, true, 16, false>(p, tiles, stream);
        } else if (bk16) rc = launch_instance<BM, BN, WM, WN, false, BK16, false>(p, tiles, stream);
        else if (elu) rc = launch_instance<BM, BN, WM, WN, true, 32, false>(p, tiles, stream);
        else if (linear) rc = launch_instance<BM, BN, WM, WN, false, 32, true>(p, tiles, stream);
        else rc = launch_instance<BM, BN, WM, WN, false, 32, false>(p, tiles, stream);
    }
    if (prof) profile_record_end(stream);
    if (rc != QA_OK) return rc;
    QA_LAUNCH_CHECK();
    return QA_OK;
}

// Tile choice of a launch (a PROF_CFG_* value that has a kernel for this launch): the cheapest of 128 x 128, 64 x 128, 128 x 64 and 64 x 64 under
// a makespan model of the instance launch_cfg would actually launch (DESIGN.md section 24 has the measurements it is fitted to and checked on).
//   - A CU holds w workgroups of an instance (registers and LDS: profiles/r10_conv_gemm_resource_usage.md; 1 .. 5, by tile, BK and arithmetic
//     form), so a round of the machine is 256 w tiles.  `share` launches of this shape run side by side and fill rounds together.
//   - A full round costs w tiles of work, (rows x columns x K) / efficiency each: co-resident workgroups share the CU's matrix pipe.
//   - The last round holds m <= 256 w tiles, ceil(m / 256) on the busiest CU and m / 256 on the average one.  It costs the mean of the two: the
//     busiest CU sets the end, but CUs that run dry early hand their part of the power budget - the bound of these GEMMs - to the others.  Never
//     less than one tile: a lone workgroup still walks its whole K loop.
//   - Every round adds one exposed ramp - first loads, prologue and epilogue that no co-resident workgroup covers - of 0.22 of a 128 x 128
//     tile's time, whatever the tile; and a launch costs about a quarter of a 128 x 128 x 512 tile before its first workgroup runs.
// Efficiencies relative to 128 x 128 at saturation.  Split-6: 0.85 / 0.80 / 0.69 for 64 x 128 / 128 x 64 / 64 x 64, from the M = 16000 layers
// (K = 512 .. 3072, no row padding) of profiles/r07_gemm_tile_sweep.txt, final build: the 64-column tiles split their weights in the K loop and fall
// behind 64 x 128, which reads the image; 8192 x 4096 x 4096 (0.86 / 0.91 / 0.81) ranks them the other way round and misleads on every layer a model
// has.  fp32 chain: round 4's 0.914 / 0.913 / 0.871 (profiles/r04_gemm_tile_sweep.txt).  Ties go to the larger tile (less L2 traffic).  Every
// configuration accumulates an output element over k in the same order, so this choice - which depends on M, i.e. on the batch size - never changes a
// bit (tests/test_kernels_gpu.py::test_conv_gemm_tile_configurations_are_bit_identical).
struct TileQuery {
    long long M, N, K;
    int C_in;
    bool lin, elu, split;  // LINEAR instance without the ELU prologue; ELU prologue; split-6 arithmetic (else the fp32 chain)
    bool image;            // split-6 only: the weight has a pre-split image (QA_GEMM_PRESPLIT), which the 128-column tiles read
    int share;             // launches of this shape that share the device (>= 1)
};
// co-resident workgroups per CU of the instance (tile, K chunk, arithmetic form): the occupancy column of the resource table, which is the same for
// the LINEAR and the table form of an instance
static int workgroups_per_cu(int cfg, bool bk16, bool split) {
    switch (cfg) {
        case PROF_CFG_128x128: return bk16 ? 3 : split ? 1 : 2;
        case PROF_CFG_64x128: return bk16 ? 4 : 2;
        case PROF_CFG_128x64: return bk16 ? 4 : 2;
        case PROF_CFG_64x64: return bk16 ? 5 : split ? 3 : 4;
        case PROF_CFG_256x128: return 2;
        default: return split ? 2 : 3;  // 128 x 32
    }
}
static double tile_cost(const TileQuery& t, int cfg, int bm, int bn, double eff) {
    constexpr double kTile = 128.0 * 128.0, kRamp = 0.22, kLaunch = 0.27 * 512.0;
    const long long tiles = ceil_div(t.M, bm) * ceil_div(t.N, bn);
    const long long w = workgroups_per_cu(cfg, takes_bk16(bm, bn, tiles, (int)t.K, t.C_in, t.elu, t.split), t.split);
    const long long n = tiles * (t.share > 1 ? t.share : 1), cap = 256 * w;
    const long long rounds = ceil_div(n, cap), m = n - (rounds - 1) * cap;
    double last = 0.5 * ((double)ceil_div(m, 256) + (double)m / 256.0);
    if (last < 1.0) last = 1.0;
    return kTile * kLaunch + (double)t.K * ((double)bm * bn / eff * ((double)(w * (rounds - 1)) + last) + kRamp * kTile * (double)rounds);
}
// The round-4 model, kept for split-6 launches WITHOUT a pre-split image: tiles dealt round-robin over 256 CUs, (tiles on the busiest CU) x (work per
// tile) / (round 4's efficiency), a quarter more for a launch that gives a CU at most one workgroup.  The split-6 efficiencies above are those of
// 64 x 128 reading the image; without one it drops to 128 x 64's level (profiles/r07_gemm_tile_sweep.txt, "no image attached"), and with the image
// figures the 4000-row layers lost 4 - 6 % there (profiles/r11_gemm_tile_sweep.txt).  No model loads weights without an image at the default knobs,
// so these launches were not re-fitted and keep the parent's choice.
static double tile_cost_r4(const TileQuery& t, int bm, int bn, double eff) {
    const long long tiles = ceil_div(t.M, bm) * ceil_div(t.N, bn);
    return (double)ceil_div(tiles, 256) * bm * bn / eff * (tiles <= 256 ? 1.25 : 1.0);
}
static int choose_tile(const TileQuery& t) {
    int cfg = (int)knob(K_GEMM_CFG);  // >= 0: forced
    if (cfg < 0) {
        if (t.N <= 32) cfg = PROF_CFG_128x32;
        else if (t.N <= 64) cfg = PROF_CFG_128x64;
        else {
            struct Cand { int cfg, bm, bn; double eff6, eff32; };
            static const Cand cands[] = {{PROF_CFG_128x128, 128, 128, 1.0, 1.0}, {PROF_CFG_64x128, 64, 128, 0.85, 0.914},
                                         {PROF_CFG_128x64, 128, 64, 0.80, 0.913}, {PROF_CFG_64x64, 64, 64, 0.69, 0.871}};
            double best = 0.0;
            cfg = PROF_CFG_128x128;
            const long long eff256 = knob(K_GEMM_256);  // 0: never; else the tile's efficiency relative to 128 x 128, in 1/1000
            const bool r4 = t.split && !t.image;
            if (eff256 > 0 && t.lin && t.M >= 8000 && t.N >= 1024) {  // try the 256 x 128 tile in front of the 128 x 128 one
                best = r4 ? tile_cost_r4(t, 256, 128, eff256 / 1000.0) : tile_cost(t, PROF_CFG_256x128, 256, 128, eff256 / 1000.0);
                cfg = PROF_CFG_256x128;
            }
            for (const Cand& c : cands) {
                const double cost = r4 ? tile_cost_r4(t, c.bm, c.bn, c.eff32) : tile_cost(t, c.cfg, c.bm, c.bn, t.split ? c.eff6 : c.eff32);
                if (best == 0.0 || cost < best * 0.995) {
                    best = cost;
                    cfg = c.cfg;
                }
            }
        }
    }
    // only BK = 32 exists for the 128 x 32 tile: C_in % 32 != 0 (possible only when forced, N > 32) takes 128 x 64
    if (cfg == PROF_CFG_128x32 && t.C_in % 32 != 0) return PROF_CFG_128x64;
    // a forced 256 x 128 on a layer it does not exist for, or a forced value that names no tile
    if ((cfg == PROF_CFG_256x128 && !t.lin) || cfg >= PROF_NCFG) return PROF_CFG_128x128;
    return cfg;
}
static int choose_tile(const ConvParams& p) {
    const bool elu = p.prologue == ACT_ELU;
    return choose_tile(TileQuery{p.M, p.N, p.K, p.C_in, is_linear(p) && !elu, elu, knob(K_GEMM_MATH) != 0 && !p.math_fp32, p.wp != nullptr, 1});
}

int launch_conv_gemm(const ConvParams& p, hipStream_t stream) {
    // fp32 chain: a K chunk never straddles two taps, so C_in must be a multiple of the chunk width (16 for the BK = 16 variants, which exist for
    // N > 32 without the ELU prologue - e.g. the 48-channel groups of the SSL positional convolution; 32 otherwise).  The split forms take any
    // multiple of 16 in every instance: the 16-wide halves of a k group look up their own taps, and a missing last half is zero-filled
    QA_REQUIRE(p.K % 16 == 0 && p.C_in % 16 == 0, "conv_gemm: K=%d / C_in=%d must be multiples of 16", p.K, p.C_in);
    QA_REQUIRE(p.C_in % 32 == 0 || gemm_planes(p) > 0 || (p.N > 32 && p.prologue != ACT_ELU),
               "conv_gemm: C_in=%d is not a multiple of 32 (the fp32 chain supports that only for N > 32 without the ELU prologue)", p.C_in);
    QA_REQUIRE((p.ldx % 4) == 0, "conv_gemm: ldx=%lld must be a multiple of 4 floats", p.ldx);
    QA_REQUIRE((long long)p.T_in * p.ldx < (1LL << 31), "conv_gemm: one batch item spans %lld floats (limit 2^31)",
               (long long)p.T_in * p.ldx);
    QA_REQUIRE(((uintptr_t)p.x % 16) == 0 && ((uintptr_t)p.w % 16) == 0, "conv_gemm: x / w must be 16-byte aligned");
    if (p.M <= 0 || p.N <= 0) return QA_OK;
    QA_REQUIRE(ceil_div(p.M, 64) * ceil_div(p.N, 32) < (1LL << 31), "conv_gemm: grid too large");
    auto al16 = [](const void* ptr) { return ((uintptr_t)ptr % 16) == 0; };
    const bool vec_epi = p.N % 4 == 0 && p.ldy % 4 == 0 && al16(p.y) && (!p.bias || al16(p.bias)) && (!p.gamma || al16(p.gamma)) &&
                         (!p.res || (p.ldr % 4 == 0 && al16(p.res))) && (!p.gate || (p.ldg % 4 == 0 && al16(p.gate)));
    QA_REQUIRE(p.in_rep <= 1 || p.pad_mode == PAD_ZERO, "conv_gemm: in_rep needs zero padding");
    const bool snake = p.act == ACT_SNAKE || p.post_act == ACT_SNAKE;
    QA_REQUIRE((!snake && !p.y2) || (vec_epi && (!snake || (p.alpha && al16(p.alpha))) &&
                                     (!p.y2 || (p.alpha2 && al16(p.alpha2) && al16(p.y2) && p.ldy2 % 4 == 0))),
               "conv_gemm: Snake activation / second output need the float4 epilogue and 16-byte aligned alpha vectors");
    QA_REQUIRE(p.dilation <= 1 || (p.pad_mode == PAD_ZERO && p.in_rep <= 1), "conv_gemm: dilation needs zero padding");
    // with in_rep > 1 (zero padding only, above) len_mul counts VIRTUAL frames: build_taps cuts r at lens[b] * len_mul before r / in_rep
    QA_REQUIRE(!p.lens || (p.len_mul >= 1 && p.max_pad >= 0), "conv_gemm: per-clip lengths need len_mul >= 1");
    QA_REQUIRE(!p.am_dist || (vec_epi && p.am_idx && p.am_x2 && p.am_e2 && al16(p.am_e2) && p.am_ld >= (p.N + 31) / 32 && !p.y2),
               "conv_gemm: the arg-min epilogue needs N %% 4 == 0, x2 / e2 / dist / idx and am_ld >= ceil(N / 32)");
    QA_REQUIRE(!p.rope || (vec_epi && p.rope_hd % 4 == 0 && p.rope_n % 4 == 0 && p.rope_T > 0 && al16(p.rope)),
               "conv_gemm: fused RoPE needs the float4 epilogue (N, strides, pointers multiples of 4 / 16 B)");
    ConvParams q = p;
    q.xcd_swizzle = (int)knob(K_GEMM_XCD);
    q.panel = (int)knob(K_GEMM_PANEL);
    // QA_GEMM_PRESPLIT: the weight's pre-split image, when a loaded store (or a caller) attached one that covers all N rows; only the
    // split-6 instances read it
    q.wp = knob(K_GEMM_PRESPLIT) != 0 ? weight_planes_find(p.w, (long long)p.N * p.K) : nullptr;
    q.vec_epi = vec_epi;
    // frame / in_rep by multiply-high: exact for frame * in_rep < 2^32 (frames of one clip are < 2^31 / ldx)
    q.rep_one = p.in_rep > 1 ? 0u : 1u;
    q.rep_magic = p.in_rep > 1 ? (unsigned)(((1ULL << 32) + p.in_rep - 1) / p.in_rep) : 0u;

    switch (choose_tile(q)) {
        case PROF_CFG_128x32: return launch_cfg<128, 32, 4, 1>(q, stream);
        case PROF_CFG_128x64: return launch_cfg<128, 64, 2, 2>(q, stream);
        case PROF_CFG_64x128: return launch_cfg<64, 128, 1, 4>(q, stream);
        case PROF_CFG_64x64: return launch_cfg<64, 64, 2, 2>(q, stream);
        case PROF_CFG_256x128: return launch_cfg<256, 128, 2, 2>(q, stream);
        default: return launch_cfg<128, 128, 2, 2>(q, stream);
    }
}

int conv_params_from_args(const qa_conv_args& a, ConvParams* out) {
    ConvParams p{};
    QA_REQUIRE(a.x && a.w && a.y, "conv1d_cl: x, w, y must be non-null");
    QA_REQUIRE(a.B > 0 && a.T_in > 0 && a.C_in > 0 && a.N > 0 && a.T_out >= 0, "conv1d_cl: bad shape");
    QA_REQUIRE(a.ksize >= 1 && a.stride >= 1 && a.pad_left >= 0 && a.pad_right >= 0, "conv1d_cl: bad geometry");
    QA_REQUIRE(a.B * a.T_out < (1LL << 31) && a.ksize * a.C_in < (1LL << 31), "conv1d_cl: shape too large");
    p.x = a.x; p.w = a.w; p.bias = a.bias; p.gamma = a.gamma; p.res = a.residual; p.gate = a.gate; p.y = a.y;
    p.ldx = a.ldx ? a.ldx : a.C_in;
    p.ldy = a.ldy ? a.ldy : a.N;
    p.ldr = a.ldr ? a.ldr : a.N;
    p.ldg = a.ldg ? a.ldg : a.N;
    p.B = (int)a.B; p.T_in = (int)a.T_in; p.C_in = (int)a.C_in; p.T_out = (int)a.T_out; p.N = (int)a.N;
    p.K = (int)(a.ksize * a.C_in);
    p.M = (int)(a.B * a.T_out);
    p.ksize = a.ksize; p.stride = a.stride; p.pad_left = a.pad_left; p.pad_mode = a.pad_mode;
    const int max_pad = a.pad_left > a.pad_right ? a.pad_left : a.pad_right;
    p.Lp = (p.T_in <= max_pad) ? max_pad + 1 : p.T_in;
    // every window must stay inside the padded signal
    p.in_rep = a.in_rep > 1 ? a.in_rep : 1;
    QA_REQUIRE(a.T_out == 0 || (a.T_out - 1) * (int64_t)a.stride + a.ksize <= a.pad_left + a.T_in * (int64_t)p.in_rep + a.pad_right,
               "conv1d_cl: T_out=%lld windows do not fit pad_left=%d + T_in=%lld + pad_right=%d", (long long)a.T_out,
               a.pad_left, (long long)a.T_in, a.pad_right);
    p.prologue = a.prologue; p.act = a.act; p.post_act = a.post_act;
    *out = p;
    return QA_OK;
}

}  // namespace qa

// test hook (not in the public header): qa_conv1d_cl with the two pieces of tap-table geometry that qa_conv_args does not carry - a dilation
// (zero padding, in_rep 1) and per-clip lengths (lens: DEVICE int [B], or null; clip b holds lens[b] * len_mul frames, as ConvParams says)
extern "C" int qa_debug_conv1d_cl_ex(const qa_conv_args* args, int dilation, const int* lens, int len_mul, void* stream) {
    if (!args || dilation < 1) {
        qa::set_error("qa_debug_conv1d_cl_ex: bad argument");
        return QA_ERR_INVALID;
    }
    qa::ConvParams p;
    QA_TRY(qa::conv_params_from_args(*args, &p));
    p.dilation = dilation;
    if (lens) {
        p.lens = lens;
        p.len_mul = len_mul;
        p.max_pad = args->pad_left > args->pad_right ? args->pad_left : args->pad_right;
    }
    return qa::launch_conv_gemm(p, static_cast<hipStream_t>(stream));
}

// test hook (not in the public header): the tile (a QA_GEMM_CFG value) launch_conv_gemm would take for an M x N x K layer of kernel size
// `ksize` - `linear`: a LINEAR-form layer without prologue; `share`: launches of this shape running side by side; the weight is taken to have a pre-split
// image, as every loaded model's has - under the current knobs, without launching anything; negative for a bad argument
extern "C" int qa_debug_conv_gemm_tile(long long M, long long N, long long K, int ksize, int linear, int math_fp32, int share) {
    if (M <= 0 || N <= 0 || K <= 0 || ksize < 1 || K % ksize != 0 || M >= (1LL << 31) || N >= (1LL << 31) || K >= (1LL << 31)) {
        qa::set_error("qa_debug_conv_gemm_tile: bad argument");
        return -1;
    }
    const bool lin = linear != 0 && ksize == 1 && qa::knob(qa::K_GEMM_LINEAR) != 0;
    return qa::choose_tile(qa::TileQuery{M, N, K, (int)(K / ksize), lin, false, qa::knob(qa::K_GEMM_MATH) != 0 && !math_fp32, true, share});
}
