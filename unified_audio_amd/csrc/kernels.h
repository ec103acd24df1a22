// kernels.h - host-side launchers of every HIP kernel in libquarkaudio_hip, grouped by the .hip file that defines them.  Every launcher
// is declared once: here, in lm_decode.h (the fused decode step, next to its argument structs) or in common.h (launch_conv_gemm,
// launch_weight_planes).  A .hip file includes the header that declares its launchers, so the compiler checks each definition against
// the declaration its callers see; a model file declares none of its own.
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

#include "common.h"
#include "lm_session_rows.h"

namespace qa {

// Per-clip lengths of a ragged H-Codec call: clip b of a [B, T, ...] launch holds n[b] * mul frames (at most T);
// n is DEVICE memory [B].  n == nullptr (the default everywhere): every clip has T frames, and the kernel takes today's path through one
// uniform branch, without a load.
struct ClipLens {
    const int* n = nullptr;
    int mul = 0;
    ClipLens times(int k) const { return ClipLens{n, mul * k}; }
};

// ew.hip
// pad_left < 0: the non-causal split of SConv1d (left = pad_total - pad_total / 2); causal SConv1d passes ksize - 1
int launch_conv_in(const float* x, const float* w_kc, const float* bias, float* y, int B, int T, int Cout, int ksize,
                   hipStream_t s, int pad_left = -1, ClipLens rl = ClipLens());
// the same filter as a VALID convolution over a window x [B, T_in] that already holds its left context: no padding, y [B, T_out, Cout]
// with T_out = T_in - ksize + 1 (the streaming encoder's conv0)
int launch_conv_in_window(const float* x, const float* w_kc, const float* bias, float* y, int B, int T_in, int Cout, int ksize, hipStream_t s);
// stream_conv.hip: the window of a causal convolution in a stream and its next state, one launch.  win [B, ctx + n, C] = head | chunk
// [B, n, C], the head being state_in [B, ctx, C] or, on the first step (n > ctx), the reflection of the chunk (position -1 - j reads frame
// 1 + j); state_out [B, ctx, C] = the window's last ctx rows.  state_in and state_out are different buffers (n < ctx: they overlap in time)
// rows.n / first_rows (device int [B], both or neither): item b holds rows.n[b] * rows.mul <= n live chunk rows and
// is a first step iff first_rows[b] != 0; zeros behind its rows in the window, its next state ends at its own last row, `first` is unused
int launch_stream_window(const float* state_in, const float* chunk, float* win, float* state_out, int B, int ctx, int n, int C, int first,
                         hipStream_t s, ClipLens rows = ClipLens(), const int* first_rows = nullptr);
// seanet_front.hip: conv0 + SEANetResnetBlock + the ELU in front of the strided conv, one launch, `a` written once
bool seanet_front_supported(int C, int hid, int L);
int launch_seanet_front(const float* wav, const float* w0, const float* b0, const float* w3, const float* b3, const float* wsc,
                        const float* bsc, const float* wpw, const float* bpw, float* a, int B, int L, int C, int hid, int causal,
                        hipStream_t s);
int launch_rmsnorm(const float* x, const float* w, float* y, long long rows, int C, float eps, hipStream_t s);
int launch_layernorm(const float* x, const float* w, const float* b, float* y, long long rows, int C, float eps,
                     hipStream_t s);
// pad_left < 0: "same" (ksize / 2 each side); the causal Conv1d of vq/conv.py:44-47 passes ksize - 1
int launch_dwconv(const float* x, const float* w_kc, const float* bias, const float* lnw, const float* lnb, float* y,
                  int B, int T, int C, int ksize, float eps, hipStream_t s, int pad_left = -1, ClipLens rl = ClipLens());
size_t groupnorm_scratch_bytes(int B, int T, int G);
int launch_groupnorm(const float* x, const float* w, const float* bias, float* y, double* scratch, int B, int T, int C,
                     int G, float eps, int swish, hipStream_t s, ClipLens rl = ClipLens());
// rot_heads > 0: only heads 0 .. rot_heads - 1 of q and k are rotated (Conformer `pe_attn_head`, conformer.py:157-160)
int launch_rope(float* qkv, const float* cos_sin, int B, int N, int H, int hd, long long ld, int pos0, hipStream_t s,
                int interleaved = 0, int rot_heads = 0);
// H-Codec 1.5 per-clip calls pass lens / cap [B] (device): the clips' code-frame counts.  Null everywhere else:
// every clip has T frames and the kernels take the path they always took through one uniform branch, without a load.
int launch_align(const float* sem, int B, int T, int D, float thr, int max_tokens, int* seg, int* start, int* len,
                 int* nseg, int* gmax, const int* lens, hipStream_t s);
int launch_agg_build(const float* feats, const int* seg, const int* start, const int* len, const int* nseg, const float* qemb,
                     float* out, int B, int T, int G, int D, const int* lens, hipStream_t s);
// valid [B, T + G] bytes: 1 where j < lens[b] + nseg[b] (the aggregators' key-padding mask in a per-clip call)
int launch_agg_key_mask(unsigned char* valid, int B, int T, int G, const int* lens, const int* nseg, hipStream_t s);
int launch_agg_gather(const float* x, const int* start, const int* len, const int* nseg, float* out, int B, int T, int G,
                      int D, hipStream_t s);
int launch_agg_query_rows(const float* x, const float* qkv, const int* start, const int* len, const int* nseg, float* xq, float* qq,
                          int B, int T, int G, int D, hipStream_t s);
int launch_agg_zero_padded(const int* nseg, float* out, int B, int G, int D, hipStream_t s);
// pad_minus1: padded groups (len 0) are written as -1 instead of code - K
int launch_codes_inject(const long long* idx, const int* len, long long* dst, int B, int T, int G, int Q, int K, bool pad_minus1,
                        hipStream_t s);
int launch_adaptive_frames(const long long* codes, int B, int Q, int G, int K, int* totals, int* tmax, hipStream_t s);
int launch_token_lengths(const long long* codes, long long* out, int B, int Q, int G, int K, hipStream_t s);
int launch_deaggregate(const long long* codes, const long long* len_codes, long long* out, int B, int Q, int G, int T, int K,
                       const int* cap, hipStream_t s);
int launch_to_channel_last(const float* x, long long sb, long long sc, long long st, float* y, int B, int C, int T,
                           hipStream_t s);
// lens [B] (device) or null: entries n >= lens[b] are written as -1 (the dropped code) whatever the source holds
int launch_codes_to_bqn(const long long* src, long long* dst, int B, int N, int Q, hipStream_t s, const int* lens = nullptr);
int launch_codes_from_bqn(const long long* src, long long* dst, int B, int N, int Q, hipStream_t s, const int* lens = nullptr);
// dst[0 .. count) (device) = the host integers src[0 .. count), in stream order like any kernel.  The values ride in the kernel arguments
// (ROW_INTS_CHUNK per launch): no staging buffer, and the host vector may be freed on return
constexpr int ROW_INTS_CHUNK = 256;
int launch_row_ints(int* dst, const int* src, long long count, hipStream_t s);
// valid [B, N] bytes: 1 where n < rl.n[b] * rl.mul (the key-padding mask of launch_attention)
int launch_len_mask(unsigned char* valid, int B, int N, ClipLens rl, hipStream_t s);
int launch_stft_post(const float* ri, float* out, long long rows, int nb, int ldi, int ldo, hipStream_t s);
int launch_istft_spec(const float* y, float* S, long long rows, int nb, int ldy, int ldS, hipStream_t s);
int launch_istft_ola(const float* frames, const float* win, float* out, int B, int T, int n_fft, int hop, hipStream_t s,
                     ClipLens rl = ClipLens());

int launch_codes_check(const long long* codes, long long n, long long limit, unsigned long long* bad, hipStream_t s);
int launch_codes_count(const long long* codes, long long n, long long lo, long long limit, unsigned long long* bad, hipStream_t s);
int launch_resample(const float* wav, const float* taps, float* out, int B, long long T, long long T_out, int orig, int nw, int width,
                    int ktaps, hipStream_t s, const int* lens = nullptr);  // lens [B] (device): the rows' sample counts, or null

// attention.hip : softmax(Q K^T * scale) V over a fused [B*N, 3*H*hd] QKV buffer (RoPE already applied)
//   causal = 0: full attention over the N keys of the same batch item (codec transformers)
//   causal = 1: key j visible to query i iff j <= i + (n_keys - n_q) (LM prefill / decode over a KV cache)
//   gate [B, H, n_q] + relbias [H, 2R+1] (optional): score(i, j) += gate[b,h,i] * relbias[h][clamp(j - i, -R, R) + R]
//   (WavLM gated relative position bias)
//   kvalid [B, n_keys] bytes (optional, non-causal only; n_q need not equal n_keys: the mask is indexed by key alone): key j of item b
//   is visible iff kvalid[b, j] != 0
//   one kernel body in two arithmetic forms (attention_kernel<HD, BIAS, KMASK, SPLIT>): split-6 on the bf16 MFMA where QA_ATT_MATH = 1
//   math_fp32: keep the fp32 form (SPLIT = false, v_mfma_f32_32x32x2_f32) whatever QA_ATT_MATH says (Ctx::att_fp32)
struct AttnArgs {
    const float *q = nullptr, *k = nullptr, *v = nullptr;  // q [B, n_q, H hd]; k, v [B, n_keys, H hd], item stride kv_batch_stride
    float* out = nullptr;                                  // [B, n_q, H hd]
    long long ldq = 0, ldkv = 0, ldo = 0, kv_batch_stride = 0;  // row strides of q, of k and v, of out
    int B = 0, n_q = 0, n_keys = 0, H = 0, hd = 0;
    float scale = 0.f;
    int causal = 0;
    const float *gate = nullptr, *relbias = nullptr;
    int R = 0;
    int context = 0, q_pos0 = 0, ring_end = 0;  // causal window; ring mode (RingKVCache): position of query 0, end of the ring
    const unsigned char* kvalid = nullptr;
    bool math_fp32 = false;
    // ragged causal chunk (fp32 form, no bias / mask / window): item b holds row_pos0[b] cached keys and row_nq[b] of
    // the n_q query rows (device int [B] each, both or neither).  Query i < row_nq[b] sees key j iff j <= i + row_pos0[b], the key walk
    // stops at row_pos0[b] + row_nq[b], query rows behind row_nq[b] are written as 0.  n_q stays the row count of the q / out layout
    const int *row_pos0 = nullptr, *row_nq = nullptr;
};
int launch_attention(const AttnArgs& a, hipStream_t s);
// self-attention over a packed projection qkv [B N, 3 d] (q | k | v, d = H hd) -> att [B N, d], scale 1 / sqrt(hd), non-causal; the
// caller sets what differs (causal, context, kvalid, gate / relbias / R)
inline AttnArgs attn_packed_qkv(const float* qkv, float* att, int B, int N, int H, int hd) {
    const long long d = (long long)H * hd;
    AttnArgs a;
    a.q = qkv; a.ldq = 3 * d; a.out = att; a.ldo = d;
    a.k = qkv + d; a.v = qkv + 2 * d; a.ldkv = 3 * d; a.kv_batch_stride = (long long)N * 3 * d;
    a.B = B; a.n_q = N; a.n_keys = N; a.H = H; a.hd = hd;
    a.scale = 1.0f / std::sqrt((float)hd);
    return a;
}
// RingKVCache.complete() write (mimi/transformer.py:243-250): rows t = 0..T-1 of k / v (row stride ld, batch stride T * ld) go to
// slot (pos0 + t) % cap of the caches [B, cap, d]
int launch_ring_append(const float* k, const float* v, long long ld, float* kc, float* vc, int B, int T, int d, int cap, int pos0,
                       hipStream_t s);

// stream_attn.hip : what a chunk of a linear (non-ring) K/V cache needs beside launch_attention
// Rotate-half RoPE of q (in place) and k of a packed projection qkv [B n, 3 d] at positions pos0 + t (table cs [.][hd / 2][2]); the
// roped k and v rows go to rows pos0 .. pos0 + n - 1 of the caches kc / vc [B, cap, d].  pos0 + n <= cap is the caller's check
// row_pos0 / row_nq (device int [B], both or neither): item b's rows sit at row_pos0[b] + t and only its first
// row_nq[b] are rotated and appended; the others write nothing.  row_pos0[b] + row_nq[b] <= cap is the caller's check
// ring_inv_freq (device [hd / 2], transformer_rope_table's inv_freq): the caches are RINGS of cap rows - position p
// goes to row p mod cap, and positions at or beyond TR_ROPE_POSITIONS take their angle from inv_freq instead of the table.  Positions
// below 2^24 and n <= cap are the caller's check
constexpr int TR_ROPE_POSITIONS = 8192;  // positions of the codec Transformer's static RoPE table
void transformer_rope_table(int hd, std::vector<float>* cs, std::vector<float>* inv_freq);
int launch_rope_append(float* qkv, const float* cs, float* kc, float* vc, int B, int n, int H, int hd, int pos0, int cap, hipStream_t s,
                       const int* row_pos0 = nullptr, const int* row_nq = nullptr, const float* ring_inv_freq = nullptr);
// Causal attention of a short chunk (n <= ATTN_SHORT_MAX_Q queries at positions pos0 + i) over such a cache, keys 0 .. pos0 + n - 1 under
// the window `context` (0 = none), fp32 arithmetic.  A (row, head) is split over workgroups that own the FIXED key ranges
// [s L, (s + 1) L), L = attn_short_split_keys(cap): a key lands in the same split, tile and lane whatever pos0 is.  Partial records
// [n, hd | m | l] per split in `part` (attn_short_part_floats), merged in split order by a second launch.  q [B n, ldq], out [B n, d]
// row_pos0 / row_nq as in launch_rope_append, max_keys = max_b(row_pos0[b] + row_nq[b]) from the host: the split count of the grid.  Item
// b attends over its own row_pos0[b] + row_nq[b] keys; its queries behind row_nq[b] are written as 0; pos0 is then unused
constexpr int ATTN_SHORT_MAX_Q = 16;
int attn_short_split_keys(int cap);
size_t attn_short_part_floats(int B, int H, int hd, int n, int cap);
int launch_attention_short(const float* q, long long ldq, const float* kc, const float* vc, float* out, float* part, int B, int n, int H,
                           int hd, int pos0, int cap, int context, hipStream_t s, const int* row_pos0 = nullptr, const int* row_nq = nullptr,
                           int max_keys = 0, bool ring = false);
// ring (ring_geometry.h): the caches are rings of cap rows under the window `context` >= 1, cap >= context - 1 + n;
// item b sits at positions pos0 (row_pos0[b]) .. + n (row_nq[b]) - 1, anywhere below 2^24, and its keys are the rows whose position p(s)
// it can see.  The grid covers every split of the ring; max_keys is unused.  A row never written for the item may hold NaN

// lstm.hip : one nn.LSTM layer (batch_first, zero initial state) given the precomputed input projection
//   xw [B, T, 4d] = x W_ih^T + b_ih + b_hh with the 4d axis permuted to (unit, gate) order,
//   w_hh [4d, d] rows permuted the same way.  h_out [B, T, d].  c_state [B, d] scratch.
// eager = true: the T step kernels are launched one by one on `s` (no hipGraph replay, no persistent kernel) - for CU-masked streams,
// whose mask a replayed graph is not known to inherit
int launch_lstm(const float* xw, const float* w_hh_ug, float* h_out, float* c_state, int B, int T, int d,
                hipStream_t s, bool eager = false);
// One chunk of a recurrence that continues (the streaming Transformer): step 0 starts from h_state / c_state [B, d], which hold the
// state behind step T - 1 on return.  Per-step kernels only, launched eagerly on `s`; h_out [B, T, d] as in launch_lstm
// nq / zero (device int [B], both or neither): row b runs its first nq[b] <= T steps - from zero where zero[b] != 0 -
// and carries the state behind step nq[b] - 1; nq[b] = 0 leaves the row's (h, c) untouched
int launch_lstm_carry(const float* xw, const float* w_hh_ug, float* h_out, float* h_state, float* c_state, int B, int T, int d,
                      hipStream_t s, const int* nq = nullptr, const int* zero = nullptr);
// persistent-recurrence bookkeeping for the model graphs: launches so far on `dev`; wait for `s` and report (and clear) a barrier
// time-out; make this thread's next launch_lstm calls take the per-step kernels
int lstm_call_begin(int dev, void** ticket);                  // open a model-graph call: own error word + launch count (thread-local)
int lstm_call_end(void* ticket, hipStream_t s, bool* failed);  // syncs `s` only if a recurrence of the call is still in flight
void lstm_call_note_sync();                                    // the graph synchronised the call's stream itself: collect now
void lstm_force_per_step(bool on);

// rvq.hip
// scratch: rvq_scratch_floats(n_vec, K, D) floats of device workspace (residuals, distance products, norms of one chunk)
size_t rvq_scratch_floats(long long n_vec, int K, int D);
int launch_rvq_search(const float* x, long long n_vec, const float* codebooks, const float* e2, int Q, int K, int D,
                      long long* indices, float* quantized, long long ldq, float* scratch, hipStream_t s);
int launch_rvq_norms(const float* codebooks, float* e2, int QK, int D, hipStream_t s);
int launch_rvq_lookup(const long long* indices, long long n_vec, const float* codebooks, int Q, int K, int D, float* out,
                      long long ldo, hipStream_t s);

// lm_kernels.hip
int launch_assemble_prompt(float* x, const float* task_vec, const float* enroll_sos, const float* enroll_emb,
                           const float* mix_sos, const float* mix_emb, int B, int Ne, int Nm, int d, hipStream_t s,
                           const int* off = nullptr);  // off [B] (device): row b holds Ne + off[b] enrollment frames, zeros behind its prompt
int launch_skinny_gemm(const float* x, long long ldx, const float* w, const float* bias, const float* gate, long long ldg,
                       const float* res, long long ldr, float* y, long long ldy, int M, int N, int K, int act, hipStream_t s,
                       float rms_eps, int dual);
// row_pos0 / row_n (device int [B], both or neither): item b's t-th row sits at position row_pos0[b] + t and only its first row_n[b]
// rows are rotated and appended (a ragged chunk); nullptr: every item at pos0 with all n rows
int launch_rope_kv(float* qkv, const float* cs, float* kc, float* vc, int B, int n, int H, int hd, int pos0, int max_len,
                   hipStream_t s, const int* row_pos0 = nullptr, const int* row_n = nullptr);
// y [B, n, d] <- x [B, n, d] for the rows t < row_n[b], exact zeros for the others, whose x rows are never read
int launch_lm_rows_masked_copy(float* y, const float* x, int B, int n, int d, const int* row_n, hipStream_t s);
// exact zeros into the rows t >= row_n[b] of every one of the `entries` tensors [B, n, d] that lie entry_stride floats apart
int launch_lm_rows_zero_pad(float* y, long long entry_stride, int entries, int B, int n, int d, const int* row_n, hipStream_t s);
int launch_lm_targets(float* x, long long ldx_seq, const float* table, const long long* gids, int G, const long long* sids, int T, int V,
                      int goff, int soff, long long* tgt, int B, int d, hipStream_t s, int drop = 0);
int launch_lm_row_loss(const float* z, long long ldl, int V, long long rows, const long long* tgt, float c, float sm, float* row_kl,
                       int* row_ok, hipStream_t s);
int launch_lm_seq_reduce(const float* row_kl, const int* row_ok, int B, int Lt, double* seq_sum, float* loss_seq, long long* correct_seq,
                         hipStream_t s);
int launch_lm_batch_reduce(const double* seq_sum, const long long* correct_seq, int B, int Lt, float* loss, float* acc, hipStream_t s);
// scoring with per-row lengths.  ne_r / nm_r / T_r / lp_r / off_r: device int [B] of one group (launch_row_ints):
// the row's enrollment frames, mixture frames, semantic ids, prompt positions and packed target-row offset
// x [B, n, d] <- prompt + input embeddings left-aligned, zeros behind; tgt (packed) <- the targets.  table == nullptr: the prompt alone
// task_vec == nullptr: CustomLlamaModel's prompt [mix_sos, mix_emb[b, :nm]] (mix_emb [B, Nm, d]: the condition embeddings) or none (mix_emb
// null).  drop = 1 in the three launchers: a row's own last position is left out, Lt_b = G + T[b] + 1
// Filled by name, like AttnArgs; every member defaults to "absent", so a prompt-only pass sets the prompt's members alone
struct ScoreAssembleArgs {
    float* x = nullptr;  // [B, n, d]
    int n = 0, B = 0, d = 0;
    const float *task_vec = nullptr, *enroll_sos = nullptr, *enroll_emb = nullptr, *mix_sos = nullptr, *mix_emb = nullptr;
    int Ne = 0, Nm = 0;  // the frame strides of enroll_emb / mix_emb
    const float* table = nullptr;  // codec_embedding [V, d]; with it gids [B, G] / sids [B, T_max] (offsets goff / soff) and tgt
    const long long *gids = nullptr, *sids = nullptr;
    int G = 0, T_max = 0, V = 0, goff = 0, soff = 0;
    long long* tgt = nullptr;
    const int *ne_r = nullptr, *nm_r = nullptr, *T_r = nullptr, *off_r = nullptr;
    int drop = 0;
};
int launch_lm_score_assemble(const ScoreAssembleArgs& a, hipStream_t s);
// y (packed [sum Lt_b, d]) <- x[b, lp[b] .. lp[b] + Lt_b - 1, :], Lt_b = G + T[b] + 2 - drop <= Lt_max
int launch_lm_score_gather(float* y, const float* x, int B, int n, int d, int G, int Lt_max, const int* lp_r, const int* T_r, const int* off_r,
                           hipStream_t s, int drop = 0);
int launch_lm_seq_reduce_rows(const float* row_kl, const int* row_ok, int B, int G, const int* T_r, const int* off_r, double* seq_sum,
                              float* loss_seq, long long* correct_seq, hipStream_t s, int drop = 0);
int launch_lm_batch_reduce_rows(const double* seq_sum, const long long* correct_seq, int B, long long total, float* loss, float* acc,
                                hipStream_t s);
// one wave of independent row moves of a KV cache (qa_lm_cache_select; KvMoves: lm_session_rows.h), passed by value
int launch_kv_row_moves(float* kc, float* vc, float* spare, int n_layers, int max_batch, int max_len, int d, const KvMoves& mv, hipStream_t s);

// ssl_kernels.hip
// wav_len / l0_len [B] (device, both or neither): clip b holds wav_len[b] of the T samples and l0_len[b] of the T1 layer-0 frames
size_t ssl_conv0_scratch_bytes(int B, int T1, int C0);
int launch_ssl_conv0(const float* wav, const float* w_kc, const float* bias, const float* gamma, const float* beta, float* y,
                     void* scratch, int B, int T, int T1, int C0, int ksize, int stride, int pad, int norm_group, float eps, int act,
                     hipStream_t s, const int* wav_len = nullptr, const int* l0_len = nullptr);
int launch_ssl_gate(const float* hidden, const float* wab, const float* bab, const float* cst, float* gate, int B, int N, int H, int hd,
                    hipStream_t s);
int launch_ssl_accumulate(float* dst, const float* src, long long n, int first, hipStream_t s);
int launch_ssl_act(float* x, long long n, int act, hipStream_t s);
// n_len [B] (device) or null: out is [B, N, d] and the rows n >= n_len[b] of clip b are written as 0
int launch_ssl_compress(const float* sum, float* out, long long n, float scale, float expo, hipStream_t s, const int* n_len = nullptr,
                        int N = 0, int d = 0);

// bicodec_kernels.hip
// The per-clip calls of BiCodec pass the clips' lengths; null everywhere else: today's path through one
// launch-uniform branch, without a load.
// lens [n / T] (device): rows t >= lens[b] of clip b are written as zeros and their tokens are never read
int launch_gather_rows(const long long* tok, const float* table, float* out, long long n, int V, int D, hipStream_t s, int T = 0,
                       const int* lens = nullptr);
// tok [B, N]: -1 at n >= lens[b];  x [B, T]: 0.0f at t >= rl.n[b] * rl.mul.  Per-clip calls only (lens not null)
int launch_tokens_fill_behind(long long* tok, int B, int N, const int* lens, hipStream_t s);
int launch_zero_behind(float* x, int B, long long T, ClipLens rl, hipStream_t s);
int launch_gather_global(const long long* tok, const float* table, float* out, int B, int N, int V, int L, hipStream_t s);
int launch_adaln(const float* x, const float* scale, const float* shift, long long ld_cond, float* y, int B, int T, int C, float eps,
                 hipStream_t s);
int launch_add_rowvec(float* x, const float* v, int B, int T, int C, hipStream_t s);
// lens_host [B] (HOST memory, 1 .. T each, travels by value in the launch) or null: row b is normalised over its own samples, zeros behind
int launch_wav_normalize(const float* x, float* y, int B, long long T, float eps, hipStream_t s, const long long* lens_host = nullptr);
int launch_l2norm_rows(const float* x, float* y, long long rows, int D, hipStream_t s);
// lens [B] (device, samples) or null: the reference clip of row b tiles by lens[b] instead of T
int launch_mel_frames(const float* wav, int B, long long T, long long ref_len, int hop, int n_frames, float* P, hipStream_t s,
                      const int* lens = nullptr);
int launch_spec_mag(const float* ri, int nbp, int nb, float* mag, int ldm, long long rows, hipStream_t s);
int launch_res2_chain(const float* x, float* y, const float* wt, const float* bst, int B, int T, int C, int d, hipStream_t s);
int launch_se_residual(const float* x, long long ldx, const float* y, const float* w1, const float* b1, const float* w2, const float* b2,
                       float* gate, float* out, long long ldo, int B, int T, int C, int Hd, hipStream_t s);
int launch_perceiver_ctx(const float* lat, long long lat_b, const float* x, float* ctx, int B, int n_lat, int T, int D, hipStream_t s);
int launch_geglu(const float* h, int F, float* out, int ldo, long long rows, hipStream_t s);
int launch_l2norm_scale(const float* x, const float* gamma, float* y, long long rows, int D, float scale, hipStream_t s);
int launch_fsq(const float* x, const float* w, const float* bias, const int* levels, int nl, int D, long long rows, int* tokens,
               float* bounded, hipStream_t s);
int launch_astp_pool(const float* logit, const float* x, int B, int T, int C, const float* bn_s, const float* bn_t, float* pool, float* bn,
                     hipStream_t s);
int launch_frame_stats(const float* x, int B, int T, int C, float* ctx, hipStream_t s);
int launch_code_usage(const long long* idx, long long n, int K, float* perplexity, float* active, hipStream_t s);
int launch_widen_i32(const int* src, long long* dst, long long n, hipStream_t s);

// conformer_kernels.hip
// the nullable last arguments are device int [B] of a call with per-row lengths: the items' frame counts (rows, frames
// of the [., F, C] tensor), sample counts, or prompt offsets n_cond[b] - T; null: today's launch
int launch_glu_dwconv_bn_silu(const float* u, const float* w31, const float* bias, const float* scale, const float* shift, float* y, int B,
                              int T, int C, hipStream_t s, const int* rows = nullptr);
int launch_masked_add(float* x, float* y, const unsigned char* valid, long long rows, int C, hipStream_t s);
int launch_mask_count(const unsigned char* valid, int B, int T, int* counts, hipStream_t s);
int launch_logmel_frames(const float* wav, int B, long long n, int pad, long long n_out, float* P, hipStream_t s, const int* rows = nullptr);
int launch_log_eps(float* x, long long n, float eps, hipStream_t s, const int* frames = nullptr, int F = 0, int C = 0);
int launch_cond_prompt(float* x, const float* sos, const float* cond, int B, int T, int d, hipStream_t s, const int* off = nullptr);

}  // namespace qa
