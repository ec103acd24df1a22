// lm.cpp - UniSE decoder-only AR-LM: prompt assembly, prefill and the greedy global + semantic decode loop.
//
// Mirrors LLM_SFT.generate (QuarkAudio-UniSE/model/llm/llm_sft.py:93-195) over the Llama body the reference lifts out of
// HF transformers (model/llm/llm.py:63-79,150-227): RMSNorm -> QKV (no bias) -> rotate-half RoPE -> causal attention over
// the KV cache -> O -> +res -> RMSNorm -> SwiGLU -> +res, final RMSNorm, output_head, vocabulary-range mask, greedy arg-max
// (llm.py:253-288 with do_sample=False, the reference's test path: model/model.py:173).
//
// The whole loop is device-resident: token ids never visit the host between steps (embedding gather and arg-max read / write a
// device int64 vector), the KV cache is owned by the handle's workspace, prefill runs on the implicit-GEMM / flash kernels
// and each decode step on the weight-streaming skinny GEMM + single-query attention kernels.
//
// qa_lm_score is the other entry point, LLM_SFT.forward (llm_sft.py:37-90): the whole teacher-forced sequence through the same body
// (every layer), output_head over the full vocabulary on the target rows, and the label-smoothed KL + accuracy (llm.py:87-104).
// qa_lm_score_ragged / qa_lm_prompt_ragged are the same with per-row lengths (host logic in lm_score_rows.h).
#include <memory>

#include <climits>
#include <cstdio>
#include <cstdlib>

#include "host_util.h"
#include "lm_decode.h"
#include "lm_score_rows.h"
#include "row_lengths.h"

using namespace qa;

namespace {
struct LMLayer {
    // RMSNorm weights are folded into the consuming projections (W' = W diag(w)): qkv <- input_layernorm, gate/up <- post_attention_layernorm
    ConvW qkv, o, gate, up, down;
    // fused decode step (lm_decode.hip): tile-major rows; qkv_dec pairs rotary partners (i, i + hd/2) inside a tile,
    // gu_dec holds per tile NT/2 gate rows then NT/2 up rows (both norm-folded)
    const float* qkv_dec = nullptr;
    const float* gu_dec = nullptr;
    const float* down_dec = nullptr;  // fused MLP: W_down slice-major [I / 16][d][16] (slice j = columns 16 j .. 16 j + 15 of every row)
};
constexpr int LM_MAX_POS = 4096;  // max_position_embeddings (conf/config.yaml:146)
constexpr int LM_MAX_CHAINS = 16;

// the buffers of the fused n = 1 step (lm_decode.hip) and the key split of its attention launch, placed by alloc_step
struct StepBufs {
    float *x = nullptr, *q = nullptr, *u = nullptr, *att_part = nullptr, *mlp_part = nullptr;
    int* state = nullptr;
    int att_tps = 0, S_att = 0;  // 16-key tiles per split, and the split count of a replayed step
};
}  // namespace

struct StepGraph {  // one captured decode step of a phase, replayable because every loop-carried scalar lives in device state
    hipGraphExec_t exec = nullptr;
    hipGraph_t graph = nullptr;
    uint64_t key = 0;
    void reset() {
        if (exec) (void)hipGraphExecDestroy(exec);
        if (graph) (void)hipGraphDestroy(graph);
        exec = nullptr;
        graph = nullptr;
        key = 0;
    }
};

// A KV cache a caller holds across qa_lm_forward calls.  One device allocation of its own: K and V as
// [layer][max_batch][max_len][hidden] fp32 (the row layout lm_body and the fused step use, with the layer stride fixed by max_batch so
// that a batch select never moves a layer), one spare row per (layer, K / V) for the select's cycles, and the buffers of the n = 1 step.
// Lengths and batch are HOST state.  Every row has a length of its own; a call that needs them on the device
// writes them, in stream order, into `rows`.
struct qa_lm_cache {
    qa_lm* lm = nullptr;
    int max_batch = 0, max_len = 0;
    int B = 0;             // 0: not fixed yet (fresh or reset)
    std::vector<int> len;  // [max_batch] positions row b holds (rows behind B: 0)
    char* mem = nullptr;
    float *kc = nullptr, *vc = nullptr, *spare = nullptr;
    // device ints [2][max_batch] of a ragged call: a chunk's (position of the first new row, new rows), a step's (offset to the step's
    // position as GemvArgs::off, 1 or 0 new rows)
    int* rows = nullptr;
    StepBufs step;  // n = 1 step, min(max_batch, 64) rows
    int longest() const { return B > 0 ? *std::max_element(len.begin(), len.begin() + B) : 0; }
    bool uniform() const { return B == 0 || std::all_of(len.begin(), len.begin() + B, [&](int v) { return v == len[0]; }); }
};
void cache_free(qa_lm_cache* c);

struct qa_lm : Handle {
    qa_lm_spec spec{};
    bool fused_ok = false;   // the shapes fit the fused decode step (required since r05: build_lm refuses a spec that does not tile)
    bool mlp_fused = false;  // QA_LM_MLP_FUSED at create time: gate/up + SwiGLU + down as one launch + a reduce launch
    int mlp_ac = 16;         // activation columns per workgroup of that launch (8 measured equal at B = 16, -4 % at B = 64: profiles/r03_lm_ab.txt)
    int att_split = 256;     // keys per workgroup of the decode attention, at most 4 splits (flat between 256 and 384, worse below: same log; re-measured in r05 with the cheaper o_proj: 128 / 160 / 192 keys 112.2 - 112.5 ms against 110.4 at 16 segments)
    int nt_qkv = 0, nt_o = 0, nt_gu = 0, nt_down = 0;
    hipStream_t cap_stream = nullptr;
    std::vector<StepGraph> graphs;  // [2 * chain + phase]: phase 0 global, 1 semantic
    std::vector<hipStream_t> chain_streams;  // internal streams of the chains of a B > 64 call
    std::vector<hipEvent_t> chain_join;
    hipEvent_t ev_fork = nullptr;
    unsigned long long calls = 0;
    const float *task_emb = nullptr, *enroll_sos = nullptr, *mix_sos = nullptr, *codec_emb = nullptr, *ones = nullptr,
                *rope = nullptr;  // `ones`: unit RMSNorm weight (the learned ones are folded into the projections)
    ConvW adapter, head;
    // the session entry points (qa_lm_forward / qa_lm_head) return and consume the final norm's OUTPUT, so they need the norm weight and the
    // un-folded output_head that generate's fused head never reads
    const float* norm_w = nullptr;
    ConvW head_raw;
    std::vector<LMLayer> layers;
    // test hook (qa_lm_enable_taps): the slice logits of every decode step, in an allocation of their own (never the workspace, so
    // turning taps on cannot move a buffer of the step); tap_n: elements of logits.global / logits.semantic of the last call (-1: none)
    bool taps = false;
    Workspace tap_buf;
    int64_t tap_n[2] = {-1, -1};
    // Three workspaces, one per family of entry points, because a call that grows its workspace frees the old buffer:
    //   ws (Handle)  qa_lm_generate*: the captured decode steps point into it (they are keyed by its address)
    //   score_ws     qa_lm_score*: scoring never moves a buffer a captured step points into
    //   sess_ws      qa_lm_forward (n >= 2 chunks, cache-less calls) and qa_lm_prompt: a session never moves a buffer of generate or score
    //                (the KV caches themselves are allocations of their own, qa_lm_cache)
    // generate plans on Handle::ctx and the sessions on sess_ctx, which run_session and its callers' graph lambdas must both name.  Score
    // plans on a Ctx on its stack: a Ctx carries nothing from one call to the next (plan re-arms it) and nothing else has to reach it.
    Workspace score_ws;
    Workspace score_tap;  // logits.forced [B][Lt][V] of the last score call (taps on), an allocation of its own like tap_buf
    int64_t score_tap_n = -1;
    Workspace sess_ws;
    Ctx sess_ctx;
    std::vector<qa_lm_cache*> caches;  // live caches of this handle (qa_lm_destroy frees the ones the caller left)
    ~qa_lm() {
        while (!caches.empty()) cache_free(caches.back());  // unregisters itself
        for (StepGraph& g : graphs) g.reset();  // before the buffers they point into
        if (cap_stream) (void)hipStreamDestroy(cap_stream);
        for (hipStream_t st : chain_streams) (void)hipStreamDestroy(st);
        for (hipEvent_t ev : chain_join) (void)hipEventDestroy(ev);
        if (ev_fork) (void)hipEventDestroy(ev_fork);
    }
};

namespace {

int vocab_of(const qa_lm_spec& s) { return 3 + s.global_size + s.semantic_size; }

// tile width of the head GEMV over a vocabulary slice of `width` entries (0: the slice does not tile)
int head_nt(int width) {
    int nt = lm_pick_nt(width);
    while (nt >= 4 && width % nt) nt >>= 1;
    return nt >= 4 ? nt : 0;
}

int build_lm(qa_lm* lm, const HostTable& tab) {
    const qa_lm_spec& sp = lm->spec;
    const int d = sp.hidden, V = vocab_of(sp), I = sp.intermediate;
    QA_REQUIRE(sp.n_heads > 0 && d % sp.n_heads == 0, "lm spec: hidden %d not divisible by %d heads", d, sp.n_heads);
    const int hd = d / sp.n_heads;
    QA_REQUIRE(hd == 32 || hd == 64 || hd == 128, "lm spec: head_dim %d unsupported", hd);
    QA_REQUIRE(d % 32 == 0 && I % 32 == 0 && sp.feats_dim % 32 == 0, "lm spec: widths must be multiples of 32");
    // fused decode step: K of every GEMV a multiple of 256, every N a multiple of its tile width, rotary pairs inside a tile
    lm->nt_qkv = lm_pick_nt(3 * d);
    lm->nt_o = lm_pick_nt(d);
    lm->nt_gu = lm_pick_nt(2 * I);
    lm->nt_down = lm_pick_nt(d);
    lm->mlp_fused = knob(K_LM_MLP_FUSED) != 0 && lm_mlp_fused_supported(d, I, lm->nt_gu);
    lm->fused_ok = lm_gemv_supported(d, I) && d % lm->nt_qkv == 0 && hd % lm->nt_qkv == 0 && d % lm->nt_o == 0 &&
                   (2 * I) % lm->nt_gu == 0 && hd % 8 == 0 && head_nt(sp.global_size) && head_nt(sp.semantic_size);
    // r05: the per-op decode step of round 1 (skinny GEMM + attention_decode kernels behind QA_LM_UNFUSED, the path a spec took when the
    // fused step did not tile it) is gone - a spec the fused step cannot tile is refused here, with the reason
    QA_REQUIRE(lm->fused_ok, "lm spec: the decode step needs hidden %% 256 == 0 (got %d), intermediate %% 256 == 0 (got %d), head_dim %% 8 == 0 and "
               "global / semantic vocabulary sizes that are multiples of 4 (got %d / %d)", d, I, sp.global_size, sp.semantic_size);
    lm->store.planes = false;  // every conv_gemm launch of the LM keeps the fp32 chain (Ctx::gemm_fp32): no pre-split image
    Loader L(tab, lm->store);
    L.vec(&lm->task_emb, "task_embedding.weight", (int64_t)sp.num_tasks * d);
    L.vec(&lm->enroll_sos, "enroll_sos_embedding.weight", d);
    L.vec(&lm->mix_sos, "mix_sos_embedding.weight", d);
    L.vec(&lm->codec_emb, "codec_embedding.weight", (int64_t)V * d);
    L.raw(&lm->ones, std::vector<float>(d, 1.0f));
    // fold W' = W diag(w_norm): rows of W scaled column-wise by the RMSNorm weight that precedes the projection
    auto folded = [&](const std::string& wname, int64_t rows, const float* nw, std::vector<float>* out) -> bool {
        const float* w = L.need(wname, rows * d);
        if (!w || !nw) return false;
        out->resize((size_t)rows * d);
        for (int64_t r = 0; r < rows; ++r)
            for (int k = 0; k < d; ++k) (*out)[(size_t)r * d + k] = w[r * d + k] * nw[k];
        return true;
    };
    L.conv(&lm->adapter, "adapter", d, sp.feats_dim, 1);
    lm->head.N = V; lm->head.C_in = d;
    {
        std::vector<float> hw;
        if (folded("output_head.weight", V, L.need("norm.weight", d), &hw)) L.raw(&lm->head.w, hw);
    }
    lm->layers.resize(sp.n_layers);
    for (int i = 0; i < sp.n_layers; ++i) {
        LMLayer& Lw = lm->layers[i];
        const std::string p = "layers." + std::to_string(i);
        const float* ln1 = L.need(p + ".input_layernorm.weight", d);
        const float* ln2 = L.need(p + ".post_attention_layernorm.weight", d);
        std::vector<float> wq((size_t)3 * d * d, 0.f);
        const char* nm[3] = {".self_attn.q_proj.weight", ".self_attn.k_proj.weight", ".self_attn.v_proj.weight"};
        for (int j = 0; j < 3; ++j) {
            std::vector<float> f;
            if (folded(p + nm[j], d, ln1, &f)) std::memcpy(&wq[(size_t)j * d * d], f.data(), sizeof(float) * d * d);
        }
        Lw.qkv.N = 3 * d; Lw.qkv.C_in = d;
        L.raw(&Lw.qkv.w, wq);
        if (lm->fused_ok) {  // tile t of a section: rows [t*NT/2, (t+1)*NT/2) of each head-half, first halves then partner halves
            const int nt = lm->nt_qkv, hp = nt / 2;
            std::vector<float> wd((size_t)3 * d * d);
            size_t r = 0;
            for (int sec = 0; sec < 3; ++sec)
                for (int h = 0; h < sp.n_heads; ++h)
                    for (int t = 0; t < hd / nt; ++t)
                        for (int half = 0; half < 2; ++half)
                            for (int j = 0; j < hp; ++j, ++r) {
                                const size_t src = (size_t)sec * d + (size_t)h * hd + (size_t)half * (hd / 2) + (size_t)t * hp + j;
                                std::memcpy(&wd[r * d], &wq[src * d], sizeof(float) * d);
                            }
            L.raw(&Lw.qkv_dec, wd);
        }
        L.conv(&Lw.o, p + ".self_attn.o_proj", d, d, 1, false);
        Lw.gate.N = I; Lw.gate.C_in = d;
        Lw.up.N = I; Lw.up.C_in = d;
        {
            std::vector<float> g, u;
            if (folded(p + ".mlp.gate_proj.weight", I, ln2, &g) && folded(p + ".mlp.up_proj.weight", I, ln2, &u)) {
                L.raw(&Lw.gate.w, g);
                L.raw(&Lw.up.w, u);
                if (lm->fused_ok) {
                    const int hp = lm->nt_gu / 2;
                    std::vector<float> gd((size_t)2 * I * d);
                    for (int t = 0; t < I / hp; ++t) {
                        std::memcpy(&gd[(size_t)(t * 2 * hp) * d], &g[(size_t)(t * hp) * d], sizeof(float) * hp * d);
                        std::memcpy(&gd[(size_t)(t * 2 * hp + hp) * d], &u[(size_t)(t * hp) * d], sizeof(float) * hp * d);
                    }
                    L.raw(&Lw.gu_dec, gd);
                }
            }
        }
        L.conv(&Lw.down, p + ".mlp.down_proj", d, I, 1, false);
        if (lm->fused_ok && lm->mlp_fused) {
            const float* wdn = L.need(p + ".mlp.down_proj.weight", (int64_t)I * d);
            if (wdn) {
                std::vector<float> ws((size_t)I * d);
                const int ac = lm->mlp_ac;
                for (int j = 0; j < I / ac; ++j)
                    for (int n = 0; n < d; ++n) std::memcpy(&ws[((size_t)j * d + n) * ac], &wdn[(size_t)n * I + (size_t)j * ac], sizeof(float) * ac);
                L.raw(&Lw.down_dec, ws);
            }
        }
    }
    // LlamaRotaryEmbedding (default rope): inv_freq = theta^(-2i/hd), cos / sin of pos * inv_freq in fp32
    const int half = hd / 2;
    std::vector<float> cs((size_t)LM_MAX_POS * half * 2);
    for (int i = 0; i < half; ++i) {
        const float inv = 1.0f / std::pow(sp.rope_theta, (float)(2 * i) / (float)hd);
        for (int t = 0; t < LM_MAX_POS; ++t) {
            const float fr = (float)t * inv;
            cs[((size_t)t * half + i) * 2] = (float)std::cos((double)fr);
            cs[((size_t)t * half + i) * 2 + 1] = (float)std::sin((double)fr);
        }
    }
    L.raw(&lm->rope, cs);
    // behind everything generate and score read: their weights keep the offsets they had
    L.vec(&lm->norm_w, "norm.weight", d);
    L.conv(&lm->head_raw, "output_head", V, d, 1, false);
    return L.upload();
}

struct LMBuffers {
    float *x, *hn, *qkv, *att, *g, *u;  // the prefill body (alloc_body)
    StepBufs step;                       // the fused decode step (alloc_step)
    float *kc, *vc;
    long long* tok;
    float *logits, *pmax;  // head, pick / sample of generate's step
    int* pidx;
    int* off;  // ragged generate, ragged session steps: per-row position offsets L_b - L_max <= 0 (lm_decode.h GemvArgs::off); nullptr everywhere else
    int* stop;  // generate with per-row semantic lengths: the rows' semantic steps (lm_decode.h GemvArgs::stop); nullptr everywhere else
    long long *ids_g, *ids_s;
    int cap;              // cache capacity
    size_t layer_stride;  // floats between two layers of kc / vc; 0: B * cap * d (generate's arena); a qa_lm_cache: max_batch * max_len * d
};

void alloc_body(Arena& a, LMBuffers& b, int64_t rows, int d, int I) {
    b.x = a.alloc<float>(rows * d);
    b.hn = a.alloc<float>(rows * d);
    b.qkv = a.alloc<float>(rows * 3 * d);
    b.att = a.alloc<float>(rows * d);
    b.g = a.alloc<float>(rows * I);
    b.u = a.alloc<float>(rows * I);
}

// The fused step's buffers for `rows` <= LM_MAX_ROWS rows over a cache of `cap` positions per row.  The attention's key split comes from
// the capacity alone (never from the batch or the step): att_split keys per split, more once four splits would not cover the cache.
// body == nullptr: x and u are allocated here like the rest.  body given (generate's chains only): s.x and s.u ALIAS body->x and body->u -
// the step runs on the first rows of the prefill buffers it follows, so a chain plans no second x / u.
void alloc_step(const qa_lm* lm, Arena& a, StepBufs& s, int rows, int cap, const LMBuffers* body = nullptr) {
    const int d = lm->spec.hidden, I = lm->spec.intermediate, H = lm->spec.n_heads;
    const int cap_tiles = (int)ceil_div(cap, 16);
    s.att_tps = std::max(lm->att_split / 16, (int)ceil_div(cap_tiles, 4));
    s.S_att = (int)ceil_div(cap_tiles, s.att_tps);
    s.x = body ? body->x : a.alloc<float>((size_t)rows * d);
    s.q = a.alloc<float>((size_t)rows * d);
    s.u = body ? body->u : a.alloc<float>((size_t)rows * I);
    s.att_part = a.alloc<float>((size_t)rows * H * s.S_att * (d / H + 4));
    s.mlp_part = a.alloc<float>(lm->mlp_fused ? (size_t)(I / lm->mlp_ac) * 32 * ceil_div(rows, 32) * d : 0);  // [row group][I / ac][32][d]
    s.state = a.alloc<int>(ST_WORDS);
}

// what a session step (qa_lm_forward, n = 1) hooks onto the layer loop of the fused step; generate passes none
struct StepIO {
    const float* x_in = nullptr;  // layer 0 reads these rows [B, d] (and adds them as its residual) instead of gathering codec_embedding[tok]
    float* hidden = nullptr;      // entry i <- the input of layer i, B rows each, entries `hidden_stride` floats apart (nullptr: no copies)
    size_t hidden_stride = 0;
};

struct SampleCfg {
    int do_sample;
    int top_k;
    float top_p, temperature;
    unsigned long long seed;
};

// Every projection of the prompt adapters, the prefill and the scoring pass runs on the implicit GEMM for EVERY row count: its tile
// configurations share one k order (test_conv_gemm_tile_configurations_are_bit_identical), so a sequence's prompt gets the same bits in
// any batch.  (The skinny kernel it took up to 32 rows sums in another order: a one-sequence call differed from the same sequence in a
// batch.)
//
// one pass of the Llama body over `n` new positions per sequence, positions pos0..pos0+n-1 (the prefill)
// one_cache: every layer writes its keys / values into the same [B, max_len, d] pair (scoring: nothing reads a layer's cache after the
// layer's own attention)
// hidden (qa_lm_forward with all_hidden): entry i [B, n, d] <- the input of layer i
// row_pos0 / row_n (device int [B], a ragged session chunk): sequence b's rows start at row_pos0[b] and only its first row_n[b] exist;
// pos0 is then the LONGEST row's, so pos0 + n bounds every row's keys
int lm_body(qa_lm* lm, Ctx& c, LMBuffers& b, int B, int n, int pos0, int max_len, bool skip_last_mlp, bool one_cache = false,
            float* hidden = nullptr, const int* row_pos0 = nullptr, const int* row_n = nullptr) {
    const qa_lm_spec& sp = lm->spec;
    const int d = sp.hidden, H = sp.n_heads, hd = d / H;
    const int64_t rows = (int64_t)B * n;
    const float scale = 1.0f / std::sqrt((float)hd);
    const size_t cache_stride = one_cache ? 0 : b.layer_stride ? b.layer_stride : (size_t)B * max_len * d;
    for (int i = 0; i < sp.n_layers; ++i) {
        const LMLayer& L = lm->layers[i];
        float* kc = b.kc + i * cache_stride;
        float* vc = b.vc + i * cache_stride;
        if (hidden && !c.dry)
            QA_HIP(hipMemcpyAsync(hidden + (size_t)i * rows * d, b.x, sizeof(float) * rows * d, hipMemcpyDeviceToDevice, c.stream));
        const bool last = skip_last_mlp && i == sp.n_layers - 1;  // prefill: only the KV cache of the last layer is consumed
        QA_TRY(rmsnorm_op(c, b.x, lm->ones, b.hn, rows, d, sp.rms_eps));
        QA_TRY(linear_op(c, b.hn, rows, L.qkv, b.qkv));
        QA_RUN(c, launch_rope_kv(b.qkv, lm->rope, kc, vc, B, n, H, hd, pos0, max_len, c.stream, row_pos0, row_n));
        if (last) break;
        AttnArgs at;  // the n new queries over the layer's KV cache, causal
        at.q = b.qkv; at.ldq = 3 * d; at.out = b.att; at.ldo = d;
        at.k = kc; at.v = vc; at.ldkv = d; at.kv_batch_stride = (long long)max_len * d;
        at.B = B; at.n_q = n; at.n_keys = pos0 + n; at.H = H; at.hd = hd;
        at.scale = scale; at.causal = 1;
        at.row_pos0 = row_pos0; at.row_nq = row_n;
        QA_TRY(attention_op(c, at));
        QA_TRY(linear_op(c, b.att, rows, L.o, b.x, epi(ACT_NONE, b.x)));
        QA_TRY(rmsnorm_op(c, b.x, lm->ones, b.hn, rows, d, sp.rms_eps));
        QA_TRY(linear_op(c, b.hn, rows, L.gate, b.g));
        QA_TRY(linear_op(c, b.hn, rows, L.up, b.u, epi(ACT_NONE, nullptr, nullptr, b.g)));
        QA_TRY(linear_op(c, b.u, rows, L.down, b.x, epi(ACT_NONE, b.x)));
    }
    return QA_OK;
}

// ONE decode step as 5 launches per layer + 2 (lm_decode.hip).  Everything step-dependent (position, ids column, RNG step) is read
// from b.state on the device, so the launch arguments are identical for every step of a phase: the sequence can be captured once
// into a hipGraph and replayed.
// fused_layers: the layers of the step (launches 1 - 5); [lo, lo + width): the head slice the last layer's prefetch plane warms
// (width 0: no head follows - a session step, which ends in the final RMSNorm instead)
// stop / col (the semantic phase of a generate with per-row semantic lengths): the rows' step counts and the step's column
int fused_layers(qa_lm* lm, const LMBuffers& b, int B, int lo, int width, hipStream_t s, int pos, const StepIO& io, const int* stop = nullptr,
                 int col = -1) {
    const qa_lm_spec& sp = lm->spec;
    const int d = sp.hidden, H = sp.n_heads, hd = d / H, I = sp.intermediate;
    const float scale = 1.0f / std::sqrt((float)hd);
    const StepBufs& sb = b.step;
    const long long kv_bstride = (long long)b.cap * d;
    const size_t cache_stride = b.layer_stride ? b.layer_stride : (size_t)B * b.cap * d;
    // key split of the attention launch: split sp owns the fixed tile range [sp, sp + 1) * sb.att_tps (lm_attn_kernel); a host-driven
    // step launches the splits that hold keys, a replayed one all of them (the others write identity records): same bits either way.
    // Ragged batch: `pos` is the LONGEST row's position, so the count covers every row; a shorter row's surplus splits are identity records
    const int S_att = pos >= 0 ? std::max(1, (int)ceil_div(ceil_div(pos + 1, 16), sb.att_tps)) : sb.S_att;
    // cross-launch prefetch (QA_LM_PF, lm_decode.h PfArgs): which launch carries the prefetch plane for which consumer
    const long long pfk = knob(K_LM_PF);
    const bool fused_mlp = lm->mlp_fused;
    auto pf_region = [](PfArgs& pf, int r, const float* w, long long tile_bytes, int n_tiles) {
        pf.p[r] = reinterpret_cast<const char*>(w);
        pf.tile_bytes[r] = tile_bytes;
        pf.n_tiles[r] = n_tiles;
    };
    auto pf_mlp = [&](PfArgs& pf, const LMLayer& L) {  // the fused MLP launch: workgroup j streams 2 gate/up tiles (32 rows) and W_down slice j
        if (!fused_mlp || !L.down_dec) return;
        pf_region(pf, 0, L.gu_dec, (long long)2 * lm->mlp_ac * d * 4, I / lm->mlp_ac);
        pf_region(pf, 1, L.down_dec, (long long)lm->mlp_ac * d * 4, I / lm->mlp_ac);
    };
    for (int i = 0; i < sp.n_layers; ++i) {
        const LMLayer& L = lm->layers[i];
        float* kc = b.kc + i * cache_stride;
        float* vc = b.vc + i * cache_stride;
        if (io.hidden)
            QA_HIP(hipMemcpyAsync(io.hidden + i * io.hidden_stride, i == 0 ? io.x_in : sb.x, sizeof(float) * B * d, hipMemcpyDeviceToDevice, s));
        GemvArgs a{};
        a.M = B; a.rms_eps = sp.rms_eps; a.state = sb.state; a.pos = pos; a.off = b.off; a.H = H; a.hd = hd; a.d = d;
        // o_proj's tile width (computed here: the qkv launch may prefetch its weights)
        int nt_o = lm->nt_o;
        if (gemv_r8_ok(d)) {
            if (B > 16 && nt_o < 8 && d % 8 == 0) nt_o = 8;
            if (B > 32 && nt_o < 16 && d % 16 == 0) nt_o = 16;
        }
        // 1. RMSNorm + QKV + RoPE + cache append; layer 0 gathers its input rows from codec_embedding (llm_sft.py:140,169)
        GemvArgs q = a;
        q.x = sb.x; q.ldx = d;
        if (i == 0 && io.x_in) q.x = io.x_in;
        else if (i == 0) { q.tok = b.tok; q.table = lm->codec_emb; }
        q.w = L.qkv_dec; q.N = 3 * d; q.K = d;
        q.rope = lm->rope; q.q = sb.q; q.kc = kc; q.vc = vc; q.kv_bstride = kv_bstride;
        q.stop = stop; q.col = col;
        PfArgs qpf{};
        if (pfk & 1) pf_region(qpf, 0, L.o.w, (long long)nt_o * d * 4, d / nt_o);
        QA_TRY(launch_lm_gemv(q, GM_QKV, lm->nt_qkv, s, &qpf));
        // 2. attention over the cache (pos + 1 keys), split over S_att workgroups per (sequence, head)
        QA_TRY(launch_lm_attn(sb.q, d, kc, vc, kv_bstride, d, sb.att_part, B, H, hd, S_att, sb.att_tps, sb.state, scale, pos, s, b.off, stop, col));
        // 3. merge of the partials + o_proj + residual
        GemvArgs o = a;
        o.att_part = sb.att_part; o.S = S_att;
        o.w = L.o.w; o.N = d; o.K = d; o.ldx = d;
        if (i == 0 && io.x_in) { o.res = io.x_in; }
        else if (i == 0) { o.res_tok = b.tok; o.res_table = lm->codec_emb; } else { o.res = sb.x; }
        o.ldr = d; o.y = sb.x; o.ldy = d;
        // tile width by the batch: the 8-row groups (lm_gemv4_kernel R8) hold a workgroup's pull of attention partials at 52 KB whatever the
        // batch, but every column tile re-reads and re-merges the partials of its rows - so the launch keeps ~256 workgroups: 4 columns x 2
        // row groups at 16 sequences, 8 x 4 at 32, 16 x 8 at 64 (r05 A/B, generate ms at 16 / 32 / 64 sequences: width 4 110.4 / 147.4 / 206.5,
        // width 8 113.1 / 143.7 / 198.6, width 16 118.5 / 149.2 / 196.4; profiles/r05_lm_oproj_ab.txt)
        PfArgs opf{};
        if (pfk & 2) pf_mlp(opf, L);
        QA_TRY(launch_lm_gemv(o, GM_RESID, nt_o, s, &opf));
        // 4. RMSNorm + gate / up + SwiGLU
        GemvArgs g = a;
        g.x = sb.x; g.ldx = d; g.w = L.gu_dec; g.N = 2 * I; g.K = d; g.y = sb.u; g.ldy = I;
        if (lm->mlp_fused && L.down_dec) {  // 4 + 5 as the fused MLP launch + the reduce launch (lm_decode.hip)
            PfArgs gpf{};
            if (pfk & 4) {
                if (i + 1 < sp.n_layers) pf_region(gpf, 0, lm->layers[i + 1].qkv_dec, (long long)lm->nt_qkv * d * 4, 3 * d / lm->nt_qkv);
                else if (width > 0) pf_region(gpf, 0, lm->head.w + (size_t)lo * d, (long long)head_nt(width) * d * 4, width / head_nt(width));
            }
            QA_TRY(launch_lm_mlp(g, I, lm->mlp_ac, L.down_dec, sb.mlp_part, sb.x, d, sb.x, d, s, &gpf));
            continue;
        }
        QA_TRY(launch_lm_gemv(g, GM_GATEUP, lm->nt_gu, s));
        // 5. down_proj + residual
        GemvArgs dn = a;
        dn.x = sb.u; dn.ldx = I; dn.w = L.down.w; dn.N = d; dn.K = I; dn.res = sb.x; dn.ldr = d; dn.y = sb.x; dn.ldy = d;
        QA_TRY(launch_lm_gemv(dn, GM_RESID, lm->nt_down, s));
    }
    return QA_OK;
}

// the whole step of generate: the layers, then head and pick / sample (launches 6 - 7)
// tap (taps on): [B][tap_cols][width] logits of the phase's steps for these B rows, column = the step's col
int fused_step(qa_lm* lm, const LMBuffers& b, int B, int lo, int width, long long* ids, int ids_ld, int keep, const SampleCfg& sc,
               hipStream_t s, int pos, int col,  // pos / col >= 0: host-driven loop; -1: read from the device state (captured step)
               float* tap, int tap_cols, const int* stop = nullptr) {  // stop: as fused_layers, read with this step's `col`
    const qa_lm_spec& sp = lm->spec;
    const int d = sp.hidden, H = sp.n_heads, hd = d / H;
    QA_TRY(fused_layers(lm, b, B, lo, width, s, pos, StepIO(), stop, col));
    // 6. final RMSNorm (weight folded into output_head) + the rows of output_head inside the active vocabulary slice (the range
    //    mask of llm_sft.py:150-153 / :180-182 sets everything else to -inf) + per-tile arg-max
    const int nt = head_nt(width);
    GemvArgs hg{};
    hg.M = B; hg.rms_eps = sp.rms_eps; hg.state = b.step.state; hg.pos = pos; hg.H = H; hg.hd = hd; hg.d = d;
    hg.x = b.step.x; hg.ldx = d; hg.w = lm->head.w + (size_t)lo * d; hg.N = width; hg.K = d;
    hg.pmax = b.pmax; hg.pidx = b.pidx; hg.logits = (sc.do_sample || tap) ? b.logits : nullptr; hg.ldl = width;
    PfArgs hpf{};
    if (knob(K_LM_PF) & 8) {  // the next step's first weights (QA_LM_PF, as in fused_layers)
        hpf.p[0] = reinterpret_cast<const char*>(lm->layers[0].qkv_dec);
        hpf.tile_bytes[0] = (long long)lm->nt_qkv * d * 4;
        hpf.n_tiles[0] = 3 * d / lm->nt_qkv;
    }
    QA_TRY(launch_lm_gemv(hg, GM_HEAD, nt, s, &hpf));
    if (tap) QA_TRY(launch_lm_tap(b.logits, width, B, tap, tap_cols, b.step.state, col, s, stop));
    // 7. next token
    if (!sc.do_sample) {
        QA_TRY(launch_lm_pick(b.pmax, b.pidx, width / nt, B, lo, b.tok, ids, ids_ld, keep, b.step.state, col, s, stop));
    } else {
        QA_TRY(launch_lm_sample(b.logits, width, width, B, lo, sc.top_k, sc.top_p, sc.temperature, 1, b.tok, ids, ids_ld, keep, b.step.state, s, stop));
        QA_TRY(launch_lm_advance(b.step.state, s));
    }
    return QA_OK;
}

uint64_t mix_key(uint64_t h, uint64_t v) {
    h ^= v + 0x9E3779B97F4A7C15ull + (h << 6) + (h >> 2);
    return h;
}

// QA_LM_GRAPH=1: replay one captured step per token instead of launching its kernels from the host.  Measured equal within 1 %
// on MI355X (the step is bound by its ~62 dependent kernels, not by the host), and a replayed step must read the position from
// device memory - one more dependent load per kernel - and cannot size the attention grid to the current key count: off by default.
bool use_graphs() { return knob(K_LM_GRAPH) != 0; }

// One chain = one batch of <= 64 sequences (LM_MAX_ROWS) with its own buffers, KV cache and (for B > 64, or QA_LM_CHAINS) its own internal stream.
struct Chain {
    int b0 = 0, B = 0;  // sequences [b0, b0 + B) of the call
    LMBuffers b{};
    float *emix = nullptr, *eenr = nullptr;
    int* ints = nullptr;  // per-row mixture / semantic lengths only: the chain's GR_* arrays (write_gen_ints)
    int steps_s = 0;      // semantic steps of THIS chain: its longest row's
    hipStream_t s = nullptr;
};

// The prompt of a call, as every entry point that builds one describes it.  cond_mode: CustomLlamaModel's [mix_sos, cond] (cond
// [B, Tc, d], already in the LM's width) or nothing (Tc = 0); otherwise LLM_SFT's [task, (enroll_sos, enroll)?, mix_sos, mix] from
// features the adapter still has to project.  ne_rows (HOST, [B]; ragged generate, DESIGN.md sections 23 and 37): row b's enrollment frames,
// 1 .. Ne - or, in cond_mode, its condition frames, 1 .. Tc - the prompt is then laid out for the LONGEST possible row (Ne / Tc frames)
struct Prompt {
    bool cond_mode = false;
    const float* cond = nullptr; int Tc = 0;
    int task = 0;
    const float* enroll = nullptr; int Ne = 0;  // nullptr and 0: no enrollment
    const float* mix = nullptr; int Nm = 0;
    const int* ne_rows = nullptr;
    // generate with per-row mixture lengths (HOST, [B]): row b's mixture frames, 1 .. Nm.  ne_rows is then given too
    // (every entry Ne where the caller passed no n_enroll), and the prompt is assembled per row the way the scoring calls assemble theirs
    const int* nm_rows = nullptr;
};

Prompt speech_prompt(int32_t task, const float* enroll_feats, int64_t n_enroll, const float* mix_feats, int64_t n_mix) {
    Prompt p;
    p.task = task;
    p.enroll = enroll_feats; p.Ne = enroll_feats ? (int)n_enroll : 0;
    p.mix = mix_feats; p.Nm = (int)n_mix;
    return p;
}
Prompt cond_prompt(const float* cond_embeds, int64_t T) {
    Prompt p;
    p.cond_mode = true;
    p.cond = cond_embeds; p.Tc = (int)T;
    return p;
}

int prompt_len(const Prompt& p) { return p.cond_mode ? (p.Tc > 0 ? p.Tc + 1 : 0) : 1 + (p.enroll ? 1 + p.Ne : 0) + 1 + p.Nm; }

// The prompt rows (llm_sft.py:110-128 / llm.py:301-306) of sequences [b0, b0 + gb) into out [gb, prompt_len, d], on c.stream.  emix /
// eenr: the adapter's output for these rows; off (ragged only, [gb], device) receives their position offsets.  Ragged: the adapter also
// runs over the padding frames (a GEMM row depends on its own input row alone) and assemble_prompt never copies their outputs.
// the adapter over the mixture and enrollment frames of sequences [b0, b0 + gb) of a speech prompt -> emix [gb, Nm, d], eenr [gb, Ne, d]
int adapt_prompt(qa_lm* lm, Ctx& c, const Prompt& p, int b0, int gb, float* emix, float* eenr) {
    const int F = lm->spec.feats_dim;
    QA_TRY(linear_op(c, p.mix + (size_t)b0 * p.Nm * F, (int64_t)gb * p.Nm, lm->adapter, emix));
    if (p.enroll) QA_TRY(linear_op(c, p.enroll + (size_t)b0 * p.Ne * F, (int64_t)gb * p.Ne, lm->adapter, eenr));
    return QA_OK;
}

// the speech prompt's members of a per-row assembly pass (score_rows_graph, prompt_call): adapter outputs and the group's device counts
void speech_assemble(ScoreAssembleArgs& as, const qa_lm* lm, const Prompt& p, const float* emix, const float* eenr, const int* ne_r,
                     const int* nm_r) {
    as.task_vec = lm->task_emb + (size_t)p.task * lm->spec.hidden;
    as.enroll_sos = p.enroll ? lm->enroll_sos : nullptr; as.enroll_emb = eenr; as.Ne = p.Ne; as.ne_r = ne_r;
    as.mix_sos = lm->mix_sos; as.mix_emb = emix; as.Nm = p.Nm; as.nm_r = nm_r;
}

// rows_r (p.nm_rows only; device, written by the caller): the group's [ne | nm] counts, gb entries each, beside the offsets already in `off`
int build_prompt(qa_lm* lm, Ctx& c, const Prompt& p, int b0, int gb, float* emix, float* eenr, float* out, int* off,
                 const int* rows_r = nullptr) {
    const int d = lm->spec.hidden;
    if (p.cond_mode) {
        if (p.ne_rows) QA_RUN(c, launch_lm_offsets(off, p.ne_rows + b0, p.Tc, gb, c.stream));
        if (p.Tc > 0) QA_RUN(c, launch_cond_prompt(out, lm->mix_sos, p.cond + (size_t)b0 * p.Tc * d, gb, p.Tc, d, c.stream, off));
        return QA_OK;
    }
    QA_TRY(adapt_prompt(lm, c, p, b0, gb, emix, eenr));
    if (p.nm_rows) {  // row b left-aligned over its own Lp_b positions, zeros behind: the scoring calls' assembly, without a table
        ScoreAssembleArgs as;
        as.x = out; as.n = prompt_len(p); as.B = gb; as.d = d;
        speech_assemble(as, lm, p, emix, eenr, rows_r, rows_r + gb);
        QA_RUN(c, launch_lm_score_assemble(as, c.stream));
        return QA_OK;
    }
    if (p.ne_rows) QA_RUN(c, launch_lm_offsets(off, p.ne_rows + b0, p.Ne, gb, c.stream));
    QA_RUN(c, launch_assemble_prompt(out, lm->task_emb + (size_t)p.task * d, p.enroll ? lm->enroll_sos : nullptr, eenr, lm->mix_sos, emix, gb,
                                     p.Ne, p.Nm, d, c.stream, off));
    return QA_OK;
}

struct GenArgs {
    Prompt p;
    int B, G, S;
    SampleCfg sc;
    int64_t *gids, *sids;
    // per-row semantic lengths (HOST, [B], 0 .. S): row b takes stop_rows[b] semantic steps, S is then the ids' stride
    // and the longest possible row's count.  nullptr: every row takes S
    const int* stop_rows = nullptr;
};

// The device ints of one chain of a generate with per-row mixture or semantic lengths, GR_COUNT arrays of `B` entries each behind one another
enum { GR_OFF = 0, GR_NE, GR_NM, GR_STOP, GR_COUNT };

void chain_alloc(qa_lm* lm, Ctx& c, Chain& ch, const GenArgs& a, int L, int cap) {
    const qa_lm_spec& sp = lm->spec;
    const int d = sp.hidden, B = ch.B;
    const int64_t prow = (int64_t)B * std::max(L, 1);  // L = 0: the empty prompt of CustomLlamaModel.generate(cond=None); a step still needs its row
    LMBuffers& b = ch.b;
    b.cap = cap;
    alloc_body(c.arena, b, prow, d, sp.intermediate);
    const int wmax = std::max(sp.global_size, sp.semantic_size);
    b.logits = c.arena.alloc<float>((size_t)B * wmax);
    b.kc = c.arena.alloc<float>((size_t)sp.n_layers * B * cap * d);
    b.vc = c.arena.alloc<float>((size_t)sp.n_layers * B * cap * d);
    b.tok = c.arena.alloc<long long>(B);
    alloc_step(lm, c.arena, b.step, B, cap, &b);  // b.step.x and b.step.u are b.x and b.u, not allocations of their own
    b.pmax = c.arena.alloc<float>((size_t)B * (wmax / 4 + 1));
    b.pidx = c.arena.alloc<int>((size_t)B * (wmax / 4 + 1));
    b.ids_g = c.arena.alloc<long long>((size_t)B * std::max(a.G, 1));
    b.ids_s = c.arena.alloc<long long>((size_t)B * std::max(a.S, 1));
    ch.emix = c.arena.alloc<float>((size_t)B * a.p.Nm * d);
    ch.eenr = a.p.enroll ? c.arena.alloc<float>((size_t)B * a.p.Ne * d) : nullptr;
    // last, and only then: the buffers of THIS chain lie where a rectangular call has them.  A later chain's move with the ints in front
    // of them (none, B or GR_COUNT * B), which is why the step-graph key holds the chain's addresses (generate_graph)
    if (a.p.nm_rows || a.stop_rows) {
        int* ints = c.arena.alloc<int>((size_t)GR_COUNT * B);
        b.off = a.p.nm_rows ? ints + GR_OFF * B : nullptr;
        b.stop = a.stop_rows ? ints + GR_STOP * B : nullptr;
        ch.ints = ints;
    } else {
        b.off = a.p.ne_rows ? c.arena.alloc<int>(B) : nullptr;
    }
}

// the chain's per-row ints (GR_*) in one upload: offsets Lp_b - Lp_max, the rows' frame counts for the assembly, the rows' semantic steps
int write_gen_ints(const Chain& ch, const GenArgs& a) {
    static_assert(GR_COUNT * LM_MAX_ROWS <= ROW_INTS_CHUNK, "the ints of a chain are one launch");
    const Prompt& p = a.p;
    std::vector<int> vals((size_t)GR_COUNT * ch.B, 0);
    for (int i = 0; i < ch.B; ++i) {
        const int b = ch.b0 + i;
        if (p.nm_rows) {
            vals[(size_t)GR_NE * ch.B + i] = p.enroll ? p.ne_rows[b] : 0;
            vals[(size_t)GR_NM * ch.B + i] = p.nm_rows[b];
            vals[(size_t)GR_OFF * ch.B + i] = (p.enroll ? p.ne_rows[b] - p.Ne : 0) + p.nm_rows[b] - p.Nm;
        }
        if (a.stop_rows) vals[(size_t)GR_STOP * ch.B + i] = a.stop_rows[b];
    }
    return launch_row_ints(ch.ints, vals.data(), (long long)vals.size(), ch.s);
}

// r05: up to 64 sequences are ONE chain - every GEMV / fused-MLP launch of the step carries two row groups of 32 (gridDim.y, lm_decode.hip
// row_group), so the step streams the 217 MB of weights once and issues 50 launches where two chains of 32 issued 100.
// Batches of more than 64 sequences run as ceil(B / 64) independent CHAINS
// on internal streams: a decode step is bound by the latency of its ~62 dependent launches and leaves the device almost idle
// (DESIGN.md section 11), so chains overlap nearly for free - tokens/s scales with the number of chains until the CUs fill.  Every
// chain replays ONE captured step per token (hipGraph), round-robin over the chains, so the host issues two graph launches per
// step instead of 124 kernel launches (eager launches go host-bound below ~3 us per kernel).  QA_LM_CHAINS forces a chain count.
// cond_mode: CustomLlamaModel.generate (llm.py:291-374) - the global phase runs exactly G steps: its last token is returned but never
// fed (llm.py:318,345)
int generate_graph(qa_lm* lm, Ctx& c, const GenArgs& a) {
    // ragged: L, pos and the capacity below are the LONGEST possible row's; the rows' own positions follow from the per-chain offsets b.off
    const qa_lm_spec& sp = lm->spec;
    const Prompt& p = a.p;
    const SampleCfg& sc = a.sc;
    const int B = a.B, G = a.G, S = a.S;
    const int L = prompt_len(p);
    const int Gs = p.cond_mode ? G : G + 1;  // steps of the global phase
    const int max_len = L + Gs + S;
    QA_REQUIRE(max_len <= LM_MAX_POS, "generate: %d positions exceed max_position_embeddings %d", max_len, LM_MAX_POS);
    const int cap = (int)round_up(max_len, 64);  // cache row stride: shapes that round alike share their captured step graphs
    // A caller that is CAPTURING its stream into a hipGraph gets the plain single-chain launches on that stream only: no
    // internal streams, no capture of our own inside theirs (the multi-chain replay path would fail there where the eager path works).
    const bool capturing = stream_capturing(c.stream);
    int nc = (int)knob(K_LM_CHAINS);
    if (nc <= 0) nc = (int)ceil_div(B, LM_MAX_ROWS);  // r05: one chain serves up to 64 sequences (two row groups per launch)
    if (capturing) nc = 1;
    nc = std::max(1, std::min(std::min(nc, B), LM_MAX_CHAINS));
    if (ceil_div(B, nc) > LM_MAX_ROWS) nc = (int)ceil_div(B, LM_MAX_ROWS);  // a forced count (or a capturing caller) that would put > 64 sequences in a chain
    QA_REQUIRE(!capturing || nc == 1, "generate: a caller that captures its stream can pass at most %d sequences per call (got %d)", LM_MAX_ROWS, B);
    const int cb = (int)ceil_div(B, nc);
    nc = (int)ceil_div(B, cb);
    std::vector<Chain> chains(nc);
    for (int i = 0; i < nc; ++i) {
        chains[i].b0 = i * cb;
        chains[i].B = std::min(cb, B - i * cb);
        chain_alloc(lm, c, chains[i], a, L, cap);
        chains[i].steps_s = S;
        if (a.stop_rows) chains[i].steps_s = *std::max_element(a.stop_rows + chains[i].b0, a.stop_rows + chains[i].b0 + chains[i].B);
    }
    if (c.dry) return QA_OK;  // real-pass-only remainder: chain_alloc above made the function's last arena allocations
    // taps: logits.global [B][G + 1][global_size], then logits.semantic [B][S][semantic_size]
    float* const tap_base = lm->taps ? reinterpret_cast<float*>(lm->tap_buf.ptr) : nullptr;
    if (a.stop_rows && tap_base && S > 0)  // exact zeros behind every row's own steps (lm_tap_kernel skips a retired row); ahead of the fork
        QA_HIP(hipMemsetAsync(tap_base + (size_t)B * Gs * sp.global_size, 0, sizeof(float) * (size_t)B * S * sp.semantic_size, c.stream));
    const bool multi = nc > 1;
    if (multi) {  // fork: the chains' streams start behind everything already queued on the caller's stream
        while ((int)lm->chain_streams.size() < nc) {
            hipStream_t st = nullptr;
            hipEvent_t ev = nullptr;
            QA_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
            QA_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
            lm->chain_streams.push_back(st);
            lm->chain_join.push_back(ev);
        }
        if (!lm->ev_fork) QA_HIP(hipEventCreateWithFlags(&lm->ev_fork, hipEventDisableTiming));
        QA_HIP(hipEventRecord(lm->ev_fork, c.stream));
        for (int i = 0; i < nc; ++i) {
            chains[i].s = lm->chain_streams[i];
            QA_HIP(hipStreamWaitEvent(chains[i].s, lm->ev_fork, 0));
        }
    } else {
        chains[0].s = c.stream;
    }
    hipStream_t caller = c.stream;

    // ---- prompt (llm_sft.py:110-128) and prefill (llm_sft.py:130-135), chain by chain (these launches fill the device by themselves)
    for (Chain& ch : chains) {
        c.stream = ch.s;
        int st = ch.ints ? write_gen_ints(ch, a) : QA_OK;
        // -1 behind every row's own steps: the fill stays wherever lm_pick_kernel / lm_sample_kernel store nothing
        if (st == QA_OK && a.stop_rows && S > 0 && hipMemsetAsync(ch.b.ids_s, 0xff, sizeof(long long) * (size_t)ch.B * S, ch.s) != hipSuccess) {
            set_error("generate: hipMemsetAsync of the semantic ids failed");
            st = QA_ERR_HIP;
        }
        if (st == QA_OK)
            st = build_prompt(lm, c, p, ch.b0, ch.B, ch.emix, ch.eenr, ch.b.x, ch.b.off, ch.ints ? ch.ints + GR_NE * ch.B : nullptr);
        // Ragged: the prefill runs unchanged over L = L_max positions and needs NO mask.  It is causal, so a valid query (position < L_b)
        // never sees a key behind itself, least of all the zero rows at L_b .. L - 1.  The queries of those zero rows are finite garbage
        // that nothing consumes (the prefill's last hidden state is not used, only its K / V), and the K / V rows they leave at L_b + t
        // are overwritten by decode step t before that step - the first to count them among its L_b + t + 1 keys - reads them.
        if (st == QA_OK && L > 0) st = lm_body(lm, c, ch.b, ch.B, L, 0, cap, true);
        c.stream = caller;
        QA_TRY(st);
    }

    // ---- decode: G+1 global tokens (the last is fed to the cache but discarded), then S semantic tokens
    int pos = L;
    const bool graphs = !capturing && (multi || use_graphs());
    auto phase = [&](int which, long long first_id, int steps, int lo, int width, int keep) -> int {
        const int ids_ld = keep;
        // the semantic phase alone reads the rows' stops, and drives each chain for its own longest row (steps: the tap's and the ids' stride)
        auto chain_stop = [&](const Chain& ch) -> const int* { return which == 1 ? ch.b.stop : nullptr; };
        auto chain_steps = [&](const Chain& ch) { return which == 1 ? ch.steps_s : steps; };
        float* const tap = tap_base ? tap_base + (which == 0 ? 0 : (size_t)B * Gs * sp.global_size) : nullptr;
        auto chain_tap = [&](const Chain& ch) { return tap ? tap + (size_t)ch.b0 * steps * width : nullptr; };
        for (Chain& ch : chains)
            QA_TRY(launch_lm_phase_init(ch.b.tok, first_id, ch.B, ch.b.step.state, pos, which == 0, sc.seed, ch.b0, ch.s));
        if (graphs && steps > 0) {
            if ((int)lm->graphs.size() < 2 * nc) lm->graphs.resize(2 * nc);
            for (int i = 0; i < nc; ++i) {
                Chain& ch = chains[i];
                if (chain_steps(ch) == 0) continue;
                long long* ids = which == 0 ? ch.b.ids_g : ch.b.ids_s;
                StepGraph& g = lm->graphs[2 * i + which];
                uint64_t key = 0x51ull;
                for (uint64_t v : {(uint64_t)(uintptr_t)lm->ws.ptr, (uint64_t)B, (uint64_t)nc, (uint64_t)ch.b0, (uint64_t)ch.B, (uint64_t)cap, (uint64_t)L,
                                   (uint64_t)G, (uint64_t)S, (uint64_t)p.Ne, (uint64_t)p.Nm, (uint64_t)(p.enroll != nullptr), (uint64_t)lo, (uint64_t)width, (uint64_t)keep, (uint64_t)sc.do_sample,
                                   (uint64_t)sc.top_k, (uint64_t)(sc.top_p * 1e6f), (uint64_t)(sc.temperature * 1e6f), (uint64_t)knob(K_LM_PF),
                                   (uint64_t)knob(K_LM_ROWSPLIT), (uint64_t)(uintptr_t)chain_tap(ch), (uint64_t)p.cond_mode,
                                   // ragged or not, stop or not - never the lengths: they live in device memory (b.off, b.stop).  The
                                   // ADDRESSES, and the chain's first buffer with them: chain_alloc ends a chain with no ints, B ints or
                                   // GR_COUNT * B ints, so the buffers of chain i >= 1 lie where the call kind of chain i - 1 put them,
                                   // and a step captured at one layout must never be replayed at another
                                   (uint64_t)(uintptr_t)ch.b.x, (uint64_t)(uintptr_t)ch.b.off, (uint64_t)(uintptr_t)chain_stop(ch)})
                    key = mix_key(key, v);
                if (!g.exec || g.key != key) {
                    g.reset();
                    if (!lm->cap_stream) QA_HIP(hipStreamCreateWithFlags(&lm->cap_stream, hipStreamNonBlocking));
                    QA_HIP(hipStreamBeginCapture(lm->cap_stream, hipStreamCaptureModeThreadLocal));
                    const int st = fused_step(lm, ch.b, ch.B, lo, width, ids, ids_ld, keep, sc, lm->cap_stream, -1, -1, chain_tap(ch), steps,
                                              chain_stop(ch));
                    hipGraph_t graph = nullptr;
                    const hipError_t e = hipStreamEndCapture(lm->cap_stream, &graph);
                    if (st != QA_OK) {
                        if (graph) (void)hipGraphDestroy(graph);
                        return st;
                    }
                    QA_HIP(e);
                    g.graph = graph;
                    QA_HIP(hipGraphInstantiate(&g.exec, graph, nullptr, nullptr, 0));
                    g.key = key;
                }
            }
            for (int st = 0; st < steps; ++st)  // round-robin: every chain advances one token per turn
                for (int i = 0; i < nc; ++i)
                    if (st < chain_steps(chains[i])) QA_HIP(hipGraphLaunch(lm->graphs[2 * i + which].exec, chains[i].s));
            pos += steps;
            return QA_OK;
        }
        for (int st = 0; st < steps; ++st)
            for (Chain& ch : chains)
                if (st < chain_steps(ch))
                    QA_TRY(fused_step(lm, ch.b, ch.B, lo, width, which == 0 ? ch.b.ids_g : ch.b.ids_s, ids_ld, keep, sc, ch.s, pos + st, st,
                                      chain_tap(ch), steps, chain_stop(ch)));
        pos += steps;
        return QA_OK;
    };
    QA_TRY(phase(0, 0, Gs, 3, sp.global_size, G));                               // llm_sft.py:137-164 / llm.py:316-343
    QA_TRY(phase(1, 1, S, 3 + sp.global_size, sp.semantic_size, S));            // llm_sft.py:166-193
    for (int i = 0; i < nc; ++i) {
        Chain& ch = chains[i];
        if (G > 0)
            QA_HIP(hipMemcpyAsync(a.gids + (size_t)ch.b0 * G, ch.b.ids_g, sizeof(long long) * (size_t)ch.B * G, hipMemcpyDeviceToDevice, ch.s));
        if (S > 0)
            QA_HIP(hipMemcpyAsync(a.sids + (size_t)ch.b0 * S, ch.b.ids_s, sizeof(long long) * (size_t)ch.B * S, hipMemcpyDeviceToDevice, ch.s));
        if (multi) {  // join: the caller's stream continues behind every chain
            QA_HIP(hipEventRecord(lm->chain_join[i], ch.s));
            QA_HIP(hipStreamWaitEvent(caller, lm->chain_join[i], 0));
        }
    }
    return QA_OK;
}

// ---- teacher-forced scoring (llm_sft.py:37-90).  Sequences go through in groups of at most LM_MAX_ROWS (the workspace stays bounded;
// every stage is batch-invariant, so a group boundary changes no bit).  Per group: adapters + prompt (as generate) and the codec_embedding
// rows of input_ids behind it, the body over all Lp + Lt positions from position 0 with every layer, the final RMSNorm on the Lt target
// rows, then output_head over the full vocabulary in chunks of QA_LM_SCORE_ROWS rows, each reduced by the row-loss kernel right behind it.
struct ScoreArgs {
    Prompt p;  // cond_mode: CustomLlamaModel.forward (llm.py:107-147), prompt [mix_sos, cond] or none, the last position dropped
    int B, G, T;
    const long long *gids, *sids;
    double eps;
    float* loss_seq;
    long long* correct_seq;
    float *loss, *acc;
    // per-row lengths (qa_lm_score_ragged): p.Ne / p.Nm / T are then the tensors' widths.  nullptr: rectangular
    const ScoreRows* rows = nullptr;
};

int score_rows_graph(qa_lm* lm, Ctx& c, const ScoreArgs& a, float* tap);

int score_graph(qa_lm* lm, Ctx& c, const ScoreArgs& a, float* tap) {
    const qa_lm_spec& sp = lm->spec;
    const int d = sp.hidden, V = vocab_of(sp);
    const Prompt& p = a.p;
    if (a.rows) return score_rows_graph(lm, c, a, tap);
    const int Lp = prompt_len(p);
    const int Lt = a.G + a.T + 2 - (p.cond_mode ? 1 : 0), n = Lp + Lt;
    QA_REQUIRE(n <= LM_MAX_POS, "qa_lm_score: %d positions (prompt %d + targets %d) exceed max_position_embeddings %d", n, Lp, Lt, LM_MAX_POS);
    const int GB = std::min(a.B, LM_MAX_ROWS);
    const int64_t prow = (int64_t)GB * n, trow = (int64_t)GB * Lt;
    const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(knob(K_LM_SCORE_ROWS), trow));
    LMBuffers b{};
    // b.hn is also the assembled prompt (before the body) and the normalised target rows (after it), b.att the compacted target rows
    alloc_body(c.arena, b, prow, d, sp.intermediate);
    b.kc = c.arena.alloc<float>(prow * d);   // one layer's cache, shared by all layers (lm_body one_cache)
    b.vc = c.arena.alloc<float>(prow * d);
    float* emix = c.arena.alloc<float>((size_t)GB * p.Nm * d);
    float* eenr = p.enroll ? c.arena.alloc<float>((size_t)GB * p.Ne * d) : nullptr;
    long long* tgt = c.arena.alloc<long long>(trow);
    float* row_kl = c.arena.alloc<float>(trow);
    int* row_ok = c.arena.alloc<int>(trow);
    float* logits = c.arena.alloc<float>((size_t)chunk * V);
    double* seq_sum = c.arena.alloc<double>(a.B);
    if (c.dry) return QA_OK;  // real-pass-only remainder: seq_sum above is the function's last arena allocation
    // the reference's true_dist is fp32: confidence 1 - eps and eps / (V - 1) filled into a float tensor (llm.py:95-98)
    const float conf = (float)(1.0 - a.eps), smooth = (float)(a.eps / (V - 1));
    for (int b0 = 0; b0 < a.B; b0 += GB) {
        const int gb = std::min(GB, a.B - b0);
        QA_TRY(build_prompt(lm, c, p, b0, gb, emix, eenr, b.hn, nullptr));
        if (Lp > 0)
            QA_HIP(hipMemcpy2DAsync(b.x, sizeof(float) * n * d, b.hn, sizeof(float) * Lp * d, sizeof(float) * Lp * d, gb, hipMemcpyDeviceToDevice,
                                    c.stream));
        QA_TRY(launch_lm_targets(b.x + (size_t)Lp * d, (long long)n * d, lm->codec_emb, a.gids + (size_t)b0 * a.G, a.G, a.sids + (size_t)b0 * a.T,
                                 a.T, V, 3, 3 + sp.global_size, tgt, gb, d, c.stream, p.cond_mode ? 1 : 0));
        QA_TRY(lm_body(lm, c, b, gb, n, 0, n, false, true));
        // final RMSNorm (its weight is folded into output_head) on the last Lt rows of every sequence (llm_sft.py:82)
        QA_HIP(hipMemcpy2DAsync(b.att, sizeof(float) * Lt * d, b.x + (size_t)Lp * d, sizeof(float) * n * d, sizeof(float) * Lt * d, gb,
                                hipMemcpyDeviceToDevice, c.stream));
        const int64_t rows = (int64_t)gb * Lt;
        QA_TRY(launch_rmsnorm(b.att, lm->ones, b.hn, rows, d, sp.rms_eps, c.stream));
        // output_head, V = 3 + global + semantic columns (odd for the UniSE vocabulary: the GEMM's scalar epilogue, no padding)
        for (int64_t r0 = 0; r0 < rows; r0 += chunk) {
            const int64_t nr = std::min(chunk, rows - r0);
            QA_TRY(linear_op(c, b.hn + (size_t)r0 * d, nr, lm->head, logits));
            QA_TRY(launch_lm_row_loss(logits, V, V, nr, tgt + r0, conf, smooth, row_kl + r0, row_ok + r0, c.stream));
            if (tap)
                QA_HIP(hipMemcpyAsync(tap + ((size_t)b0 * Lt + r0) * V, logits, sizeof(float) * nr * V, hipMemcpyDeviceToDevice, c.stream));
        }
        QA_TRY(launch_lm_seq_reduce(row_kl, row_ok, gb, Lt, seq_sum + b0, a.loss_seq + b0, a.correct_seq + b0, c.stream));
    }
    return launch_lm_batch_reduce(seq_sum, a.correct_seq, a.B, Lt, a.loss, a.acc, c.stream);
}

// The device ints of one group of a ragged score / prompt call, SR_COUNT arrays of `gb` entries each behind one another
enum { SR_NE = 0, SR_NM, SR_T, SR_OFF, SR_LP, SR_L, SR_ZERO, SR_COUNT };

int write_score_ints(int* dst, const ScoreRows& R, const ScoreGroup& g, hipStream_t s) {
    std::vector<int> vals((size_t)SR_COUNT * g.gb, 0);
    for (int i = 0; i < g.gb; ++i) {
        const size_t b = (size_t)g.b0 + i;
        vals[(size_t)SR_NE * g.gb + i] = R.ne[b];
        vals[(size_t)SR_NM * g.gb + i] = R.nm[b];
        vals[(size_t)SR_T * g.gb + i] = R.T[b];
        vals[(size_t)SR_OFF * g.gb + i] = (int)(R.off[b] - g.row0);  // inside the group: at most gb * LM_MAX_POS
        vals[(size_t)SR_LP * g.gb + i] = R.Lp[b];
        vals[(size_t)SR_L * g.gb + i] = R.L[b];
    }
    return launch_row_ints(dst, vals.data(), (long long)vals.size(), s);
}

// score_graph with per-row lengths.  The same structure - groups of at most LM_MAX_ROWS sequences in index order,
// adapters, assembly, body, final norm, head in QA_LM_SCORE_ROWS chunks, row loss, fixed-order reduces - with these differences: a group is
// laid out at its OWN longest row; one assembly pass writes prompt, input embeddings and the packed targets; the body runs with the rows'
// counts (a query block wholly behind a row's length exits at once, K / V behind it are not written); and the tail - norm, head, row loss -
// runs over the PACKED target rows alone, so no padded row reaches the full-vocabulary head.
// cond_mode (qa_lm_score_cond_ragged): no adapter - the condition embeddings are the prompt's frames as they are - and
// a row's own last position dropped.
int score_rows_graph(qa_lm* lm, Ctx& c, const ScoreArgs& a, float* tap) {
    const qa_lm_spec& sp = lm->spec;
    const int d = sp.hidden, V = vocab_of(sp);
    const Prompt& p = a.p;
    const ScoreRows& R = *a.rows;
    const int GB = std::min(a.B, LM_MAX_ROWS), drop = p.cond_mode ? 1 : 0;
    const int64_t prow = R.body_rows_max, trow = R.packed_rows_max;
    const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(knob(K_LM_SCORE_ROWS), trow));
    LMBuffers b{};
    // as score_graph: b.att holds the packed target rows, b.hn their normalised form (a group's packed rows are fewer than its body rows)
    alloc_body(c.arena, b, prow, d, sp.intermediate);
    b.kc = c.arena.alloc<float>(prow * d);
    b.vc = c.arena.alloc<float>(prow * d);
    float* emix = c.arena.alloc<float>((size_t)GB * p.Nm * d);
    float* eenr = p.enroll ? c.arena.alloc<float>((size_t)GB * p.Ne * d) : nullptr;
    long long* tgt = c.arena.alloc<long long>(trow);
    float* row_kl = c.arena.alloc<float>(trow);
    int* row_ok = c.arena.alloc<int>(trow);
    float* logits = c.arena.alloc<float>((size_t)chunk * V);
    double* seq_sum = c.arena.alloc<double>(a.B);
    int* ints = c.arena.alloc<int>((size_t)SR_COUNT * GB);
    if (c.dry) return QA_OK;  // real-pass-only remainder: ints above is the function's last arena allocation
    const float conf = (float)(1.0 - a.eps), smooth = (float)(a.eps / (V - 1));
    for (const ScoreGroup& g : R.groups) {
        const int b0 = g.b0, gb = g.gb, n = g.n;
        const int *ne_r = ints + SR_NE * gb, *nm_r = ints + SR_NM * gb, *T_r = ints + SR_T * gb, *off_r = ints + SR_OFF * gb,
                  *lp_r = ints + SR_LP * gb, *L_r = ints + SR_L * gb, *zero_r = ints + SR_ZERO * gb;
        QA_TRY(write_score_ints(ints, R, g, c.stream));
        ScoreAssembleArgs as;
        as.x = b.x; as.n = n; as.B = gb; as.d = d;
        as.table = lm->codec_emb; as.V = V; as.goff = 3; as.soff = 3 + sp.global_size;
        as.gids = a.gids + (size_t)b0 * a.G; as.G = a.G; as.sids = a.sids + (size_t)b0 * a.T; as.T_max = a.T;
        as.tgt = tgt; as.T_r = T_r; as.off_r = off_r; as.drop = drop;
        if (p.cond_mode) {  // the condition embeddings are the prompt's frames as they are; none at all without a condition
            as.mix_sos = lm->mix_sos; as.mix_emb = p.cond ? p.cond + (size_t)b0 * p.Tc * d : nullptr; as.Nm = p.Tc; as.nm_r = nm_r;
        } else {
            // the adapters run over the padding frames too: a GEMM row depends on its own input row alone, and those outputs are never copied
            QA_TRY(adapt_prompt(lm, c, p, b0, gb, emix, eenr));
            speech_assemble(as, lm, p, emix, eenr, ne_r, nm_r);
        }
        QA_TRY(launch_lm_score_assemble(as, c.stream));
        QA_TRY(lm_body(lm, c, b, gb, n, 0, n, false, true, nullptr, zero_r, L_r));
        QA_TRY(launch_lm_score_gather(b.att, b.x, gb, n, d, a.G, g.Lt_max, lp_r, T_r, off_r, c.stream, drop));
        const int64_t rows = g.rows;
        QA_TRY(launch_rmsnorm(b.att, lm->ones, b.hn, rows, d, sp.rms_eps, c.stream));
        for (int64_t r0 = 0; r0 < rows; r0 += chunk) {
            const int64_t nr = std::min(chunk, rows - r0);
            QA_TRY(linear_op(c, b.hn + (size_t)r0 * d, nr, lm->head, logits));
            QA_TRY(launch_lm_row_loss(logits, V, V, nr, tgt + r0, conf, smooth, row_kl + r0, row_ok + r0, c.stream));
            if (tap)
                QA_HIP(hipMemcpyAsync(tap + ((size_t)g.row0 + r0) * V, logits, sizeof(float) * nr * V, hipMemcpyDeviceToDevice, c.stream));
        }
        QA_TRY(launch_lm_seq_reduce_rows(row_kl, row_ok, gb, a.G, T_r, off_r, seq_sum + b0, a.loss_seq + b0, a.correct_seq + b0, c.stream, drop));
    }
    return launch_lm_batch_reduce_rows(seq_sum, a.correct_seq, a.B, R.total_rows, a.loss, a.acc, c.stream);
}

// grow the workspace or the tap buffer of generate: earlier calls may still be running out of the old buffer, and captured steps point
// into it (they are keyed by its address and re-captured)
int grow_step_buffer(qa_lm* lm, Workspace& w, size_t bytes) {
    if (bytes <= w.cap) return QA_OK;
    QA_HIP(hipDeviceSynchronize());
    for (StepGraph& g : lm->graphs) g.reset();
    return w.ensure(bytes);
}

// the tap storage of a B x (G + 1, S) call: its own allocation, grown like the workspace
int ensure_taps(qa_lm* lm, int64_t B, int G, int S, void* stream) {
    QA_REQUIRE(!stream_capturing(static_cast<hipStream_t>(stream)), "qa_lm_generate: taps (a test hook) are not supported under a stream capture");
    const size_t n = (size_t)B * ((size_t)(G + 1) * lm->spec.global_size + (size_t)S * lm->spec.semantic_size);
    return grow_step_buffer(lm, lm->tap_buf, sizeof(float) * n);
}

// ---- sessions: qa_lm_forward over a caller-held qa_lm_cache (CustomLlamaModel.llm_forward, llm.py:150-227)

// The refusals of the length vectors of qa_lm_score_ragged / qa_lm_prompt_ragged as the library's messages (lm_score_rows.h)
int score_rows_refusal(const char* fn, ScoreRowsFault f, const ScoreRowsShape& s, int64_t row, int64_t value) {
    QA_REQUIRE(f != SCR_ENROLL_WITHOUT, "%s: n_enroll given (n_enroll[0] = %lld) without an enrollment (enroll_feats is NULL)", fn, (long long)value);
    QA_REQUIRE(f != SCR_ENROLL_RANGE, "%s: n_enroll[%lld] = %lld is outside 1 .. n_enroll_max = %lld", fn, (long long)row, (long long)value,
               (long long)s.ne_max);
    QA_REQUIRE(f != SCR_COND_WITHOUT, "%s: n_cond given (n_cond[0] = %lld) without a condition (cond_embeds is NULL or T_max = 0)", fn,
               (long long)value);
    QA_REQUIRE(f != SCR_MIX_RANGE || !s.cond_form, "%s: n_cond[%lld] = %lld is outside 1 .. T_max = %lld", fn, (long long)row, (long long)value,
               (long long)s.nm_max);
    QA_REQUIRE(f != SCR_MIX_RANGE, "%s: n_mix[%lld] = %lld is outside 1 .. n_mix_max = %lld", fn, (long long)row, (long long)value,
               (long long)s.nm_max);
    QA_REQUIRE(f != SCR_SEMANTIC_RANGE, "%s: n_semantic[%lld] = %lld is outside 0 .. semantic_length_max = %lld", fn, (long long)row,
               (long long)value, (long long)s.T_max);
    QA_REQUIRE(f != SCR_TOO_LONG, "%s: row %lld holds %lld positions (prompt + targets), which exceed max_position_embeddings %d", fn,
               (long long)row, (long long)value, s.max_pos);
    return QA_OK;
}

struct ForwardArgs {
    qa_lm_cache* cache;  // nullptr: use_cache = False, the keys live in the call's workspace
    const float* x;      // [B, n, d]
    int B, n;
    float *last_hidden, *all_hidden;
    // ragged (needs a cache): row b feeds its first n_rows[b] <= n positions (HOST, checked); nullptr: rectangular
    const int* n_rows = nullptr;
};

int forward_graph(qa_lm* lm, Ctx& c, const ForwardArgs& a) {
    const qa_lm_spec& sp = lm->spec;
    const int d = sp.hidden, B = a.B, n = a.n;
    const bool ragged = a.n_rows != nullptr;
    // ragged: the position of the LONGEST row that takes part - the step's position (the others sit off[b] <= 0 behind it), and with
    // pos0 + n a bound on every row's keys in the chunk path
    int pos0 = a.cache && !ragged ? a.cache->len[0] : 0;
    if (ragged)
        for (int i = 0; i < B; ++i)
            if (a.n_rows[i] > 0) pos0 = std::max(pos0, a.cache->len[(size_t)i]);
    const int64_t rows = (int64_t)B * n;
    const bool step = n == 1 && lm->fused_ok;
    LMBuffers b{};
    if (a.cache) {
        b.kc = a.cache->kc;
        b.vc = a.cache->vc;
        b.cap = a.cache->max_len;
        b.layer_stride = (size_t)a.cache->max_batch * a.cache->max_len * d;
    } else {  // every layer keeps its own keys here too: the n = 1 step appends to layer i's cache before layer i's attention reads it
        b.cap = (int)round_up(n, 16);
        b.kc = c.arena.alloc<float>((size_t)sp.n_layers * B * b.cap * d);
        b.vc = c.arena.alloc<float>((size_t)sp.n_layers * B * b.cap * d);
    }
    const size_t hs = (size_t)rows * d;  // one entry of all_hidden
    int idle = 0;                        // idle rows of a ragged n = 1 step
    if (!step) {
        alloc_body(c.arena, b, rows, d, sp.intermediate);
        if (c.dry) return QA_OK;  // real-pass-only remainder
        if (ragged) {
            // the rows' lengths travel as kernel arguments into the cache's device array; the padded input rows are replaced by zeros
            // without being read, and a zero row stays zero through the body (lm_rows_masked_copy_kernel): every padded output row is 0
            int* const row_pos0 = a.cache->rows;
            int* const row_n = a.cache->rows + B;
            std::vector<int> vals((size_t)2 * B);
            std::copy(a.cache->len.begin(), a.cache->len.begin() + B, vals.begin());
            std::copy(a.n_rows, a.n_rows + B, vals.begin() + B);
            QA_TRY(launch_row_ints(row_pos0, vals.data(), 2 * (long long)B, c.stream));
            QA_TRY(launch_lm_rows_masked_copy(b.x, a.x, B, n, d, row_n, c.stream));
            QA_TRY(lm_body(lm, c, b, B, n, pos0, b.cap, false, false, a.all_hidden, row_pos0, row_n));
        } else {
            QA_HIP(hipMemcpyAsync(b.x, a.x, sizeof(float) * hs, hipMemcpyDeviceToDevice, c.stream));
            QA_TRY(lm_body(lm, c, b, B, n, pos0, b.cap, false, false, a.all_hidden));
        }
        QA_TRY(launch_rmsnorm(b.x, lm->norm_w, a.last_hidden, rows, d, sp.rms_eps, c.stream));
    } else {
        // the fused step's launches on the caller's rows, at most LM_MAX_ROWS of them per pass (a row's arithmetic does not know its group)
        const int GB = std::min(B, LM_MAX_ROWS);
        if (a.cache) b.step = a.cache->step;
        else alloc_step(lm, c.arena, b.step, GB, b.cap);  // its state words are never read: the position is a launch argument
        if (c.dry) return QA_OK;  // real-pass-only remainder
        const size_t row_stride = (size_t)b.cap * d;
        if (ragged) {  // off[b] as ragged generate passes it; an idle row's is -(pos0 + 1): position -1, no key, no append (lm_decode.hip)
            std::vector<int> vals((size_t)2 * B);
            for (int i = 0; i < B; ++i) {
                const bool on = a.n_rows[i] > 0;
                vals[(size_t)i] = on ? a.cache->len[(size_t)i] - pos0 : -(pos0 + 1);
                vals[(size_t)B + i] = on ? 1 : 0;
                idle += !on;
            }
            QA_TRY(launch_row_ints(a.cache->rows, vals.data(), 2 * (long long)B, c.stream));
        }
        for (int b0 = 0; b0 < B; b0 += GB) {
            const int gb = std::min(GB, B - b0);
            LMBuffers g = b;
            g.kc = b.kc + b0 * row_stride;
            g.vc = b.vc + b0 * row_stride;
            if (!g.layer_stride) g.layer_stride = (size_t)B * b.cap * d;  // the whole call's layer, not the group's
            if (ragged) g.off = a.cache->rows + b0;
            StepIO io;
            io.x_in = a.x + (size_t)b0 * d;
            if (a.all_hidden) {
                io.hidden = a.all_hidden + (size_t)b0 * d;
                io.hidden_stride = hs;
            }
            QA_TRY(fused_layers(lm, g, gb, 0, 0, c.stream, pos0, io));
            QA_TRY(launch_rmsnorm(b.step.x, lm->norm_w, a.last_hidden + (size_t)b0 * d, gb, d, sp.rms_eps, c.stream));
        }
    }
    // a ragged step computed its idle rows too (on whatever their input rows held): their outputs become exact zeros, one launch each for
    // last_hidden and for the layer inputs of all_hidden
    const int* const step_n = step && ragged && idle ? a.cache->rows + B : nullptr;
    if (step_n) QA_TRY(launch_lm_rows_zero_pad(a.last_hidden, 0, 1, B, 1, d, step_n, c.stream));
    if (a.all_hidden) {  // llm.py:216-220: the last entry is the final norm's output
        if (step_n) QA_TRY(launch_lm_rows_zero_pad(a.all_hidden, (long long)hs, sp.n_layers, B, 1, d, step_n, c.stream));
        QA_HIP(hipMemcpyAsync(a.all_hidden + (size_t)sp.n_layers * hs, a.last_hidden, sizeof(float) * hs, hipMemcpyDeviceToDevice, c.stream));
    }
    return QA_OK;
}

// plan + run on the session workspace; growing it waits for the device (earlier session calls may still read the old buffer)
template <typename G>
int run_session(qa_lm* lm, hipStream_t s, G&& graph) {
    Ctx& c = lm->sess_ctx;
    c.gemm_fp32 = true;  // as generate and score: the fp32 chain everywhere
    c.att_fp32 = true;
    QA_TRY(plan(lm->device, s, c, lm->sess_ws, graph, [&](size_t) -> int {
        QA_HIP(hipDeviceSynchronize());
        return QA_OK;
    }));
    return graph();
}

}  // namespace

void cache_free(qa_lm_cache* c) {
    if (!c) return;
    if (c->lm) {
        auto& v = c->lm->caches;
        v.erase(std::remove(v.begin(), v.end(), c), v.end());
    }
    if (c->mem) (void)hipFree(c->mem);  // waits for the work that still reads it
    delete c;
}

extern "C" {

int qa_lm_cache_create(qa_lm* lm, int64_t max_batch, int64_t max_len, qa_lm_cache** out) {
    if (!lm || !out) {
        set_error("qa_lm_cache_create: null argument");
        return QA_ERR_INVALID;
    }
    *out = nullptr;
    QA_REQUIRE(max_batch >= 1 && max_batch <= (1 << 16), "qa_lm_cache_create: max_batch %lld outside [1, 65536]", (long long)max_batch);
    QA_REQUIRE(max_len >= 1 && max_len <= LM_MAX_POS, "qa_lm_cache_create: max_len %lld outside [1, %d] (max_position_embeddings)",
               (long long)max_len, LM_MAX_POS);
    QA_HIP(hipSetDevice(lm->device));
    const qa_lm_spec& sp = lm->spec;
    std::unique_ptr<qa_lm_cache> c(new qa_lm_cache());
    c->max_batch = (int)max_batch;
    c->max_len = (int)max_len;
    c->len.assign((size_t)max_batch, 0);
    const int GB = (int)std::min<int64_t>(max_batch, LM_MAX_ROWS);
    Arena layout;  // sizes the one allocation, then places the buffers in it
    auto place = [&] {
        const size_t plane = (size_t)sp.n_layers * max_batch * max_len * sp.hidden;
        c->kc = layout.alloc<float>(plane);
        c->vc = layout.alloc<float>(plane);
        c->spare = layout.alloc<float>((size_t)sp.n_layers * 2 * max_len * sp.hidden);
        alloc_step(lm, layout, c->step, GB, c->max_len);
        c->rows = layout.alloc<int>((size_t)2 * max_batch);  // behind everything else: the other buffers keep their offsets
    };
    layout.begin(nullptr, 0);
    place();
    const size_t bytes = layout.peak();
    if (hipMalloc(reinterpret_cast<void**>(&c->mem), bytes) != hipSuccess) {
        (void)hipGetLastError();
        c->mem = nullptr;
        set_error("qa_lm_cache_create: no device memory for a cache of %lld rows x %lld positions (%zu bytes)", (long long)max_batch,
                  (long long)max_len, bytes);
        return QA_ERR_HIP;
    }
    layout.begin(c->mem, bytes);
    place();
    c->lm = lm;
    lm->caches.push_back(c.get());
    *out = c.release();
    return QA_OK;
}

void qa_lm_cache_destroy(qa_lm_cache* cache) {
    if (!cache) return;
    if (cache->lm) (void)hipSetDevice(cache->lm->device);
    cache_free(cache);
}

int64_t qa_lm_cache_length(const qa_lm_cache* cache) { return cache ? cache->longest() : 0; }

int qa_lm_cache_lengths(const qa_lm_cache* cache, int64_t* out) {
    if (!cache || !out) {
        set_error("qa_lm_cache_lengths: null argument");
        return QA_ERR_INVALID;
    }
    for (int b = 0; b < cache->B; ++b) out[b] = cache->len[(size_t)b];
    return QA_OK;
}
int64_t qa_lm_cache_batch(const qa_lm_cache* cache) { return cache ? cache->B : 0; }

int qa_lm_cache_reset(qa_lm_cache* cache) {
    if (!cache) {
        set_error("qa_lm_cache_reset: null cache");
        return QA_ERR_INVALID;
    }
    std::fill(cache->len.begin(), cache->len.end(), 0);
    cache->B = 0;
    return QA_OK;
}

int qa_lm_cache_crop(qa_lm_cache* cache, int64_t len) {
    if (!cache) {
        set_error("qa_lm_cache_crop: null cache");
        return QA_ERR_INVALID;
    }
    QA_REQUIRE(len >= 0 && len <= cache->longest(), "qa_lm_cache_crop: length %lld outside [0, %d] (the cache's current length)", (long long)len,
               cache->longest());
    for (int b = 0; b < cache->B; ++b)  // the rows behind it are stale and invisible: every reader stops at its row's length
        cache->len[(size_t)b] = std::min(cache->len[(size_t)b], (int)len);
    return QA_OK;
}

int qa_lm_cache_crop_rows(qa_lm_cache* cache, const int64_t* lens) {
    if (!cache || !lens) {
        set_error("qa_lm_cache_crop_rows: null argument");
        return QA_ERR_INVALID;
    }
    const int64_t bad = check_crop_rows(lens, cache->len.data(), cache->B);
    QA_REQUIRE(bad < 0, "qa_lm_cache_crop_rows: lens[%lld] = %lld outside [0, %d] (the length of row %lld)", (long long)bad, (long long)lens[bad],
               cache->len[(size_t)bad], (long long)bad);
    for (int b = 0; b < cache->B; ++b) cache->len[(size_t)b] = (int)lens[b];
    return QA_OK;
}

int qa_lm_cache_select(qa_lm_cache* cache, const int64_t* idx, int64_t n, void* stream) {
    if (!cache || !idx) {
        set_error("qa_lm_cache_select: null argument");
        return QA_ERR_INVALID;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    QA_TRY(refuse_capture("qa_lm_cache_select", s, CACHE_IS_HOST_STATE));
    QA_REQUIRE(cache->B > 0, "qa_lm_cache_select: the cache has no batch yet (no qa_lm_forward call since create / reset)");
    QA_REQUIRE(n >= 1 && n <= cache->max_batch, "qa_lm_cache_select: %lld rows requested, the cache was created with max_batch %d", (long long)n,
               cache->max_batch);
    for (int64_t j = 0; j < n; ++j)
        QA_REQUIRE(idx[j] >= 0 && idx[j] < cache->B, "qa_lm_cache_select: idx[%lld] = %lld outside the cache's %d rows (IndexError in the reference)",
                   (long long)j, (long long)idx[j], cache->B);
    qa_lm* lm = cache->lm;
    QA_HIP(hipSetDevice(lm->device));
    if (cache->longest() > 0) {  // every move carries the length of the row it moves
        std::vector<KvMoves> waves;
        plan_cache_moves(idx, cache->len.data(), (int)n, std::max(cache->B, (int)n), &waves);
        for (const KvMoves& w : waves)
            QA_TRY(launch_kv_row_moves(cache->kc, cache->vc, cache->spare, lm->spec.n_layers, cache->max_batch, cache->max_len, lm->spec.hidden, w, s));
    }
    std::vector<int> len_new((size_t)cache->max_batch, 0);
    for (int64_t j = 0; j < n; ++j) len_new[(size_t)j] = cache->len[(size_t)idx[j]];
    cache->len.swap(len_new);
    cache->B = (int)n;
    return QA_OK;
}

// what qa_lm_forward and qa_lm_forward_ragged share once their arguments are checked: run, then advance the rows
static int lm_forward_run(qa_lm* lm, hipStream_t s, const ForwardArgs& a) {
    QA_TRY(run_session(lm, s, [&] { return forward_graph(lm, lm->sess_ctx, a); }));
    if (qa_lm_cache* cache = a.cache) {
        cache->B = a.B;
        for (int b = 0; b < a.B; ++b) cache->len[(size_t)b] += a.n_rows ? a.n_rows[b] : a.n;
    }
    return QA_OK;
}

static int lm_forward_cache_checks(const char* fn, qa_lm* lm, qa_lm_cache* cache, int64_t B) {
    QA_REQUIRE(cache->lm == lm, "%s: the cache belongs to another qa_lm handle", fn);
    QA_REQUIRE(B <= cache->max_batch, "%s: B = %lld exceeds the cache's max_batch %d", fn, (long long)B, cache->max_batch);
    QA_REQUIRE(cache->B == 0 || B == cache->B, "%s: B = %lld, but the cache holds %d sequences (the first call fixes the batch; "
               "qa_lm_cache_select changes it, qa_lm_cache_reset frees it)", fn, (long long)B, cache->B);
    return QA_OK;
}

int qa_lm_forward_ragged(qa_lm* lm, qa_lm_cache* cache, const float* inputs_embeds, int64_t B, int64_t n_max, const int64_t* n,
                         float* last_hidden, float* all_hidden, void* stream) {
    const char* fn = "qa_lm_forward_ragged";
    if (!lm || !inputs_embeds || !last_hidden) {
        set_error("%s: null argument", fn);
        return QA_ERR_INVALID;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    QA_TRY(refuse_capture(fn, s, CACHE_IS_HOST_STATE));
    QA_REQUIRE(cache, "%s: a qa_lm_cache is required - without one every row starts at position 0 and a causal pass over left-aligned rows "
               "is qa_lm_forward", fn);
    QA_REQUIRE(n, "%s: null n (HOST int64 [B], the rows' position counts)", fn);
    QA_REQUIRE(B >= 1 && n_max >= 1 && B <= (1 << 16) && n_max <= LM_MAX_POS, "%s: bad shape B = %lld, n_max = %lld", fn, (long long)B,
               (long long)n_max);
    QA_TRY(lm_forward_cache_checks(fn, lm, cache, B));
    // every check comes before the first launch and leaves the cache as it was
    std::vector<int> n_rows;
    int64_t row = 0;
    int active = 0;
    bool uniform = false;
    const SessionRowsFault f = check_session_rows(n, cache->len.data(), B, n_max, cache->max_len, &row, &n_rows, &active, &uniform);
    QA_REQUIRE(f != SR_COUNT_RANGE, "%s: n[%lld] = %lld is outside 0 .. n_max = %lld", fn, (long long)row, (long long)n[row], (long long)n_max);
    QA_REQUIRE(f != SR_OVER_CAPACITY, "%s: row %lld holds %d positions, + n[%lld] = %lld exceed the cache's max_len %d", fn, (long long)row,
               cache->len[(size_t)row], (long long)row, (long long)n[row], cache->max_len);
    if (active == 0) {  // nothing to do: no launch, no row advances (the batch is still fixed, as by any call)
        cache->B = (int)B;
        return QA_OK;
    }
    ForwardArgs a{cache, inputs_embeds, (int)B, (int)n_max, last_hidden, all_hidden};
    if (!uniform) a.n_rows = n_rows.data();  // a rectangular call IS qa_lm_forward: its launches, its bits
    return lm_forward_run(lm, s, a);
}

int qa_lm_forward(qa_lm* lm, qa_lm_cache* cache, const float* inputs_embeds, int64_t B, int64_t n, float* last_hidden, float* all_hidden,
                  void* stream) {
    if (!lm || !inputs_embeds || !last_hidden) {
        set_error("qa_lm_forward: null argument");
        return QA_ERR_INVALID;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    QA_TRY(refuse_capture("qa_lm_forward", s, CACHE_IS_HOST_STATE));
    QA_REQUIRE(B >= 1 && n >= 1 && B <= (1 << 16), "qa_lm_forward: bad shape B = %lld, n = %lld", (long long)B, (long long)n);
    std::vector<int> n_rows;
    if (cache) {
        QA_TRY(lm_forward_cache_checks("qa_lm_forward", lm, cache, B));
        QA_REQUIRE(cache->longest() + n <= cache->max_len, "qa_lm_forward: %d cached + %lld new positions exceed the cache's max_len %d%s",
                   cache->longest(), (long long)n, cache->max_len, cache->uniform() ? "" : " (the longest row)");
        if (!cache->uniform()) n_rows.assign((size_t)B, (int)n);  // rows of unequal lengths: the ragged call with n[b] = n
    } else {
        QA_REQUIRE(n <= LM_MAX_POS, "qa_lm_forward: %lld positions exceed max_position_embeddings %d", (long long)n, LM_MAX_POS);
    }
    ForwardArgs a{cache, inputs_embeds, (int)B, (int)n, last_hidden, all_hidden};
    if (!n_rows.empty()) a.n_rows = n_rows.data();
    return lm_forward_run(lm, s, a);
}

int qa_lm_embed(qa_lm* lm, const int64_t* ids, int64_t n, float* out, void* stream) {
    if (!lm || !ids || !out) {
        set_error("qa_lm_embed: null argument");
        return QA_ERR_INVALID;
    }
    QA_REQUIRE(n >= 0, "qa_lm_embed: bad count %lld", (long long)n);
    QA_HIP(hipSetDevice(lm->device));
    return launch_gather_rows(reinterpret_cast<const long long*>(ids), lm->codec_emb, out, n, vocab_of(lm->spec), lm->spec.hidden,
                              static_cast<hipStream_t>(stream));
}

int qa_lm_head(qa_lm* lm, const float* hidden, int64_t rows, int32_t lo, int32_t width, float* logits, void* stream) {
    if (!lm || !hidden || !logits) {
        set_error("qa_lm_head: null argument");
        return QA_ERR_INVALID;
    }
    const int V = vocab_of(lm->spec);
    QA_REQUIRE(rows >= 1 && rows <= (1 << 24), "qa_lm_head: bad row count %lld", (long long)rows);
    QA_REQUIRE(lo >= 0 && width >= 1 && (int64_t)lo + width <= V, "qa_lm_head: slice [%d, %d + %d) outside the vocabulary of %d", lo, lo, width, V);
    QA_HIP(hipSetDevice(lm->device));
    ConvW w = lm->head_raw;  // rows lo .. lo + width - 1 of output_head
    w.w += (size_t)lo * w.C_in;
    w.N = w.algo_n = width;
    Ctx c;
    c.stream = static_cast<hipStream_t>(stream);
    c.gemm_fp32 = true;
    return linear_op(c, hidden, rows, w, logits);
}

int qa_lm_create(qa_lm** out, const qa_lm_spec* spec, const qa_tensor* tensors, int64_t n_tensors, int device) {
    if (!out || !spec || !tensors) {
        set_error("qa_lm_create: null argument");
        return QA_ERR_INVALID;
    }
    *out = nullptr;
    QA_HIP(hipSetDevice(device));
    std::unique_ptr<qa_lm> lm(new qa_lm());
    lm->spec = *spec;
    lm->device = device;
    QA_TRY(build_lm(lm.get(), HostTable(tensors, n_tensors)));
    *out = lm.release();
    return QA_OK;
}

void qa_lm_destroy(qa_lm* lm) { destroy_handle(lm); }

// ---- generate, score and prompt: one front per family.  An entry point builds its Prompt, fills the family's
// argument struct and passes the name its messages carry; every check lives in the front, runs once, and comes before the first launch,
// before any handle state is written and before any output is touched.  The order of the checks is part of the contract: it decides
// which of two simultaneous faults a caller sees.

// a count of the API as the int the graphs take.  Saturating: a value beyond int lands on the same side of every bound it is held to
static int narrow(int64_t v) { return (int)std::min<int64_t>(std::max<int64_t>(v, INT_MIN), INT_MAX); }

// the shape the length vectors of a prompt / score call are planned against (lm_score_rows.h): the Prompt's widths are the tensors' strides
static ScoreRowsShape prompt_rows_shape(const Prompt& p, int64_t B) {
    ScoreRowsShape s;
    s.B = B; s.cond_form = p.cond_mode; s.has_enroll = p.enroll != nullptr; s.ne_max = p.Ne; s.nm_max = p.cond_mode ? p.Tc : p.Nm;
    s.targets = false; s.group_rows = LM_MAX_ROWS; s.max_pos = 2 * LM_MAX_POS + 3;  // no target rows: the frame counts bound it
    return s;
}
static ScoreRowsShape score_rows_shape(const ScoreArgs& a) {
    ScoreRowsShape s = prompt_rows_shape(a.p, a.B);
    s.targets = true; s.G = a.G; s.T_max = a.T; s.max_pos = LM_MAX_POS;
    return s;
}

// the HOST length vectors [B] of a score / prompt call, each NULL for "every row at full width": the rows' enrollment frames, mixture - or, in
// cond_mode, condition - frames and semantic ids
struct ScoreLens {
    const int64_t *enroll, *mix, *semantic;
    bool any() const { return enroll || mix || semantic; }
};
static const ScoreLens NO_LENS{};

// qa_lm_prompt / qa_lm_prompt_ragged.  No vector, or every row at full width: the rectangular launches
static int prompt_call(const char* fn, qa_lm* lm, const Prompt& p, int64_t B, const ScoreLens& n, float* out, void* stream) {
    if (!lm || !p.mix || !out) {
        set_error("%s: null argument", fn);
        return QA_ERR_INVALID;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    // without vectors: the adapters' scratch lives in the session workspace, which may have to grow
    QA_TRY(refuse_capture(fn, s, n.any() ? LENGTHS_ARE_HOST_DATA : CACHE_IS_HOST_STATE));
    QA_REQUIRE(p.task >= 0 && p.task < lm->spec.num_tasks, "%s: task %d out of range (KeyError in the reference)", fn, p.task);
    QA_REQUIRE(B >= 1 && p.Nm >= 1 && p.Nm <= LM_MAX_POS && B <= (1 << 16), "%s: bad shape", fn);
    QA_REQUIRE(!p.enroll || (p.Ne >= 1 && p.Ne <= LM_MAX_POS), "%s: enrollment given with no frames", fn);
    ScoreRows R;
    if (n.any()) {
        const ScoreRowsShape shape = prompt_rows_shape(p, B);
        int64_t row = 0, value = 0;
        QA_TRY(score_rows_refusal(fn, plan_score_rows(n.enroll, n.mix, nullptr, shape, &R, &row, &value), shape, row, value));
    }
    const int d = lm->spec.hidden;
    Ctx& c = lm->sess_ctx;
    if (R.uniform)
        return run_session(lm, s, [&]() -> int {
            float* emix = c.arena.alloc<float>((size_t)B * p.Nm * d);
            float* eenr = p.enroll ? c.arena.alloc<float>((size_t)B * p.Ne * d) : nullptr;
            return build_prompt(lm, c, p, 0, (int)B, emix, eenr, out, nullptr);
        });
    return run_session(lm, s, [&]() -> int {
        const int GB = (int)std::min<int64_t>(B, LM_MAX_ROWS);
        float* emix = c.arena.alloc<float>((size_t)GB * p.Nm * d);
        float* eenr = p.enroll ? c.arena.alloc<float>((size_t)GB * p.Ne * d) : nullptr;
        int* ints = c.arena.alloc<int>((size_t)SR_COUNT * GB);
        if (c.dry) return QA_OK;  // real-pass-only remainder
        for (const ScoreGroup& g : R.groups) {  // groups bound the adapters' scratch; a row's prompt does not know its group
            QA_TRY(write_score_ints(ints, R, g, c.stream));
            QA_TRY(adapt_prompt(lm, c, p, g.b0, g.gb, emix, eenr));
            ScoreAssembleArgs as;  // no table: the prompt alone
            as.x = out + (size_t)g.b0 * R.Lp_max * d; as.n = R.Lp_max; as.B = g.gb; as.d = d;
            speech_assemble(as, lm, p, emix, eenr, ints + SR_NE * g.gb, ints + SR_NM * g.gb);
            QA_TRY(launch_lm_score_assemble(as, c.stream));
        }
        return QA_OK;
    });
}

int qa_lm_prompt(qa_lm* lm, int32_t task, const float* enroll_feats, int64_t n_enroll, const float* mix_feats, int64_t n_mix, int64_t B,
                 float* out, void* stream) {
    return prompt_call("qa_lm_prompt", lm, speech_prompt(task, enroll_feats, narrow(n_enroll), mix_feats, narrow(n_mix)), B, NO_LENS, out, stream);
}

int qa_lm_prompt_ragged(qa_lm* lm, int32_t task, const float* enroll_feats, int64_t n_enroll_max, const int64_t* n_enroll, const float* mix_feats,
                        int64_t n_mix_max, const int64_t* n_mix, int64_t B, float* out, void* stream) {
    return prompt_call(n_enroll || n_mix ? "qa_lm_prompt_ragged" : "qa_lm_prompt", lm,
                       speech_prompt(task, enroll_feats, narrow(n_enroll_max), mix_feats, narrow(n_mix_max)), B,
                       ScoreLens{n_enroll, n_mix, nullptr}, out, stream);
}

// What the per-row vector of a ragged generate entry point is held to.  The two families differ in every member
struct GenRows {
    bool ragged;              // false: a rectangular entry point, nothing below is read
    const int64_t* n;         // HOST [B], 1 .. the prompt's Ne (speech) or Tc (condition)
    const char *vec, *bound;  // as the messages name them
    bool optional;            // a NULL vector is the rectangular call; false: refused
    bool full_is_rect;        // every row at the bound: the rectangular launches; false: still a ragged call
    bool host_only;           // refused under a stream capture
    // qa_lm_generate_rows with one of these given: HOST [B], mixture frames 1 .. Nm and semantic steps 0 .. S, each NULL
    // for "every row at full width"; `n` is then optional too, and every given vector at full width is the rectangular call
    const int64_t *mix = nullptr, *semantic = nullptr;
};
static const GenRows NO_ROWS{};
static GenRows enroll_rows(const int64_t* n_enroll) { return GenRows{true, n_enroll, "n_enroll", "n_enroll_max", false, false, false}; }
// the three vectors of qa_lm_generate_rows: none is qa_lm_generate, n_enroll alone qa_lm_generate_ragged - the same launches, the same bits
static GenRows speech_rows(const int64_t* n_enroll, const int64_t* n_mix, const int64_t* n_semantic) {
    if (!n_mix && !n_semantic) return n_enroll ? enroll_rows(n_enroll) : NO_ROWS;
    return GenRows{true, n_enroll, "n_enroll", "n_enroll_max", true, true, true, n_mix, n_semantic};
}
static GenRows cond_rows(const int64_t* n_cond) { return GenRows{true, n_cond, "n_cond", "T_max", true, true, true}; }

static GenArgs gen_args(const Prompt& p, int64_t B, int32_t global_length, int32_t semantic_length, const SampleCfg& sc, int64_t* global_ids,
                        int64_t* semantic_ids) {
    return GenArgs{p, (int)B, global_length, semantic_length, sc, global_ids, semantic_ids};
}
static SampleCfg greedy(float temperature, int32_t top_k, float top_p) { return SampleCfg{0, top_k, top_p, temperature, 0ull}; }
static SampleCfg sampled(float temperature, int32_t top_k, float top_p, uint64_t seed) {
    return SampleCfg{1, top_k, top_p, temperature, (unsigned long long)seed};
}

// the ten qa_lm_generate* entry points.  A ragged call lays its prompt out for the LONGEST possible row (a.p.Ne / a.p.Tc) and hands the
// checked vector on as a.p.ne_rows
static int generate_call(const char* fn, qa_lm* lm, GenArgs a, const GenRows& r, void* stream) {
    Prompt& p = a.p;
    if (!lm || (!p.cond_mode && !p.mix) || !a.gids || !a.sids) {
        set_error("%s: null argument", fn);
        return QA_ERR_INVALID;
    }
    const SampleCfg& sc = a.sc;
    QA_REQUIRE(p.cond_mode || (p.task >= 0 && p.task < lm->spec.num_tasks), "%s: task %d out of range (KeyError in the reference)", fn, p.task);
    QA_REQUIRE(a.B > 0 && (p.cond_mode || p.Nm > 0) && a.G >= 0 && a.S >= 0, "%s: bad shape", fn);
    QA_REQUIRE(!p.cond_mode || (p.Tc >= 0 && p.Tc < LM_MAX_POS && (p.cond != nullptr) == (p.Tc > 0) && a.G + a.S > 0),
               "%s: cond_embeds [B, T, hidden] with T > 0, or NULL with T = 0 (got T = %d); at least one step", fn, p.Tc);
    QA_REQUIRE(!p.enroll || p.Ne > 0, "%s: enrollment given with no frames", fn);
    QA_REQUIRE(sc.temperature > 0.f && sc.temperature <= 1.0f, "%s: temperature must be in (0, 1] (llm.py:278)", fn);
    QA_REQUIRE(sc.top_k >= 0 && sc.top_p > 0.f, "%s: bad top_k / top_p", fn);
    std::vector<int> rows_host, mix_host, stop_host;
    if (r.mix || r.semantic) {  // per-row mixture / semantic lengths: every check before the first launch, each naming its row and value
        QA_TRY(refuse_capture(fn, static_cast<hipStream_t>(stream), LENGTHS_ARE_HOST_DATA));
        QA_REQUIRE(!r.n || p.enroll, "%s: n_enroll given (n_enroll[0] = %lld) without an enrollment (enroll_feats is NULL)", fn, (long long)r.n[0]);
        const long long total = (long long)prompt_len(p) + a.G + 1 + a.S;  // the longest possible row, as section 23 checks it
        QA_REQUIRE(total <= LM_MAX_POS,
                   "%s: %lld positions (prompt %d with n_enroll_max %d and n_mix_max %d, + %d + 1 + semantic_length_max %d) exceed "
                   "max_position_embeddings %d", fn, total, prompt_len(p), p.Ne, p.Nm, a.G, a.S, LM_MAX_POS);
        bool full_e = true, full_m = true, full_s = true;
        if (r.n) {
            const int64_t bad = check_row_lengths(r.n, a.B, 1, p.Ne, &rows_host, &full_e);
            QA_REQUIRE(bad < 0, "%s: n_enroll[%d] = %lld is outside 1 .. n_enroll_max = %d", fn, (int)bad, (long long)r.n[bad], p.Ne);
        }
        if (r.mix) {
            const int64_t bad = check_row_lengths(r.mix, a.B, 1, p.Nm, &mix_host, &full_m);
            QA_REQUIRE(bad < 0, "%s: n_mix[%d] = %lld is outside 1 .. n_mix_max = %d", fn, (int)bad, (long long)r.mix[bad], p.Nm);
        }
        if (r.semantic) {
            const int64_t bad = check_row_lengths(r.semantic, a.B, 0, a.S, &stop_host, &full_s);
            QA_REQUIRE(bad < 0, "%s: n_semantic[%d] = %lld is outside 0 .. semantic_length_max = %d", fn, (int)bad, (long long)r.semantic[bad], a.S);
        }
        if (!full_e || !full_m) {  // one per-row assembly for both sources: a vector the caller left out stands at full width
            if (!r.n) rows_host.assign((size_t)a.B, p.Ne);
            if (!r.mix) mix_host.assign((size_t)a.B, p.Nm);
            p.ne_rows = p.enroll ? rows_host.data() : nullptr;
            p.nm_rows = mix_host.data();
        }
        if (!full_s) a.stop_rows = stop_host.data();
    } else if (r.ragged && (r.n || !r.optional)) {
        if (r.host_only) QA_TRY(refuse_capture(fn, static_cast<hipStream_t>(stream), LENGTHS_ARE_HOST_DATA));
        // the tensor the vector indexes must be there, and the longest possible row must fit: the two families' own texts
        char prompt_is[96];
        if (p.cond_mode) {
            QA_REQUIRE(p.cond && p.Tc > 0, "%s: n_cond given (n_cond[0] = %lld) without a condition (cond_embeds is NULL or T_max = 0)", fn,
                       (long long)r.n[0]);
            std::snprintf(prompt_is, sizeof(prompt_is), "prompt 1 + T_max %d", p.Tc);
        } else {
            QA_REQUIRE(p.enroll && r.n, "%s: per-row enrollment lengths need enroll_feats [B, n_enroll_max, feats_dim] and n_enroll [B]", fn);
            std::snprintf(prompt_is, sizeof(prompt_is), "prompt %d with n_enroll_max %d and n_mix %d", prompt_len(p), p.Ne, p.Nm);
        }
        const long long total = (long long)prompt_len(p) + a.G + 1 + a.S;
        QA_REQUIRE(total <= LM_MAX_POS, "%s: %lld positions (%s, + %d + 1 + %d) exceed max_position_embeddings %d", fn, total, prompt_is, a.G, a.S,
                   LM_MAX_POS);
        const int hi = p.cond_mode ? p.Tc : p.Ne;
        bool full = true;
        const int64_t bad = check_row_lengths(r.n, a.B, 1, hi, &rows_host, &full);
        QA_REQUIRE(bad < 0, "%s: %s[%d] = %lld is outside 1 .. %s = %d", fn, r.vec, (int)bad, (long long)r.n[bad], r.bound, hi);
        if (!full || !r.full_is_rect) p.ne_rows = rows_host.data();
    }
    QA_HIP(hipSetDevice(lm->device));
    if (sc.do_sample) QA_TRY(lm_sample_prepare());
    lm->tap_n[0] = lm->tap_n[1] = -1;
    if (lm->taps) QA_TRY(ensure_taps(lm, a.B, a.G, a.S, stream));
    Ctx& c = lm->ctx;
    c.gemm_fp32 = true;  // ConvParams::math_fp32
    c.att_fp32 = true;   // the prefill attention stays consistent with the fp32 decode kernels
    auto graph = [&] { return generate_graph(lm, c, a); };
    QA_TRY(plan(lm->device, static_cast<hipStream_t>(stream), c, lm->ws, graph, [&](size_t bytes) -> int {
        // growing the workspace synchronises the device and allocates: neither is possible inside a caller's stream capture
        QA_REQUIRE(!stream_capturing(c.stream),
                   "qa_lm_generate under a stream capture needs %zu bytes of workspace, the handle holds %zu: make one call of the same shape outside "
                   "the capture first (with QA_LM_CHAINS=1 for batches above 64: a capturing caller gets the single-chain launches)",
                   bytes, lm->ws.cap);
        return grow_step_buffer(lm, lm->ws, bytes);
    }));
    int st = graph();
    if (st != QA_OK) {  // an error between the fork and the join of a multi-chain call: the chains' streams may still be running out of the
        c.stream = static_cast<hipStream_t>(stream);  // workspace the next call re-uses - quiesce them (error path only)
        for (hipStream_t cs : lm->chain_streams) (void)hipStreamSynchronize(cs);
    } else if (lm->taps) {
        lm->tap_n[0] = (int64_t)a.B * (a.G + (p.cond_mode ? 0 : 1)) * lm->spec.global_size;
        lm->tap_n[1] = (int64_t)a.B * a.S * lm->spec.semantic_size;
    }
    return st;
}

int qa_lm_generate(qa_lm* lm, int32_t task, const float* enroll_feats, int64_t n_enroll, const float* mix_feats,
                   int64_t n_mix, int64_t B, int32_t global_length, int32_t semantic_length, float temperature,
                   int32_t top_k, float top_p, int64_t* global_ids, int64_t* semantic_ids, void* stream) {
    const Prompt p = speech_prompt(task, enroll_feats, n_enroll, mix_feats, n_mix);
    const SampleCfg sc = greedy(temperature, top_k, top_p);
    return generate_call("qa_lm_generate", lm, gen_args(p, B, global_length, semantic_length, sc, global_ids, semantic_ids), NO_ROWS, stream);
}

int qa_lm_generate_sampled(qa_lm* lm, int32_t task, const float* enroll_feats, int64_t n_enroll, const float* mix_feats,
                           int64_t n_mix, int64_t B, int32_t global_length, int32_t semantic_length, float temperature,
                           int32_t top_k, float top_p, uint64_t seed, int64_t* global_ids, int64_t* semantic_ids, void* stream) {
    const Prompt p = speech_prompt(task, enroll_feats, n_enroll, mix_feats, n_mix);
    const SampleCfg sc = sampled(temperature, top_k, top_p, seed);
    return generate_call("qa_lm_generate", lm, gen_args(p, B, global_length, semantic_length, sc, global_ids, semantic_ids), NO_ROWS, stream);
}

int qa_lm_generate_ragged(qa_lm* lm, int32_t task, const float* enroll_feats, int64_t n_enroll_max, const int64_t* n_enroll,
                          const float* mix_feats, int64_t n_mix, int64_t B, int32_t global_length, int32_t semantic_length, float temperature,
                          int32_t top_k, float top_p, int64_t* global_ids, int64_t* semantic_ids, void* stream) {
    const Prompt p = speech_prompt(task, enroll_feats, n_enroll_max, mix_feats, n_mix);
    const SampleCfg sc = greedy(temperature, top_k, top_p);
    return generate_call("qa_lm_generate_ragged", lm, gen_args(p, B, global_length, semantic_length, sc, global_ids, semantic_ids),
                         enroll_rows(n_enroll), stream);
}

int qa_lm_generate_ragged_sampled(qa_lm* lm, int32_t task, const float* enroll_feats, int64_t n_enroll_max, const int64_t* n_enroll,
                                  const float* mix_feats, int64_t n_mix, int64_t B, int32_t global_length, int32_t semantic_length,
                                  float temperature, int32_t top_k, float top_p, uint64_t seed, int64_t* global_ids, int64_t* semantic_ids,
                                  void* stream) {
    const Prompt p = speech_prompt(task, enroll_feats, n_enroll_max, mix_feats, n_mix);
    const SampleCfg sc = sampled(temperature, top_k, top_p, seed);
    return generate_call("qa_lm_generate_ragged", lm, gen_args(p, B, global_length, semantic_length, sc, global_ids, semantic_ids),
                         enroll_rows(n_enroll), stream);
}

int qa_lm_generate_rows(qa_lm* lm, int32_t task, const float* enroll_feats, int64_t n_enroll_max, const int64_t* n_enroll,
                        const float* mix_feats, int64_t n_mix_max, const int64_t* n_mix, int64_t B, int32_t global_length,
                        int32_t semantic_length_max, const int64_t* n_semantic, float temperature, int32_t top_k, float top_p,
                        int64_t* global_ids, int64_t* semantic_ids, void* stream) {
    const Prompt p = speech_prompt(task, enroll_feats, narrow(n_enroll_max), mix_feats, narrow(n_mix_max));
    const SampleCfg sc = greedy(temperature, top_k, top_p);
    return generate_call("qa_lm_generate_rows", lm, gen_args(p, B, global_length, semantic_length_max, sc, global_ids, semantic_ids),
                         speech_rows(n_enroll, n_mix, n_semantic), stream);
}

int qa_lm_generate_rows_sampled(qa_lm* lm, int32_t task, const float* enroll_feats, int64_t n_enroll_max, const int64_t* n_enroll,
                                const float* mix_feats, int64_t n_mix_max, const int64_t* n_mix, int64_t B, int32_t global_length,
                                int32_t semantic_length_max, const int64_t* n_semantic, float temperature, int32_t top_k, float top_p,
                                uint64_t seed, int64_t* global_ids, int64_t* semantic_ids, void* stream) {
    const Prompt p = speech_prompt(task, enroll_feats, narrow(n_enroll_max), mix_feats, narrow(n_mix_max));
    const SampleCfg sc = sampled(temperature, top_k, top_p, seed);
    return generate_call("qa_lm_generate_rows", lm, gen_args(p, B, global_length, semantic_length_max, sc, global_ids, semantic_ids),
                         speech_rows(n_enroll, n_mix, n_semantic), stream);
}

int qa_lm_generate_cond(qa_lm* lm, const float* cond_embeds, int64_t T, int64_t B, int32_t global_length, int32_t semantic_length,
                        float temperature, int32_t top_k, float top_p, int64_t* global_ids, int64_t* semantic_ids, void* stream) {
    const SampleCfg sc = greedy(temperature, top_k, top_p);
    return generate_call("qa_lm_generate_cond", lm, gen_args(cond_prompt(cond_embeds, T), B, global_length, semantic_length, sc, global_ids, semantic_ids),
                         NO_ROWS, stream);
}

int qa_lm_generate_cond_sampled(qa_lm* lm, const float* cond_embeds, int64_t T, int64_t B, int32_t global_length, int32_t semantic_length,
                                float temperature, int32_t top_k, float top_p, uint64_t seed, int64_t* global_ids, int64_t* semantic_ids,
                                void* stream) {
    const SampleCfg sc = sampled(temperature, top_k, top_p, seed);
    return generate_call("qa_lm_generate_cond", lm, gen_args(cond_prompt(cond_embeds, T), B, global_length, semantic_length, sc, global_ids, semantic_ids),
                         NO_ROWS, stream);
}

int qa_lm_generate_cond_ragged(qa_lm* lm, const float* cond_embeds, int64_t T_max, const int64_t* n_cond, int64_t B, int32_t global_length,
                               int32_t semantic_length, float temperature, int32_t top_k, float top_p, int64_t* global_ids,
                               int64_t* semantic_ids, void* stream) {
    const SampleCfg sc = greedy(temperature, top_k, top_p);
    return generate_call("qa_lm_generate_cond_ragged", lm,
                         gen_args(cond_prompt(cond_embeds, T_max), B, global_length, semantic_length, sc, global_ids, semantic_ids), cond_rows(n_cond),
                         stream);
}

int qa_lm_generate_cond_ragged_sampled(qa_lm* lm, const float* cond_embeds, int64_t T_max, const int64_t* n_cond, int64_t B,
                                       int32_t global_length, int32_t semantic_length, float temperature, int32_t top_k, float top_p,
                                       uint64_t seed, int64_t* global_ids, int64_t* semantic_ids, void* stream) {
    const SampleCfg sc = sampled(temperature, top_k, top_p, seed);
    return generate_call("qa_lm_generate_cond_ragged", lm,
                         gen_args(cond_prompt(cond_embeds, T_max), B, global_length, semantic_length, sc, global_ids, semantic_ids), cond_rows(n_cond),
                         stream);
}

static ScoreArgs score_args(const Prompt& p, int64_t B, const int64_t* global_ids, int32_t global_length, const int64_t* semantic_ids,
                            int32_t semantic_length, double label_smoothing, float* loss_per_seq, int64_t* correct_per_seq, float* loss, float* acc) {
    return ScoreArgs{p, narrow(B), global_length, semantic_length, reinterpret_cast<const long long*>(global_ids),
                     reinterpret_cast<const long long*>(semantic_ids), label_smoothing, loss_per_seq, reinterpret_cast<long long*>(correct_per_seq),
                     loss, acc};
}

// the four qa_lm_score* entry points.  With a vector a.p.Ne / a.p.Nm / a.p.Tc / a.T are the tensors' widths.  No vector is the rectangular
// call, with the rectangular checks (fn is then the rectangular sibling's name); vectors that hold every row at full width pass the
// per-row checks and then take the rectangular graph.
static int score_call(const char* fn, qa_lm* lm, ScoreArgs a, const ScoreLens& n, void* stream) {
    const Prompt& p = a.p;
    const bool ragged = n.any(), cm = p.cond_mode;
    if (!lm || (!cm && !p.mix) || !a.loss_seq || !a.correct_seq || !a.loss || !a.acc || (a.G > 0 && !a.gids) || (a.T > 0 && !a.sids)) {
        set_error("%s: null argument", fn);
        return QA_ERR_INVALID;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (ragged) QA_TRY(refuse_capture(fn, s, LENGTHS_ARE_HOST_DATA));
    QA_REQUIRE(cm || (p.task >= 0 && p.task < lm->spec.num_tasks), "%s: task %d out of range (KeyError in the reference)", fn, p.task);
    const bool cond_ok = p.Tc >= 0 && p.Tc < LM_MAX_POS && (p.cond != nullptr) == (p.Tc > 0);
    if (!ragged) {
        QA_REQUIRE(a.B > 0 && (cm || p.Nm > 0) && a.G >= 0 && a.T >= 0, "%s: bad shape", fn);
        QA_REQUIRE(!cm || cond_ok, "qa_lm_score_cond: cond_embeds [B, T, hidden] with T > 0, or NULL with T = 0 (got T = %lld)", (long long)p.Tc);
        QA_REQUIRE(!p.enroll || p.Ne > 0, "%s: enrollment given with no frames", fn);
    } else {  // the widths are bounded before the vectors are read against them
        const bool sizes_ok = a.B > 0 && a.B <= (1 << 24) && a.G >= 0 && a.G <= LM_MAX_POS && a.T >= 0 && a.T <= LM_MAX_POS;
        QA_REQUIRE(!cm || (sizes_ok && cond_ok),
                   "%s: cond_embeds [B, T_max, hidden] with T_max > 0, or NULL with T_max = 0 (got T_max = %lld); bad shape otherwise", fn,
                   (long long)p.Tc);
        QA_REQUIRE(cm || (sizes_ok && p.Nm > 0 && p.Nm <= LM_MAX_POS), "%s: bad shape", fn);
        QA_REQUIRE(!p.enroll || (p.Ne > 0 && p.Ne <= LM_MAX_POS), "%s: enrollment given with no frames", fn);
    }
    QA_REQUIRE(a.eps >= 0.0 && a.eps <= 1.0, "%s: label_smoothing %g outside [0, 1]", fn, a.eps);
    if (!ragged) QA_REQUIRE(p.Nm <= LM_MAX_POS && p.Ne <= LM_MAX_POS && a.B <= (1 << 24), "%s: bad shape", fn);
    ScoreRows R;
    if (ragged) {
        const ScoreRowsShape shape = score_rows_shape(a);
        int64_t row = 0, value = 0;
        QA_TRY(score_rows_refusal(fn, plan_score_rows(n.enroll, n.mix, n.semantic, shape, &R, &row, &value), shape, row, value));
        if (!R.uniform) a.rows = &R;  // else the rectangular call: its launches, its bits
    }
    QA_HIP(hipSetDevice(lm->device));
    const bool capturing = stream_capturing(s);
    const int Lt = a.G + a.T + 2 - (cm ? 1 : 0);
    // logits.forced: [B, Lt, V], or packed [sum Lt_b, V] after a call with per-row lengths
    const size_t tap_rows = a.rows ? (size_t)R.total_rows : (size_t)a.B * Lt;
    lm->score_tap_n = -1;
    float* tap = nullptr;
    if (lm->taps) {
        QA_REQUIRE(!capturing, "qa_lm_score: taps (a test hook) are not supported under a stream capture");
        const size_t bytes = sizeof(float) * tap_rows * vocab_of(lm->spec);
        if (bytes > lm->score_tap.cap) QA_HIP(hipDeviceSynchronize());  // earlier calls may still be writing the old buffer
        QA_TRY(lm->score_tap.ensure(bytes));
        tap = reinterpret_cast<float*>(lm->score_tap.ptr);
    }
    Ctx c;
    c.gemm_fp32 = true;  // ConvParams::math_fp32
    c.att_fp32 = true;   // the prefill attention stays consistent with the fp32 decode kernels
    auto graph = [&] { return score_graph(lm, c, a, tap); };
    QA_TRY(plan(lm->device, s, c, lm->score_ws, graph, [&](size_t bytes) -> int {
        QA_REQUIRE(!capturing, "qa_lm_score under a stream capture needs %zu bytes of workspace, the handle holds %zu: make one call of the "
                   "same shape outside the capture first", bytes, lm->score_ws.cap);
        QA_HIP(hipDeviceSynchronize());  // earlier calls may still be running out of the old workspace
        return QA_OK;
    }));
    QA_TRY(graph());
    if (tap) lm->score_tap_n = (int64_t)tap_rows * vocab_of(lm->spec);
    return QA_OK;
}

int qa_lm_score(qa_lm* lm, int32_t task, const float* enroll_feats, int64_t n_enroll, const float* mix_feats, int64_t n_mix, int64_t B,
                const int64_t* global_ids, int32_t global_length, const int64_t* semantic_ids, int32_t semantic_length, double label_smoothing,
                float* loss_per_seq, int64_t* correct_per_seq, float* loss, float* acc, void* stream) {
    const Prompt p = speech_prompt(task, enroll_feats, narrow(n_enroll), mix_feats, narrow(n_mix));
    const ScoreArgs a = score_args(p, B, global_ids, global_length, semantic_ids, semantic_length, label_smoothing, loss_per_seq, correct_per_seq, loss, acc);
    return score_call("qa_lm_score", lm, a, NO_LENS, stream);
}

int qa_lm_score_ragged(qa_lm* lm, int32_t task, const float* enroll_feats, int64_t n_enroll_max, const int64_t* n_enroll, const float* mix_feats,
                       int64_t n_mix_max, const int64_t* n_mix, int64_t B, const int64_t* global_ids, int32_t global_length,
                       const int64_t* semantic_ids, int32_t semantic_length_max, const int64_t* n_semantic, double label_smoothing,
                       float* loss_per_seq, int64_t* correct_per_seq, float* loss, float* acc, void* stream) {
    const Prompt p = speech_prompt(task, enroll_feats, narrow(n_enroll_max), mix_feats, narrow(n_mix_max));
    const ScoreArgs a = score_args(p, B, global_ids, global_length, semantic_ids, semantic_length_max, label_smoothing, loss_per_seq, correct_per_seq, loss, acc);
    const ScoreLens n{n_enroll, n_mix, n_semantic};
    return score_call(n.any() ? "qa_lm_score_ragged" : "qa_lm_score", lm, a, n, stream);
}

int qa_lm_score_cond(qa_lm* lm, const float* cond_embeds, int64_t T, int64_t B, const int64_t* global_ids, int32_t global_length,
                     const int64_t* semantic_ids, int32_t semantic_length, double label_smoothing, float* loss_per_seq,
                     int64_t* correct_per_seq, float* loss, float* acc, void* stream) {
    const Prompt p = cond_prompt(cond_embeds, narrow(T));
    const ScoreArgs a = score_args(p, B, global_ids, global_length, semantic_ids, semantic_length, label_smoothing, loss_per_seq, correct_per_seq, loss, acc);
    return score_call("qa_lm_score_cond", lm, a, NO_LENS, stream);
}

int qa_lm_score_cond_ragged(qa_lm* lm, const float* cond_embeds, int64_t T_max, const int64_t* n_cond, int64_t B, const int64_t* global_ids,
                            int32_t global_length, const int64_t* semantic_ids, int32_t semantic_length_max, const int64_t* n_semantic,
                            double label_smoothing, float* loss_per_seq, int64_t* correct_per_seq, float* loss, float* acc, void* stream) {
    const Prompt p = cond_prompt(cond_embeds, narrow(T_max));
    const ScoreArgs a = score_args(p, B, global_ids, global_length, semantic_ids, semantic_length_max, label_smoothing, loss_per_seq, correct_per_seq, loss, acc);
    const ScoreLens n{nullptr, n_cond, n_semantic};
    return score_call(n.any() ? "qa_lm_score_cond_ragged" : "qa_lm_score_cond", lm, a, n, stream);
}

int qa_lm_enable_taps(qa_lm* lm, int on) {
    if (!lm) {
        set_error("qa_lm_enable_taps: null handle");
        return QA_ERR_INVALID;
    }
    lm->taps = on != 0;
    return QA_OK;
}

int64_t qa_lm_tap(qa_lm* lm, const char* name, float* dst, int64_t cap, void* stream) {
    if (!lm || !name) {
        set_error("qa_lm_tap: null argument");
        return QA_ERR_INVALID;
    }
    const std::string nm(name);
    const int which = nm == "logits.global" ? 0 : nm == "logits.semantic" ? 1 : nm == "logits.forced" ? 2 : -1;
    if (which < 0 || (which < 2 ? lm->tap_n[which] : lm->score_tap_n) < 0) {
        set_error("qa_lm_tap: no intermediate named '%s' in the last call (names: logits.global, logits.semantic of generate, "
                  "logits.forced of score; taps must be on)", name);
        return QA_ERR_MISSING;
    }
    const int64_t n = which < 2 ? lm->tap_n[which] : lm->score_tap_n;
    if (dst) {
        if (cap < n) {
            set_error("qa_lm_tap: '%s' has %lld elements, capacity %lld", name, (long long)n, (long long)cap);
            return QA_ERR_INVALID;
        }
        const float* src = reinterpret_cast<const float*>(which == 2 ? lm->score_tap.ptr : lm->tap_buf.ptr) + (which == 1 ? lm->tap_n[0] : 0);
        QA_HIP(hipMemcpyAsync(dst, src, sizeof(float) * n, hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream)));
    }
    return n;
}

int qa_sample_logits(const float* logits, int64_t B, int64_t width, int64_t ld, int32_t top_k, float top_p, float temperature,
                     int32_t do_sample, uint64_t seed, int64_t* out_index, void* stream) {
    if (!logits || !out_index) {
        set_error("qa_sample_logits: null argument");
        return QA_ERR_INVALID;
    }
    QA_REQUIRE(B > 0 && width > 0 && ld >= width, "qa_sample_logits: bad shape");
    QA_REQUIRE(temperature > 0.f && temperature <= 1.0f, "qa_sample_logits: temperature must be in (0, 1] (llm.py:278)");
    QA_REQUIRE(top_k >= 0 && top_p > 0.f, "qa_sample_logits: bad top_k / top_p");
    hipStream_t s = static_cast<hipStream_t>(stream);
    QA_TRY(lm_sample_prepare());
    char* scratch = nullptr;
    QA_HIP(hipMalloc(reinterpret_cast<void**>(&scratch), 256 + sizeof(long long) * (size_t)B));
    int* state = reinterpret_cast<int*>(scratch);
    long long* tok = reinterpret_cast<long long*>(scratch + 256);
    int st = launch_lm_phase_init(tok, 0, (int)B, state, 0, 1, (unsigned long long)seed, 0, s);
    if (st == QA_OK)
        st = launch_lm_sample(logits, ld, (int)width, (int)B, 0, top_k, top_p, temperature, do_sample, tok, (long long*)out_index, 1, 1,
                              state, s);
    const hipError_t e = hipStreamSynchronize(s);
    (void)hipFree(scratch);
    if (st != QA_OK) return st;
    QA_HIP(e);
    return QA_OK;
}

}  // extern "C"
