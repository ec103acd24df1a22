// hcodec.cpp - H-Codec 1.0 encode / decode graphs on top of the HIP kernels (host orchestration, C-ABI handle).
//
// Mirrors, stage for stage, Codec.encode / Codec.decode of the reference
// (QuarkAudio-HCodec/HCodec-1.0/vq/codec.py:166-187) with every activation kept time-major / channel-last
// ([B, frames, C] rows) so that all convolutions and linears are one implicit-GEMM kernel (conv_gemm.hip).
// Weights arrive in the reference's state_dict layout; weight-norm is folded and filters re-laid out here, once.
#include <atomic>
#include <memory>

#include "host_util.h"
#include "stream_step.h"

namespace qa {

namespace {

struct TransformerLayerW {
    const float *ln1, *ln2;
    ConvW ih;            // [4d][d] rows in (unit, gate) order, bias = b_ih + b_hh
    const float* w_hh;   // [4d][d] rows in (unit, gate) order
    ConvW qkv, o, w1, w3, w2;
};

struct TransformerW {
    std::vector<TransformerLayerW> layers;
    int d = 0, heads = 0, inter = 0;
    const float* rope = nullptr;      // [MAX_POS][hd/2][2]
    const float* rope_inv = nullptr;  // [hd/2]: the table's inverse frequencies, for the positions of a ring stream beyond it
};

struct ResBlockW {  // SEANetResnetBlock
    ConvW k3, pw, sc;
};
struct DecResW {  // ResnetBlock (GroupNorm + swish)
    const float *n1w, *n1b, *n2w, *n2b;
    ConvW c1, c2;
};
struct ConvNeXtW {
    const float *dw, *dwb, *lnw, *lnb, *gamma;
    ConvW pw1, pw2;
};

struct MimiLayerW {  // StreamingTransformerLayer (mimi/transformer.py:436-594)
    const float *n1w, *n1b, *n2w, *n2b, *ls1, *ls2;
    ConvW in_proj, out_proj, lin1, lin2;
};
struct MimiW {
    std::vector<MimiLayerW> layers;
    int d = 0, heads = 0, ff = 0;
    int causal = 0, context = 0;  // StreamingMultiheadAttention causal / context (mimi/transformer.py:403-413); context is ignored unless causal
    const float* rope = nullptr;  // interleaved-pair table [MAX_POS][hd/2][2]
};
// _MHAState of every layer (mimi/transformer.py:284-293): RingKVCache [B, cap, d] x 2 and the offset
struct MimiStream {
    std::vector<float*> kc, vc;
    int B = 0, cap = 0, offset = 0;
    // streaming_forever(): past the static RoPE table the step reads a rolling window of it (positions rope_base .. rope_base + len)
    // rebuilt on the host whenever the stream leaves it, so the offset is unbounded like the reference's (module/rope.py computes
    // the angles from the running offset)
    DeviceFloats rope_win;  // allocated by the first step that leaves the static table
    int rope_base = 0, rope_len = 0;
};

constexpr int MAX_POS = TR_ROPE_POSITIONS;

// the per-layer views of `mem`: `lead` floats per layer in front of the two [B, cap, d] caches (the streaming state's h and c)
void transformer_kv_views(float* mem, size_t layers, size_t lead, size_t per, std::vector<float*>* kc, std::vector<float*>* vc) {
    kc->resize(layers);
    vc->resize(layers);
    for (size_t l = 0; l < layers; ++l) {
        (*kc)[l] = mem + l * (lead + 2 * per) + lead;
        (*vc)[l] = (*kc)[l] + per;
    }
}

// The streaming state of one codec Transformer: per layer the LSTM's (h, c) [B, d] and the roped K / V rows
// [B, cap, d], one allocation of the handle's own (not arena memory).  B > 0: streaming.  qa_transformer and the streaming H-Codec encoder
// (section 43) both carry one.
struct TrStream {
    int B = 0, cap = 0, d = 0;
    // ring mode: the caches are rings of cap rows under the window `window` and the stream has no end; a step takes
    // at most max_chunk frames.  window = 0: linear, a step ends at or before row cap
    int window = 0, max_chunk = 0;
    bool ring() const { return window > 0; }
    // The rows' offsets (section 47), in the unit its owner counts in: `rate` Transformer frames each (code frames of the H-Codec stream at
    // 2, frames of a Transformer stream at 1).  off[b]: units of row b since begin / its reset.  A row at 0 takes a first step next: its
    // (h, c) zeroed, earlier K / V rows invisible (no step reads a row at or behind its own key count), the codec's reflect fill.  Begin
    // and every reset are therefore host writes of zeros and nothing else
    std::vector<int> off;
    int rate = 1;
    int offset() const { return off.empty() ? 0 : *std::max_element(off.begin(), off.end()); }
    int cap_units() const { return cap / rate; }
    StepPlan plan;                  // scratch of the step front, kept for its vectors' storage: a refused step overwrites it too, and
                                    // nothing reads it outside a running step (what a refusal leaves as it was is `off` and the device state)
    const int* dev[4] = {nullptr, nullptr, nullptr, nullptr};  // the device copies of plan.cnt / first / pos0 / nq in `ints`
    bool rows = false;              // the running step has per-row lengths (set around its graph only): dev[] and plan.max_keys hold
    DeviceFloats mem;
    DeviceInts ints{4};             // a step with per-row lengths (section 45): the plan's four vectors, written once per step
    std::vector<float*> kc, vc, hs, cs;
    void release() {  // not streaming any more (the caller has set the device)
        mem.release();
        off.clear();
        B = cap = window = max_chunk = 0;
    }
    // a fresh state for B sequences of up to `capacity` Transformer frames counted `unit_rate` to the unit, in place of the one it held;
    // never cleared: no kernel reads a K / V row at or behind the key count of its step, and (h, c) are zeroed by the first step
    int begin(const TransformerW& w, int64_t batch, int64_t capacity, int unit_rate) {
        release();
        const size_t L = w.layers.size(), st = (size_t)batch * w.d, per = (size_t)batch * capacity * w.d;
        QA_TRY(mem.allocate(L * (2 * st + 2 * per)));
        transformer_kv_views(mem.ptr, L, 2 * st, per, &kc, &vc);
        hs.resize(L);
        cs.resize(L);
        for (size_t l = 0; l < L; ++l) {
            hs[l] = kc[l] - 2 * st;
            cs[l] = kc[l] - st;
        }
        B = (int)batch;
        cap = (int)capacity;
        d = w.d;
        rate = unit_rate;
        off.assign((size_t)batch, 0);
        return QA_OK;
    }
    // the same as a ring for chunks of up to `chunk` frames under the window `left_context`.  The rings ARE cleared, once: the short
    // kernel never loads a row its item has not written, but attention_kernel's ring mode (long chunks) loads every row and multiplies the
    // hidden ones by a zero probability, which needs them finite
    int begin_ring(const TransformerW& w, int64_t batch, int left_context, int64_t chunk, int unit_rate) {
        const int64_t rows = ring::capacity(left_context, chunk);
        QA_TRY(begin(w, batch, rows, unit_rate));
        QA_HIP(hipMemset(mem.ptr, 0, sizeof(float) * w.layers.size() * 2 * ((size_t)batch * w.d + (size_t)batch * rows * w.d)));
        QA_HIP(hipDeviceSynchronize());  // the steps run on the caller's stream, which need not wait for the null stream
        window = left_context;
        max_chunk = (int)chunk;
        return QA_OK;
    }
    StreamView view(int first_min) const { return StreamView{off.data(), B, rate, cap_units(), first_min, window, max_chunk}; }
    // a rectangular step of rows at offset 0: (h, c) = 0 of every layer, in stream order like the step itself.  A step with per-row
    // lengths zeroes the rows that start in its own kernel (plan.first)
    int zero_lstm(hipStream_t s) {
        for (size_t l = 0; l < hs.size(); ++l) QA_HIP(hipMemsetAsync(hs[l], 0, sizeof(float) * 2 * (size_t)B * d, s));
        return QA_OK;
    }
};

// One stateful convolution of the streaming SEANet encoder: its carried context, the last `ctx` rows [B, ctx, C]
// of its own input buffer.  Two buffers, alternated by the host: a step reads st[cur] and writes st[cur ^ 1] (stream_conv.hip)
struct StreamConv {
    int ctx = 0, C = 0;
    float* st[2] = {nullptr, nullptr};
};
// The streaming state of a causal H-Codec 1.0 encoder, between qa_hcodec_stream_begin and _end: what the convolutions add to the state
// of its Transformer, which owns the rows' offsets (in code frames) and the running step's row arrays
struct CodecStream {
    int cur = 0;                     // which of the two state buffers of every convolution holds the current state
    int first_min = 0;               // the fewest code frames a first chunk may have (stream_geometry)
    DeviceFloats conv_mem;
    std::vector<StreamConv> convs;   // conv0, then (k3, down) per stage, then the out conv
    TrStream tr;
};

}  // namespace

}  // namespace qa

using namespace qa;

struct qa_hcodec : Handle {
    qa_hcodec_spec spec{};
    // encoder
    const float *conv0_w = nullptr, *conv0_b = nullptr;
    std::vector<ResBlockW> res;
    std::vector<ConvW> down;
    TransformerW enc_tr;
    ConvW enc_out;
    // semantic encoder
    ConvW sem_in;
    struct SemBlock {
        ConvW u1[2], u2[2], conv;
        int stride;
    };
    std::vector<SemBlock> sem_blocks;
    ConvW sem_out;
    // rvq
    const float *cb_a = nullptr, *cb_s = nullptr, *e2_a = nullptr, *e2_s = nullptr;
    DeviceFloats e2_dev;
    // decoder
    ConvW up;
    const float *up_dw = nullptr, *up_dwb = nullptr;
    DecResW dres[4];
    TransformerW dec_tr;
    const float *gn_w = nullptr, *gn_b = nullptr, *norm_w = nullptr, *norm_b = nullptr, *fnorm_w = nullptr,
                *fnorm_b = nullptr;
    std::vector<ConvNeXtW> cnx;
    ConvW head, basis;
    const float* window = nullptr;
    int spec_ld = 0;
    // H-Codec 2.0 encoder
    ConvW stft_basis, enc_embed, enc_out20, dec_embed20;
    const float *enc_norm_w = nullptr, *enc_norm_b = nullptr, *enc_fnorm_w = nullptr, *enc_fnorm_b = nullptr;
    std::vector<ConvNeXtW> enc_cnx;
    int stft_ld = 0;
    // H-Codec 1.5
    MimiW agg_sem, agg_ac, bottleneck;
    const float *qemb_sem = nullptr, *qemb_ac = nullptr;
    int* host_sync = nullptr;  // pinned host scalar for the data-dependent group / frame counts
    hipStream_t side = nullptr;  // second stream: the two aggregator stacks are independent and run concurrently
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    // semantic decoder (semantic_module.py:205-300): attached by qa_hcodec_load_semantic_decoder, read by forward only
    struct SemDecBlock {
        int stride = 1, c_out = 0;
        ConvW conv;                // stride 1: Conv1d k3 "same"
        std::vector<ConvW> phase;  // stride s > 1: the ConvTranspose1d as s stride-1 filters, phase phi writes rows q s + phi
        std::vector<int> pad_left;
        ConvW u1[2], u2[2];        // ResidualUnit: x + conv2(ELU(conv1(ELU(x))))
    };
    struct SemDec {
        qa_semantic_decoder_spec spec{};
        WeightStore store;
        ConvW conv1, conv2;
        std::vector<SemDecBlock> blocks;
    };
    std::unique_ptr<SemDec> sdec;
    // frame geometry, set once by build(): frames per CODE frame wherever the graphs or the entry points need a rate
    struct Geom {
        int samples = 0;        // waveform samples: 2 * prod(ratios); H-Codec 2.0: hop * frame_stride
        int feat = 0;           // SSL feature frames: prod(sem_strides)
        int dec = 0;            // decoder (ISTFT) frames: 2; H-Codec 2.0: frame_stride
        std::vector<int> enc;   // SEANet: at the input of stage i; enc[n_ratios] = 2, the rate of its transformer.  H-Codec 2.0: enc[0] =
                                // 2 * frame_stride, the STFT's input blocks of (n_fft - hop) / 2 samples; enc[1] = frame_stride, its frames
        std::vector<int> sem;   // semantic encoder: at the input of block i; sem[n_sem_strides] = 1, the rate of its output
    } geom;
    // ragged calls (qa_hcodec_encode_ragged / _decode_ragged and their _adaptive_ twins): the clips' code-frame counts, written on the call's
    // stream
    DeviceInts lens;
    // the chunked encoder of a causal H-Codec 1.0 handle (qa_hcodec_stream_*); null: not streaming
    std::unique_ptr<CodecStream> strm;
    ~qa_hcodec() {
        if (host_sync) (void)hipHostFree(host_sync);
        if (side) (void)hipStreamDestroy(side);
        if (ev_fork) (void)hipEventDestroy(ev_fork);
        if (ev_join) (void)hipEventDestroy(ev_join);
    }
};

// One StreamingTransformer with its optional streaming state (mimi/transformer.py:605-698)
struct qa_mimi : Handle {
    qa_mimi_spec spec{};
    MimiW w;
    MimiStream st;       // st.B > 0: inside `with model.streaming(B)`
    DeviceFloats ring;   // backing store of the ring caches
};

// One codec Transformer (encoder_modules/transformer.py:396-489) on its own: offline forward, the reference's cache mode and a
// streaming state
struct qa_transformer : Handle {
    qa_transformer_spec spec{};
    TransformerW w;
    TrStream st;  // streaming state (st.B > 0: between qa_transformer_stream_begin and _end), its offsets in frames
};
// past_key_values of Transformer.forward(x, past_key_values, use_cache=True): per layer the roped K and V rows [B, cap, d] in fp32
struct qa_transformer_cache {
    const qa_transformer* owner = nullptr;
    int device = 0, B = 0, cap = 0, len = 0;
    DeviceFloats mem;
    std::vector<float*> kc, vc;
};

namespace qa {
namespace {

// ---------------------------------------------------------------- weight folding (host)

// apply_rope (mimi/module/rope.py:38-56): freqs = exp(i * (-ln(P) * 2 / D)), angle = freqs * t, all in fp32; (cos, sin) pairs of
// positions pos0 .. pos0 + n - 1 as [n][hd/2][2]
void mimi_rope_table(int hd, int pos0, int n, std::vector<float>* cs) {
    const int half = hd / 2;
    cs->resize((size_t)n * half * 2);
    const float coef = (float)(-std::log(10000.0) * 2.0 / hd);
    for (int i = 0; i < half; ++i) {
        const float fr = std::exp((float)i * coef);
        for (int t = 0; t < n; ++t) {
            const float ang = fr * (float)(pos0 + t);
            (*cs)[((size_t)t * half + i) * 2] = (float)std::cos((double)ang);
            (*cs)[((size_t)t * half + i) * 2 + 1] = (float)std::sin((double)ang);
        }
    }
}

void build_transformer(Loader& b, TransformerW* tw, const std::string& p, int d, int n_layers, int heads, int inter = 0) {
    if (inter <= 0) inter = 4 * d;
    tw->d = d;
    tw->heads = heads;
    tw->inter = inter;
    tw->layers.resize(n_layers);
    for (int l = 0; l < n_layers; ++l) {
        TransformerLayerW& L = tw->layers[l];
        const std::string lp = p + ".layers." + std::to_string(l);
        const std::string ap = lp + ".self_attn";
        b.vec(&L.ln1, lp + ".input_layernorm.weight", d);
        b.vec(&L.ln2, lp + ".post_attention_layernorm.weight", d);
        const float* wih = b.need(ap + ".rnn.weight_ih_l0", (int64_t)4 * d * d);
        const float* whh = b.need(ap + ".rnn.weight_hh_l0", (int64_t)4 * d * d);
        const float* bih = b.need(ap + ".rnn.bias_ih_l0", 4 * d);
        const float* bhh = b.need(ap + ".rnn.bias_hh_l0", 4 * d);
        // rows of an LSTM matrix / bias go from PyTorch's gate-major order (i,f,g,o blocks of d) to (unit, gate)
        std::vector<float> wi((size_t)4 * d * d, 0.f), wh((size_t)4 * d * d, 0.f), bb((size_t)4 * d, 0.f);
        if (wih && whh && bih && bhh) {
            for (int u = 0; u < d; ++u)
                for (int g = 0; g < 4; ++g) {
                    const size_t dst = (size_t)u * 4 + g, src = (size_t)g * d + u;
                    std::memcpy(&wi[dst * d], &wih[src * d], sizeof(float) * d);
                    std::memcpy(&wh[dst * d], &whh[src * d], sizeof(float) * d);
                    bb[dst] = bih[src] + bhh[src];
                }
        }
        L.ih.N = 4 * d; L.ih.C_in = d; L.ih.ksize = 1;
        b.raw(&L.ih.w, wi);
        b.raw(&L.ih.b, bb);
        b.raw(&L.w_hh, wh);
        // fused QKV
        std::vector<float> wq((size_t)3 * d * d, 0.f), bq((size_t)3 * d, 0.f);
        const char* names[3] = {".q_proj", ".k_proj", ".v_proj"};
        for (int i = 0; i < 3; ++i) {
            const float* w = b.need(ap + names[i] + ".weight", (int64_t)d * d);
            const float* bi = b.need(ap + names[i] + ".bias", d);
            if (w) std::memcpy(&wq[(size_t)i * d * d], w, sizeof(float) * d * d);
            if (bi) std::memcpy(&bq[(size_t)i * d], bi, sizeof(float) * d);
        }
        L.qkv.N = 3 * d; L.qkv.C_in = d; L.qkv.ksize = 1;
        b.raw(&L.qkv.w, wq);
        b.raw(&L.qkv.b, bq);
        b.linear(&L.o, ap + ".o_proj.weight", "", d, d);
        b.linear(&L.w1, lp + ".mlp.w1.weight", "", inter, d);
        b.linear(&L.w3, lp + ".mlp.w3.weight", "", inter, d);
        b.linear(&L.w2, lp + ".mlp.w2.weight", "", d, inter);
    }
    // RoPE table, RotaryEmbedding of transformer.py:8-74 evaluated in fp32 like the reference
    std::vector<float> cs, inv;
    transformer_rope_table(d / heads, &cs, &inv);
    b.raw(&tw->rope, cs);
    b.raw(&tw->rope_inv, inv);
}

void build_mimi(Loader& b, MimiW* mw, const std::string& p, int d, int n_layers, int heads, int ff, int causal, int context) {
    mw->d = d;
    mw->heads = heads;
    mw->ff = ff;
    mw->causal = causal;
    mw->context = context;
    mw->layers.resize(n_layers);
    for (int l = 0; l < n_layers; ++l) {
        MimiLayerW& L = mw->layers[l];
        const std::string lp = p + ".layers." + std::to_string(l);
        b.norm(&L.n1w, &L.n1b, lp + ".norm1", d);
        b.norm(&L.n2w, &L.n2b, lp + ".norm2", d);
        b.vec(&L.ls1, lp + ".layer_scale_1.scale", d);
        b.vec(&L.ls2, lp + ".layer_scale_2.scale", d);
        b.linear(&L.in_proj, lp + ".self_attn.in_proj_weight", "", 3 * d, d);
        b.linear(&L.out_proj, lp + ".self_attn.out_proj.weight", "", d, d);
        b.linear(&L.lin1, lp + ".linear1.weight", "", ff, d);
        b.linear(&L.lin2, lp + ".linear2.weight", "", d, ff);
    }
    std::vector<float> cs;
    mimi_rope_table(d / heads, 0, MAX_POS, &cs);
    b.raw(&mw->rope, cs);
}

// ---------------------------------------------------------------- graph helpers

// The caller's SSL features [B, sem_in, n] as element strides: any layout
struct FeatView {
    const float* p;
    int64_t sb, sc, st;
    int n;
};

// y [t.B, T_out, w.N] = conv(x [t.B, t.T, w.C_in], w) with o's geometry, prologue and epilogue.  In a ragged call the clips' lengths at
// t's rate go to every filter with a temporal footprint; a 1x1 is row-wise and takes none.
int conv_at(Ctx& c, const float* x, const TimeAxis& t, const ConvW& w, float* y, int T_out, ConvOpt o) {
    if (w.ksize > 1) o.rl = t.rl;
    return conv_op(c, x, w.C_in, t.B, t.T, w, y, w.N, T_out, o);
}
// "same" zero-padded stride-1 conv (vq/conv.py:33-56, semantic_module.py:28-31); o: prologue and epilogue
int conv_same(Ctx& c, const float* x, const TimeAxis& t, const ConvW& w, float* y, ConvOpt o = ConvOpt()) {
    const int pad = (w.ksize - 1) / 2;
    o.stride = 1;
    o.pad_left = t.causal ? w.ksize - 1 : pad;
    o.pad_right = t.causal ? 0 : pad;
    return conv_at(c, x, t, w, y, t.T, o);
}
// ELU(conv(ELU(x))): the first convolution of a residual unit
inline ConvOpt elu_conv_elu() {
    ConvOpt o = epi(ACT_ELU);
    o.prologue = ACT_ELU;
    return o;
}

// SConv1d geometry (encoder_modules/conv.py:195-211): returns T_out and the paddings
struct SGeom {
    int T_out, left, right;
};
SGeom sconv_geom(int L, int k, int stride, bool causal) {
    int64_t t = 0;
    int32_t left = 0, right = 0;
    (void)qa_sconv_geometry(L, k, stride, &t, &left, &right);
    if (causal) {  // conv.py:203-206: pad (padding_total, extra_padding)
        right -= (k - stride) / 2;
        left = k - stride;
    }
    return {(int)t, left, right};
}
// qa_hcodec::Geom::enc of a SEANet ladder: frames per code frame at the input of stage i, 2 at its transformer
std::vector<int> seanet_rates(const qa_hcodec_spec& sp) {
    std::vector<int> enc(sp.n_ratios + 1, 2);
    for (int i = sp.n_ratios - 1; i >= 0; --i) enc[i] = enc[i + 1] * sp.ratios[i];
    return enc;
}
// zero padding of vq/conv.py's Conv1d (stride 1, :44-47): (k - 1, 0) if causal else (k / 2, k / 2)
inline int zpad_left(int k, bool causal) { return causal ? k - 1 : k / 2; }
inline int zpad_right(int k, bool causal) { return causal ? 0 : k / 2; }

// The K / V caches and carried state of a chunk of t.T frames at positions pos0 .. pos0 + t.T - 1: the cached forward and the streaming step of
// a codec Transformer.  Per layer the chunk's roped K and V rows are written to cache rows pos0 .. pos0 + t.T - 1 before
// its queries attend over rows 0 .. pos0 + t.T - 1.
struct TrChunk {
    float* const* kc = nullptr;  // [layer] -> [B, cap, d]
    float* const* vc = nullptr;
    int cap = 0, pos0 = 0;
    // streaming: the carried LSTM state of every layer [B, d] (read at step 0, left at the chunk's last step); null: the LSTM starts from
    // zero, as the reference's does on every call (transformer.py:133)
    float* const* hs = nullptr;
    float* const* cs = nullptr;
    // a streaming step with per-row lengths: device int [B] each, all or none - item b sits at row_pos0[b] with
    // row_nq[b] of the t.T frames, and starts from a zero LSTM state where row_zero[b] != 0; max_keys = max_b(row_pos0[b] + row_nq[b]).
    // pos0 is then unused.  Null: every item at pos0 with all t.T frames, today's launches
    const int *row_pos0 = nullptr, *row_nq = nullptr, *row_zero = nullptr;
    int max_keys = 0;
    // window > 0: the caches are rings of cap rows under this sliding window, which replaces the left_context of the call
    int window = 0;
};

// Whether a carried causal chunk of N frames x B rows takes the split-key kernel (stream_attn.hip): QA_TR_SHORT_ATTN 0 never, 1 up to 256
// query rows per head, 2 every chunk of <= ATTN_SHORT_MAX_Q frames.  One rule for transformer_op and for the checks in front of a step
inline bool tr_short_chunk(int B, int N) {
    const long long mode = knob(K_TR_SHORT_ATTN);
    return N <= ATTN_SHORT_MAX_Q && (mode == 2 || (mode == 1 && (int64_t)B * N <= 256));
}

// In place on x [t.B, t.T, d].  Ragged calls (non-causal): only the attention looks past a clip's end - the LSTM runs forward, everything
// else is row-wise - so the lengths become one [B, N] key-padding mask, built once per call, for the KMASK form.
// left_context > 0 (causal graphs only): the sliding window of Transformer(use_sliding_window=True) - query i sees key j iff i - j < left_context.
// t.causal = 0: every query sees every key, the later ones of its own chunk included (mask None).
// ch: null for the offline form (RoPE in place, attention over the packed qkv); else the chunk over ch's caches, which takes no taps.
int transformer_op(Ctx& c, const TransformerW& tw, float* x, const TimeAxis& t, const std::string& tap_prefix, int left_context = 0,
                   const TrChunk* ch = nullptr) {
    const int d = tw.d, H = tw.heads, hd = d / H, B = t.B, N = t.T;
    const int64_t rows = t.rows();
    const bool carried = ch && ch->hs;
    QA_REQUIRE(N <= MAX_POS, "transformer: sequence of %d frames exceeds %d", N, MAX_POS);
    const size_t mark = c.arena.mark();
    float* hn = c.arena.alloc<float>(rows * d);
    const int wide = std::max(4 * d, tw.inter);
    float* big = c.arena.alloc<float>(rows * wide);   // xw (4d) / gate buffer
    float* big2 = c.arena.alloc<float>(rows * wide);  // swiglu product
    float* hl = c.arena.alloc<float>(rows * d);
    float* qkv = c.arena.alloc<float>(rows * 3 * d);
    float* att = c.arena.alloc<float>(rows * d);
    float* cst = carried ? nullptr : c.arena.alloc<float>((size_t)B * d);
    // a stream step of a few frames over a long history: the split-key kernel (stream_attn.hip), 1.0 - 1.5 x the step through
    // attention_kernel up to 256 query rows per head and 0.92 - 1.01 x at 512 (B = 32 x 16 frames: its partial records outweigh the
    // parallelism it adds; profiles/transformer_stream_bench.jsonl).  QA_TR_SHORT_ATTN: 0 never, 2 every chunk of <= 16 frames
    const bool short_chunk = carried && t.causal && tr_short_chunk(B, N);
    float* part = short_chunk ? c.arena.alloc<float>(attn_short_part_floats(B, H, hd, N, ch->cap)) : nullptr;
    AttnArgs at = attn_packed_qkv(qkv, att, B, N, H, hd);
    at.causal = t.causal ? 1 : 0;
    const bool ring = ch && ch->window > 0;
    if (ring) left_context = ch->window;
    at.context = t.causal ? left_context : 0;
    const bool ragged = ch && ch->row_nq;
    if (ch) {  // keys and values: rows 0 .. pos0 + N - 1 of the layer's caches
        at.ldkv = d; at.kv_batch_stride = (long long)ch->cap * d;
        at.n_keys = ragged ? ch->max_keys : ch->pos0 + N;
    }
    if (ring) {  // the long chunk of a ring, rows moving together: attention_kernel's ring mode over all cap rows, keys appended first
        QA_REQUIRE(carried && t.causal && ch->cap > ring::min_rows(ch->window, N), "transformer: a ring of %d rows under a window of %d "
                   "holds chunks of fewer than %d frames", ch->cap, ch->window, ch->cap - ch->window + 1);
        at.n_keys = ch->cap; at.q_pos0 = ch->pos0; at.ring_end = ch->pos0 + N;
    }
    if (ragged) {
        QA_REQUIRE(carried && t.causal && ch->row_pos0 && ch->row_zero && (ring || (ch->max_keys >= 1 && ch->max_keys <= ch->cap)),
                   "transformer: per-row lengths exist for the streaming step of a causal Transformer");
        // the chunk form of attention_kernel with per-item counts is its fp32 form without a window (section 34); attention_op keeps it
        // (the entry point has refused this on the host, in front of its first launch, with the words a caller needs)
        QA_REQUIRE(short_chunk || at.context == 0, "transformer: per-row lengths under a sliding window need the short-chunk attention");
        at.row_pos0 = ch->row_pos0; at.row_nq = ch->row_nq;
    }
    if (t.rl.n) {
        QA_REQUIRE(!t.causal && !ch, "transformer: per-clip lengths exist for the non-causal offline graph only");
        unsigned char* kvalid = c.arena.alloc<unsigned char>(rows);
        QA_RUN(c, launch_len_mask(kvalid, B, N, t.rl, c.stream));
        at.kvalid = kvalid;
    }
    // the names are built in a tapping call only: a single-frame stream step is launch-bound, and this is its per-layer host work
    const bool taps = c.capture && !ch;
    std::string lp;
    auto tap = [&](const char* name, const float* p) {
        if (taps) c.tap(lp + name, p, rows * d);
    };
    for (size_t l = 0; l < tw.layers.size(); ++l) {
        const TransformerLayerW& L = tw.layers[l];
        if (taps) lp = tap_prefix + ".layers." + std::to_string(l);
        QA_TRY(rmsnorm_op(c, x, L.ln1, hn, rows, d, 1e-6f));
        QA_TRY(linear_op(c, hn, rows, L.ih, big));
        if (carried) QA_RUN(c, launch_lstm_carry(big, L.w_hh, hl, ch->hs[l], ch->cs[l], B, N, d, c.stream, ch->row_nq, ch->row_zero));
        else QA_RUN(c, launch_lstm(big, L.w_hh, hl, cst, B, N, d, c.stream));
        tap(".self_attn.rnn", hl);
        QA_TRY(linear_op(c, hl, rows, L.qkv, qkv));
        if (ch) {
            QA_RUN(c, launch_rope_append(qkv, tw.rope, ch->kc[l], ch->vc[l], B, N, H, hd, ch->pos0, ch->cap, c.stream, ch->row_pos0, ch->row_nq,
                                         ring ? tw.rope_inv : nullptr));
            at.k = ch->kc[l]; at.v = ch->vc[l];
        } else {
            QA_TRY(rope_op(c, qkv, tw.rope, B, N, H, hd, 3 * d, 0));
        }
        if (short_chunk) {
            QA_RUN(c, launch_attention_short(qkv, 3 * d, at.k, at.v, att, part, B, N, H, hd, ch->pos0, ch->cap, at.context, c.stream, ch->row_pos0,
                                             ch->row_nq, ch->max_keys, ring));
        } else {
            QA_TRY(attention_op(c, at));
        }
        tap(".att", att);
        QA_TRY(linear_op(c, att, rows, L.o, x, epi(ACT_NONE, x)));
        tap(".x_attn", x);
        QA_TRY(rmsnorm_op(c, x, L.ln2, hn, rows, d, 1e-6f));
        QA_TRY(linear_op(c, hn, rows, L.w1, big));
        QA_TRY(linear_op(c, hn, rows, L.w3, big2, epi(ACT_NONE, nullptr, nullptr, big)));
        QA_TRY(linear_op(c, big2, rows, L.w2, x, epi(ACT_NONE, x)));
        tap(".x_mlp", x);
    }
    c.arena.release(mark);
    return QA_OK;
}

// the running step of a streaming state: the K / V rows and the carried LSTM state of `st`, at its rows' common position or, in a step
// with per-row lengths (st.rows), with the uploaded row arrays
TrChunk stream_chunk(const TrStream& st) {
    TrChunk ch;
    ch.kc = st.kc.data(); ch.vc = st.vc.data();
    ch.cap = st.cap; ch.pos0 = st.rate * st.offset();
    ch.hs = st.hs.data(); ch.cs = st.cs.data();
    ch.window = st.window;
    if (st.rows) {
        ch.pos0 = 0;
        ch.row_zero = st.dev[1]; ch.row_pos0 = st.dev[2]; ch.row_nq = st.dev[3];
        ch.max_keys = st.plan.max_keys;
    }
    return ch;
}

// StreamingTransformer.forward, non-causal / non-streaming (mimi/transformer.py:377-425,553-594,674-698), in place on x
struct MimiTemps {
    float *hn, *qkv, *att, *u;
};
MimiTemps mimi_temps(Ctx& c, const MimiW& mw, int64_t rows) {
    MimiTemps t;
    t.hn = c.arena.alloc<float>(rows * mw.d);
    t.qkv = c.arena.alloc<float>(rows * 3 * mw.d);
    t.att = c.arena.alloc<float>(rows * mw.d);
    t.u = c.arena.alloc<float>(rows * mw.ff);
    return t;
}
// st != nullptr: streaming step of N frames at st->offset (layer index li selects the ring caches); the caller advances the offset.
// kvalid: the key-padding mask [B, N] of a per-clip call (non-causal, non-streaming), or null.
int mimi_layer(Ctx& c, const MimiW& mw, const MimiLayerW& L, float* x, const MimiTemps& t, int B, int N, const unsigned char* kvalid,
               MimiStream* st = nullptr, size_t li = 0) {
    const int d = mw.d, H = mw.heads, hd = d / H;
    const int64_t rows = (int64_t)B * N;
    const int pos0 = st ? st->offset : 0;
    const bool win = st && st->rope_len > 0;  // RoPE angles from the rolling window (positions beyond the static table)
    const float* rope = win ? st->rope_win.ptr : mw.rope;
    const int rope_pos0 = win ? pos0 - st->rope_base : pos0;
    QA_TRY(layernorm_op(c, x, L.n1w, L.n1b, t.hn, rows, d, 1e-5f));
    // fused QKV projection with the interleaved-pair RoPE of q and k applied in the GEMM epilogue (one launch less per layer)
    ConvOpt qo;
    qo.rope = rope; qo.rope_n = 2 * d; qo.rope_hd = hd; qo.rope_T = N; qo.rope_pos0 = rope_pos0;
    QA_TRY(linear_op(c, t.hn, rows, L.in_proj, t.qkv, qo));
    AttnArgs at = attn_packed_qkv(t.qkv, t.att, B, N, H, hd);
    if (st) {
        // RingKVCache.complete(): the chunk's keys / values are written first, then every query attends over the ring
        QA_RUN(c, launch_ring_append(t.qkv + d, t.qkv + 2 * d, 3 * d, st->kc[li], st->vc[li], B, N, d, st->cap, pos0, c.stream));
        at.k = st->kc[li]; at.v = st->vc[li]; at.ldkv = d;
        at.n_keys = st->cap;
        at.kv_batch_stride = (long long)st->cap * d;
        at.causal = 1;
        at.context = mw.context; at.q_pos0 = pos0; at.ring_end = pos0 + N;
    } else {
        at.causal = mw.causal;
        at.context = mw.causal ? mw.context : 0;
        at.kvalid = kvalid;
    }
    QA_TRY(attention_op(c, at));
    QA_TRY(linear_op(c, t.att, rows, L.out_proj, x, epi(ACT_NONE, x, L.ls1)));
    QA_TRY(layernorm_op(c, x, L.n2w, L.n2b, t.hn, rows, d, 1e-5f));
    QA_TRY(linear_op(c, t.hn, rows, L.lin1, t.u, epi(ACT_GELU)));
    return linear_op(c, t.u, rows, L.lin2, x, epi(ACT_NONE, x, L.ls2));
}
int mimi_op(Ctx& c, const MimiW& mw, float* x, int B, int N, const unsigned char* kvalid) {
    QA_REQUIRE(N <= MAX_POS, "mimi transformer: sequence of %d tokens exceeds %d", N, MAX_POS);
    QA_REQUIRE(!kvalid || !mw.causal, "mimi transformer: a key-padding mask needs a non-causal stack");
    const size_t mark = c.arena.mark();
    const MimiTemps t = mimi_temps(c, mw, (int64_t)B * N);
    for (const MimiLayerW& L : mw.layers) QA_TRY(mimi_layer(c, mw, L, x, t, B, N, kvalid));
    c.arena.release(mark);
    return QA_OK;
}
// The read-out of a QueryTokenAggregator stack over x [B, T + G, d]: the output rows at the G query positions per clip -> out [B, G, d],
// zeros for padded groups (start / len / nseg as in agg_build / agg_gather).
struct AggReadout {
    const int *start, *len, *nseg;
    int T, G;
    float* out;
};
// Last layer of an aggregator stack, read-out included (QA_AGG_LAST_ROWS): the keys and values need every row, so LayerNorm 1 and in_proj run
// as in mimi_layer; everything after them is row-wise and runs on the B G query rows alone, gathered into xq / qq [B, G, d].  Every op gives
// a row the bits it gives it in the full layer (conv_gemm does not depend on M or the tile, attention not on n_q), so out equals
// agg_gather(mimi_layer(x)).  Non-causal stacks only: a compact query has lost its position.  kvalid [B, T + G] or null, as in mimi_layer:
// the mask is per key, so the G compact queries take it as the T + G queries of the full layer do.
int mimi_readout_layer(Ctx& c, const MimiW& mw, const MimiLayerW& L, const float* x, const MimiTemps& t, float* xq, float* qq, int B,
                       const AggReadout& ro, const unsigned char* kvalid) {
    const int d = mw.d, H = mw.heads, hd = d / H, N = ro.T + ro.G;
    const int64_t rows = (int64_t)B * N, qrows = (int64_t)B * ro.G;
    QA_TRY(layernorm_op(c, x, L.n1w, L.n1b, t.hn, rows, d, 1e-5f));
    ConvOpt qo;
    qo.rope = mw.rope; qo.rope_n = 2 * d; qo.rope_hd = hd; qo.rope_T = N; qo.rope_pos0 = 0;
    QA_TRY(linear_op(c, t.hn, rows, L.in_proj, t.qkv, qo));
    QA_RUN(c, launch_agg_query_rows(x, t.qkv, ro.start, ro.len, ro.nseg, xq, qq, B, ro.T, ro.G, d, c.stream));
    AttnArgs at = attn_packed_qkv(t.qkv, t.att, B, N, H, hd);  // keys and values of all N rows ...
    at.q = qq; at.ldq = d; at.n_q = ro.G;                      // ... under the G compact queries
    at.kvalid = kvalid;
    QA_TRY(attention_op(c, at));
    QA_TRY(linear_op(c, t.att, qrows, L.out_proj, xq, epi(ACT_NONE, xq, L.ls1)));
    QA_TRY(layernorm_op(c, xq, L.n2w, L.n2b, t.hn, qrows, d, 1e-5f));
    QA_TRY(linear_op(c, t.hn, qrows, L.lin1, t.u, epi(ACT_GELU)));
    QA_TRY(linear_op(c, t.u, qrows, L.lin2, ro.out, epi(ACT_NONE, xq, L.ls2)));
    QA_RUN(c, launch_agg_zero_padded(ro.nseg, ro.out, B, ro.G, d, c.stream));
    return QA_OK;
}
std::atomic<long long> g_split_regions;  // regions that ran as two half-batch lanes so far (qa_debug_batch_split_regions)

// One side of mimi_pair_op: a stack over x [B, N, d].  kvalid [B, N] or null: its key-padding mask, written on the caller's stream before
// the fork.  ro: its read-out, or null.
struct MimiStack {
    const MimiW& w;
    float* x;
    int B;
    const unsigned char* kvalid;
    const AggReadout* ro;
};
// The workspace bytes [lo, hi) that one lane of a two-stream region was handed.  The arena is a bump allocator: what one lane releases the
// other would receive while the first lane's kernels still run, so every region gives its lanes ranges of their own and checks them at the
// join, in the planning and in the real pass.
struct LaneSpan {
    size_t lo, hi;
};
int lanes_disjoint(const LaneSpan& a, const LaneSpan& b) {
    QA_REQUIRE(a.lo <= a.hi && b.lo <= b.hi && (a.hi <= b.lo || b.hi <= a.lo),
               "two-stream region: the lanes' workspace ranges [%zu, %zu) and [%zu, %zu) overlap", a.lo, a.hi, b.lo, b.hi);
    return QA_OK;
}
// two independent stacks of equal depth over N rows per clip, layer-interleaved on two streams (a on the caller's stream, b on `side`); with
// read-outs (both or neither) the last layer of each stack is mimi_readout_layer, which leaves a.x / b.x at the input of that layer.  The
// stacks may be the two aggregators over one batch, or ONE stack over the two halves of a batch (QA_BATCH_SPLIT): every op of a layer is
// per clip, so a half batch is a row range of the same buffer and gets the bits the whole batch gives it.  The caller forks and joins.
// gemm_lanes = 2: the two sides launch the same GEMM shapes side by side (GemmLanes, common.h) - the halves of a batch; the aggregators
// measured no faster with it and keep 1.
int mimi_pair_op(Ctx& c, hipStream_t side, const MimiStack& a, const MimiStack& b, int N, int gemm_lanes = 1) {
    const MimiW &wa = a.w, &wb = b.w;
    QA_REQUIRE(N <= MAX_POS && wa.layers.size() == wb.layers.size(), "mimi pair: mismatched stacks");
    QA_REQUIRE((!a.kvalid && !b.kvalid) || (!wa.causal && !wb.causal), "mimi pair: a key-padding mask needs non-causal stacks");
    QA_REQUIRE(!a.ro == !b.ro && (!a.ro || (!wa.causal && !wb.causal && wa.d == wb.d && !wa.layers.empty())), "mimi pair: bad read-out");
    const size_t mark = c.arena.mark();
    float* cq[4] = {nullptr, nullptr, nullptr, nullptr};  // xq, qq of either stack
    const MimiTemps ta = mimi_temps(c, wa, (int64_t)a.B * N);
    if (a.ro)
        for (int i = 0; i < 2; ++i) cq[i] = c.arena.alloc<float>((size_t)a.B * a.ro->G * wa.d);
    const size_t mid = c.arena.mark();
    const MimiTemps tb = mimi_temps(c, wb, (int64_t)b.B * N);
    if (b.ro)
        for (int i = 2; i < 4; ++i) cq[i] = c.arena.alloc<float>((size_t)b.B * b.ro->G * wb.d);
    QA_TRY(lanes_disjoint(LaneSpan{mark, mid}, LaneSpan{mid, c.arena.mark()}));
    if (!c.dry) {  // real pass only, more than launches: c.stream alternates between the two streams
        hipStream_t main = c.stream;
        const GemmLanes lanes(gemm_lanes);
        for (size_t l = 0; l < wa.layers.size(); ++l) {
            const bool last = a.ro && l + 1 == wa.layers.size();
            c.stream = main;
            int st = last ? mimi_readout_layer(c, wa, wa.layers[l], a.x, ta, cq[0], cq[1], a.B, *a.ro, a.kvalid)
                          : mimi_layer(c, wa, wa.layers[l], a.x, ta, a.B, N, a.kvalid);
            c.stream = side;
            if (st == QA_OK)
                st = last ? mimi_readout_layer(c, wb, wb.layers[l], b.x, tb, cq[2], cq[3], b.B, *b.ro, b.kvalid)
                          : mimi_layer(c, wb, wb.layers[l], b.x, tb, b.B, N, b.kvalid);
            c.stream = main;
            QA_TRY(st);
        }
    }
    c.arena.release(mark);
    return QA_OK;
}

int groupnorm_op(Ctx& c, const float* x, const float* w, const float* b, float* y, const TimeAxis& t, int C, int G, int swish) {
    const size_t mark = c.arena.mark();
    double* scratch = c.arena.alloc<double>(groupnorm_scratch_bytes(t.B, t.T, G) / sizeof(double));
    QA_RUN(c, launch_groupnorm(x, w, b, y, scratch, t.B, t.T, C, G, 1e-6f, swish, c.stream, t.rl));
    c.arena.release(mark);
    return QA_OK;
}

int dec_resblock_op(Ctx& c, const DecResW& w, float* x, const TimeAxis& t, int C, int G) {
    const size_t mark = c.arena.mark();
    float* t1 = c.arena.alloc<float>((size_t)t.rows() * C);
    float* t2 = c.arena.alloc<float>((size_t)t.rows() * C);
    QA_TRY(groupnorm_op(c, x, w.n1w, w.n1b, t1, t, C, G, 1));
    QA_TRY(conv_same(c, t1, t, w.c1, t2));
    QA_TRY(groupnorm_op(c, t2, w.n2w, w.n2b, t1, t, C, G, 1));
    QA_TRY(conv_same(c, t1, t, w.c2, x, epi(ACT_NONE, x)));
    c.arena.release(mark);
    return QA_OK;
}

// ---------------------------------------------------------------- encode / decode graphs

int convnext_op(Ctx& c, const ConvNeXtW& w, float* x, float* t1, float* u, const TimeAxis& t, int d) {
    QA_TRY(dwconv_op(c, x, w.dw, w.dwb, w.lnw, w.lnb, t1, t.B, t.T, d, 7, 1e-6f, zpad_left(7, t.causal), t.rl));
    QA_TRY(linear_op(c, t1, t.rows(), w.pw1, u, epi(ACT_GELU)));
    return linear_op(c, u, t.rows(), w.pw2, x, epi(ACT_NONE, x, w.gamma));
}

// H-Codec 2.0 CodecEncoder.forward (HCodec-2.0/vq/codec_encoder.py:62-79): wav [B, T] -> emb [B, T / (hop*stride), code_dim]
int encoder20(qa_hcodec* h, Ctx& c, const float* wav, const TimeAxis& tw, float** emb_out, int* n50_out, int* nf_out) {
    const qa_hcodec_spec& sp = h->spec;
    const int B = tw.B, T = tw.T;
    const int blk = (sp.n_fft - sp.hop) / 2;  // 480: pad = (n_fft - hop) / 2 and hop = 2 * blk, n_fft = 4 * blk
    const int N50 = T / sp.hop, d = sp.enc_dim, nb = sp.n_fft / 2 + 1;
    // Ragged calls (non-causal): clip b has tw.rl.n[b] code frames, geom.enc[0] of the STFT's input blocks and geom.enc[1] frames per code
    // frame.  Every filter with a temporal footprint ends the clip there, so nothing behind a clip's last sample is read.
    const TimeAxis tb = tw.at(T / blk, h->geom.enc[0]);
    const TimeAxis t = tw.at(N50, h->geom.enc[1]);
    const int64_t rows = t.rows();
    // STFT as an implicit GEMM: the signal is a [B, T / blk, blk] "channel-last" tensor, a frame is 4 consecutive blocks
    // starting one block before 2 t (zero padded), the filter bank is the windowed DFT basis (re | im)
    float* ri = c.arena.alloc<float>(rows * 2 * nb);
    QA_TRY(conv_at(c, wav, tb, h->stft_basis, ri, N50, conv_geom(2, 1, 1)));
    float* feat = c.arena.alloc<float>(rows * h->stft_ld);
    QA_RUN(c, launch_stft_post(ri, feat, rows, nb, 2 * nb, h->stft_ld, c.stream));
    c.tap("enc.stft", feat, rows * h->stft_ld);
    float* x = c.arena.alloc<float>(rows * d);
    float* t1 = c.arena.alloc<float>(rows * d);
    float* u = c.arena.alloc<float>(rows * sp.enc_inter);
    // vq/conv.py Conv1d (:39-47): zero padding (k - stride, 0) in the causal variant, (k / 2, k / 2) otherwise
    const bool cz = t.causal;
    QA_TRY(conv_at(c, feat, t, h->enc_embed, t1, N50, conv_geom(1, cz ? 2 : 1, cz ? 0 : 1)));
    QA_TRY(layernorm_op(c, t1, h->enc_norm_w, h->enc_norm_b, x, rows, d, 1e-6f));
    for (const ConvNeXtW& w : h->enc_cnx) QA_TRY(convnext_op(c, w, x, t1, u, t, d));
    c.tap("enc.prior", x, rows * d);
    QA_TRY(transformer_op(c, h->enc_tr, x, t, "encoder.post_net.1"));
    QA_TRY(layernorm_op(c, x, h->enc_fnorm_w, h->enc_fnorm_b, t1, rows, d, 1e-6f));
    const int k = h->enc_out20.ksize, st = sp.frame_stride;
    const int pl = cz ? k - st : k / 2, pr = cz ? 0 : k / 2;
    const int Nf = (N50 + pl + pr - k) / st + 1;
    float* emb = c.arena.alloc<float>((size_t)B * Nf * sp.code_dim);
    QA_TRY(conv_at(c, t1, t, h->enc_out20, emb, Nf, conv_geom(st, pl, pr)));
    *emb_out = emb;
    *n50_out = N50;
    *nf_out = Nf;
    return QA_OK;
}

// SEANet encoder (seanet.py:121-187): wav [B, T] -> emb [B, N25, code_dim] (*emb_out null: an arena buffer); *n50_out: the frames of its
// transformer.
// Ragged calls (H-Codec 1.0, non-causal): clip b has tw.rl.n[b] code frames.  Every stage's length is that count times the stage's frames
// per code frame (h->geom.enc), which is what each layer with a temporal footprint receives; samples behind a clip's end are never read,
// and the rows behind it that the rectangular launches still compute stay finite (they are built from valid rows and zeros).
// st: null for a whole utterance, else one step of a stream - wav holds the next tw.T / geom.samples code frames of
// a causal model.  The ladder is the same; what differs is where a convolution with a temporal footprint finds its left context (sconv
// below) and the front: a step takes the unfused launches, as a ragged call does - the fused front stages whole halo tiles with a reflect
// rule of its own (a carried-halo form of it is not built) - and has neither lengths nor taps.  The 1x1 shortcut and the 1x1 behind the k3
// are row-wise and carry nothing.  The Transformer continues over its carried (h, c) and K / V rows at 2 frames per code frame.  A step
// reads st->cur and st->tr.off / rows, which the step front advances behind a successful step.  With rows (per-row lengths, section 45)
// every window holds zeros behind a row's own frames, so whatever the caller's waveform holds there never enters the ladder; the launches
// between the windows run on the rectangle.
int seanet_encoder(qa_hcodec* h, Ctx& c, const float* wav, const TimeAxis& tw, float** emb_out, int* n50_out, int* n25_out,
                   CodecStream* st = nullptr) {
    const qa_hcodec_spec& sp = h->spec;
    const int B = tw.B;
    const bool cz = tw.causal, taps = c.capture && !st;
    int C = sp.n_filters;
    TimeAxis t = tw;
    size_t ci = 0;
    const int code_frames = st ? tw.T / h->geom.samples : 0;
    // stream: the window [B, ctx + L, C] of the next stateful convolution over chunk [B, L, C], assembled from its carried state (first
    // step: the reflection of the chunk) and the chunk; conv_op has no batch stride for x, so the window is a buffer of its own.  The state
    // of a convolution is the raw rows of its own input buffer, before any prologue ELU; for the down convs those rows hold the fused
    // post-ELU values.
    auto window = [&](const float* chunk, int L, int Cw, float** win) -> int {
        QA_REQUIRE(ci < st->convs.size() && st->convs[ci].C == Cw, "stream: convolution %zu of the ladder has no state of %d channels", ci, Cw);
        const StreamConv& sc = st->convs[ci++];
        *win = c.arena.alloc<float>((size_t)B * (sc.ctx + L) * Cw);
        // per-row lengths: the row's live rows of this buffer are its code frames times the buffer's rows per code frame
        const bool rs = st->tr.rows;
        QA_RUN(c, launch_stream_window(sc.st[st->cur], chunk, *win, sc.st[st->cur ^ 1], B, sc.ctx, L, Cw, st->tr.offset() == 0 ? 1 : 0, c.stream,
                                       rs ? ClipLens{st->tr.dev[0], L / code_frames} : ClipLens(), rs ? st->tr.dev[1] : nullptr));
        return QA_OK;
    };
    // SConv1d(k = w.ksize, stride) over x [B, ta.T, w.C_in] -> *y [B, *T_out, w.N] (*y null: an arena buffer); o: prologue and epilogue.
    // Offline the paddings of sconv_geom, reflected.  In a stream a VALID convolution (pads 0 / 0) over the window: a waveform of a whole
    // number of code frames needs no right padding anywhere, so ta.T / stride frames.
    auto sconv = [&](const float* x, const TimeAxis& ta, const ConvW& w, int stride, ConvOpt o, float** y, int* T_out) -> int {
        TimeAxis tx = ta;
        o.stride = stride;
        if (st) {
            float* win = nullptr;
            QA_TRY(window(x, ta.T, w.C_in, &win));
            x = win;
            tx.T += st->convs[ci - 1].ctx;
            *T_out = ta.T / stride;
        } else {
            const SGeom g = sconv_geom(ta.T, w.ksize, stride, cz);
            o.pad_left = g.left;
            o.pad_right = g.right;
            o.pad_mode = PAD_REFLECT;
            *T_out = g.T_out;
        }
        if (!*y) *y = c.arena.alloc<float>((size_t)B * *T_out * w.N);
        return conv_at(c, x, tx, w, *y, *T_out, o);
    };
    // stage 0 at C = 32: conv0 + residual block + ELU in ONE launch (seanet_front.hip): the [B L, 32] conv0 output never exists in HBM
    // ... except in a ragged call, which takes the unfused launches as a capture does: they already resolve padding per (row, tap) and take
    // the clips' lengths there, where the fused kernel stages whole halo tiles of one shared length
    const bool front = seanet_front_supported(C, C / 2, t.T) && !t.rl.n && !st;
    float* x = nullptr;
    if (st) {
        float* win = nullptr;
        QA_TRY(window(wav, t.T, 1, &win));
        x = c.arena.alloc<float>((size_t)t.rows() * C);
        QA_RUN(c, launch_conv_in_window(win, h->conv0_w, h->conv0_b, x, B, st->convs[0].ctx + t.T, C, 7, c.stream));
    } else if (!front || c.capture) {
        x = c.arena.alloc<float>((size_t)t.rows() * C);
        QA_RUN(c, launch_conv_in(wav, h->conv0_w, h->conv0_b, x, B, t.T, C, 7, c.stream, cz ? 6 : -1, t.rl));
        c.tap("enc.conv0", x, t.rows() * C);
    }
    for (int i = 0; i < sp.n_ratios; ++i) {
        const int r = sp.ratios[i], L = t.T;
        const ResBlockW& rb = h->res[i];
        // the block's temporaries stay allocated to the end of the call
        float* sc = c.arena.alloc<float>((size_t)B * L * C);
        if (i == 0 && front) {
            QA_RUN(c, launch_seanet_front(wav, h->conv0_w, h->conv0_b, rb.k3.w, rb.k3.b, rb.sc.w, rb.sc.b, rb.pw.w, rb.pw.b, sc, B, L, C,
                                          C / 2, cz ? 1 : 0, c.stream));
        } else {
            float* hh = c.arena.alloc<float>((size_t)B * L * rb.k3.N);
            int Lk = 0;
            // shortcut_1x1(x)
            QA_TRY(conv_op(c, x, C, B, L, rb.sc, sc, C, L, ConvOpt()));
            // ELU(k3(ELU(x)))  (offline: reflect pad 1,1; causal 2,0 - sconv_geom(L, 3, 1))
            QA_TRY(sconv(x, t, rb.k3, 1, elu_conv_elu(), &hh, &Lk));
            // ELU(shortcut + 1x1(.))  -> the activation in front of the down-sampling conv is fused here
            ConvOpt pw;
            pw.res = sc;
            pw.ldr = C;
            pw.post_act = ACT_ELU;
            QA_TRY(conv_op(c, hh, rb.pw.C_in, B, L, rb.pw, sc, C, L, pw));
        }
        float* y = nullptr;
        int To = 0;
        QA_TRY(sconv(sc, t, h->down[i], r, ConvOpt(), &y, &To));
        x = y;
        t = t.at(To, h->geom.enc[i + 1]);
        C *= 2;
        if (taps) c.tap("enc.stage" + std::to_string(i), x, t.rows() * C);
    }
    QA_REQUIRE(C == sp.dimension, "encoder: channel ladder ends at %d, spec.dimension is %d", C, sp.dimension);
    QA_REQUIRE(!st || t.T * h->geom.samples == 2 * tw.T, "stream: the ladder ends at %d frames for a step of %d samples", t.T, tw.T);
    const TrChunk ch = st ? stream_chunk(st->tr) : TrChunk();
    QA_TRY(transformer_op(c, h->enc_tr, x, t, taps ? "encoder.model." + std::to_string(3 * sp.n_ratios + 2) : std::string(), 0, st ? &ch : nullptr));
    if (taps) c.tap("enc.transformer", x, t.rows() * C);
    ConvOpt eo;
    eo.prologue = ACT_ELU;
    QA_TRY(sconv(x, t, h->enc_out, 2, eo, emb_out, n25_out));
    *n50_out = t.T;
    return QA_OK;
}

// ---- the causal encoder as a stream

// Which models stream, and why the others do not; `fn` names the entry point.
int stream_refuse(const qa_hcodec_spec& sp, const char* fn) {
    const char* why = sp.version == 20 ? "an H-Codec 2.0 model: its encoder has an STFT front and a d = 1536 recurrence with no carried form"
                      : (sp.adaptive || sp.version == 15) ? "an H-Codec 1.5 model: its codes come from a whole-utterance alignment"
                                                          : nullptr;
    if (why) {
        set_error("%s: the chunked encoder exists for the causal H-Codec 1.0 only; this is %s - encode the whole utterance with "
                  "qa_hcodec_encode%s", fn, why, sp.adaptive ? "_adaptive" : "");
        return QA_ERR_UNSUPPORTED;
    }
    if (!sp.causal) {
        set_error("%s: streaming needs a causal model (spec.causal = 1): a non-causal frame depends on samples that have not arrived yet - "
                  "encode the whole utterance with qa_hcodec_encode", fn);
        return QA_ERR_UNSUPPORTED;
    }
    QA_REQUIRE(sp.n_ratios >= 1 && sp.n_ratios <= 8, "%s: spec.n_ratios = %d outside 1 .. 8", fn, sp.n_ratios);
    for (int i = 0; i < sp.n_ratios; ++i) QA_REQUIRE(sp.ratios[i] >= 1 && sp.ratios[i] <= 64, "%s: spec.ratios[%d] = %d", fn, i, sp.ratios[i]);
    return QA_OK;
}

// The stateful convolutions of the causal SEANet encoder in graph order - conv0 (k7), per stage the residual k3 and the down conv
// (k = 2 r, stride r), the out conv (k4, stride 2) - each with ctx = k_eff - stride, the rows of left context a causal SConv1d pads
// (conv.py:203-206).  A waveform of a whole number of code frames needs no right padding anywhere (extra = 0: a stride-1 conv keeps L, a
// k = 2 r / s = r conv has L / r frames with r | L), so a chunk needs nothing from the future.  The first chunk's left padding is the
// reflection of its own first ctx frames, which is what the offline pad1d does only while the input of that layer is LONGER than ctx
// (conv.py:79-96: otherwise the short-input rule, another function): first_min is the fewest code frames for which that holds everywhere.
struct StreamGeom {
    int samples = 0, first_min = 1;
    std::vector<int> ctx, rate;  // per stateful conv: context rows, input rows per code frame
};
StreamGeom stream_geometry(const qa_hcodec_spec& sp) {
    StreamGeom g;
    const std::vector<int> enc = seanet_rates(sp);
    g.samples = enc[0];
    auto add = [&](int k, int stride, int rate) {
        g.ctx.push_back(k - stride);
        g.rate.push_back(rate);
    };
    add(7, 1, enc[0]);
    for (int i = 0; i < sp.n_ratios; ++i) {
        add(3, 1, enc[i]);
        add(2 * sp.ratios[i], sp.ratios[i], enc[i]);
    }
    add(4, 2, 2);
    for (size_t i = 0; i < g.ctx.size(); ++i) g.first_min = std::max(g.first_min, g.ctx[i] / g.rate[i] + 1);  // n rate > ctx
    return g;
}

// one step of Codec.encode's acoustic half: SEANet step -> emb [B, n, code_dim] -> ResidualVQ -> codes [B, nq, n]; either output may be null
int stream_encode_graph(qa_hcodec* h, Ctx& c, const float* wav, int n, long long* ac_out, float* emb_out) {
    const qa_hcodec_spec& sp = h->spec;
    const int B = h->strm->tr.B, Q = sp.num_quantizers;
    float* emb = emb_out ? emb_out : c.arena.alloc<float>((size_t)B * n * sp.code_dim);
    int n50 = 0, n25 = 0;
    QA_TRY(seanet_encoder(h, c, wav, TimeAxis{B, n * h->geom.samples, true, ClipLens()}, &emb, &n50, &n25, h->strm.get()));
    // per-row lengths: exact zeros behind a row's frames in emb (in front of the search, which then sees finite rows it would see anyway),
    // and the dropped code -1 there, as a ragged encode writes them
    const int* rs = h->strm->tr.rows ? h->strm->tr.dev[0] : nullptr;
    if (rs) QA_RUN(c, launch_lm_rows_zero_pad(emb, 0, 1, B, n, sp.code_dim, rs, c.stream));
    if (!ac_out) return QA_OK;
    long long* ia = c.arena.alloc<long long>((size_t)B * n * Q);
    float* rvq_ws = c.arena.alloc<float>(rvq_scratch_floats((long long)B * n, sp.codebook_size, sp.code_dim));
    QA_RUN(c, launch_rvq_search(emb, (long long)B * n, h->cb_a, h->e2_a, Q, sp.codebook_size, sp.code_dim, ia, nullptr, 0, rvq_ws, c.stream));
    QA_RUN(c, launch_codes_to_bqn(ia, ac_out, B, n, Q, c.stream, rs));
    return QA_OK;
}

// Semantic encoder (semantic_module.py:157-201): feat [B, sem_in, f.n] -> sem [B, *ls_out, code_dim].  tf: the feature frames' axis; in a
// ragged call feature frames behind a clip's end are never read (the rates of the stages are h->geom.sem).
int semantic_encoder(qa_hcodec* h, Ctx& c, const FeatView& f, const TimeAxis& tf, float** sem_out, int* ls_out) {
    const qa_hcodec_spec& sp = h->spec;
    QA_REQUIRE(f.n > 0, "encode: feat has no frames");
    const int B = tf.B, SC = sp.sem_ch;
    const float* fcl = f.p;
    if (!(f.sc == 1 && f.st == sp.sem_in && f.sb == (int64_t)f.n * sp.sem_in)) {
        float* buf = c.arena.alloc<float>((size_t)B * f.n * sp.sem_in);
        QA_TRY(to_channel_last_op(c, f.p, f.sb, f.sc, f.st, buf, B, sp.sem_in, f.n));
        fcl = buf;
    }
    TimeAxis t = tf;
    float* s = c.arena.alloc<float>((size_t)t.rows() * SC);
    float* tmp = c.arena.alloc<float>((size_t)t.rows() * SC);
    QA_TRY(conv_same(c, fcl, t, h->sem_in, s));
    for (size_t bi = 0; bi < h->sem_blocks.size(); ++bi) {
        const auto& blk = h->sem_blocks[bi];
        for (int u = 0; u < 2; ++u) {
            QA_TRY(conv_same(c, s, t, blk.u1[u], tmp, elu_conv_elu()));      // ELU(conv1(ELU(s)))
            QA_TRY(conv_same(c, tmp, t, blk.u2[u], s, epi(ACT_NONE, s)));  // s + conv2(.): 1x1, row-wise
        }
        const int k = blk.conv.ksize, pad = (k - 1) / 2;
        const int To = (t.T + 2 * pad - k) / blk.stride + 1;
        float* y = c.arena.alloc<float>((size_t)B * To * SC);
        QA_TRY(conv_at(c, s, t, blk.conv, y, To, conv_geom(blk.stride, pad, pad)));
        s = y;
        t = t.at(To, h->geom.sem[bi + 1]);
    }
    float* sem = c.arena.alloc<float>((size_t)t.rows() * sp.code_dim);
    QA_TRY(conv_same(c, s, t, h->sem_out, sem));
    *sem_out = sem;
    *ls_out = t.T;
    return QA_OK;
}

// acoustic encoder + semantic encoder: wav, feat -> emb, sem  [B, N25, code_dim] each (codec.py:169-170); independent of each other
// until the RVQ / alignment.  tw: the waveform's axis (in a ragged call its lengths are samples, h->geom.samples per code frame).
int encode_front(qa_hcodec* h, Ctx& c, const float* wav, const TimeAxis& tw, const FeatView& f, float** emb_out, float** sem_out,
                 int* n25_out) {
    int N50 = 0, N25 = 0, Ls = 0;
    if (h->spec.version == 20) {
        QA_TRY(encoder20(h, c, wav, tw, emb_out, &N50, &N25));
    } else {
        QA_TRY(seanet_encoder(h, c, wav, tw, emb_out, &N50, &N25));
    }
    c.tap("enc.emb", *emb_out, (int64_t)tw.B * N25 * h->spec.code_dim);
    TimeAxis tf = tw.at(f.n, h->geom.feat);
    tf.causal = false;  // the semantic encoder has no causal variant
    QA_TRY(semantic_encoder(h, c, f, tf, sem_out, &Ls));
    QA_REQUIRE(Ls == N25, "encode: semantic stream has %d frames, acoustic stream %d (feat must have T/%d frames)", Ls, N25,
               tw.T / std::max(1, N50));
    c.tap("enc.sem", *sem_out, (int64_t)tw.B * Ls * h->spec.code_dim);
    *n25_out = N25;
    return QA_OK;
}

int encode_graph(qa_hcodec* h, Ctx& c, const float* wav, const TimeAxis& tw, const FeatView& f, long long* ac_out, long long* sc_out) {
    const qa_hcodec_spec& sp = h->spec;
    const int B = tw.B;
    float *emb = nullptr, *sem = nullptr;
    int N25 = 0;
    QA_TRY(encode_front(h, c, wav, tw, f, &emb, &sem, &N25));
    // ---- RVQ (both streams)
    const int Q = sp.num_quantizers;
    long long* ia = c.arena.alloc<long long>((size_t)B * N25 * Q);
    long long* is = c.arena.alloc<long long>((size_t)B * N25 * Q);
    float* rvq_ws = c.arena.alloc<float>(rvq_scratch_floats((long long)B * N25, sp.codebook_size, sp.code_dim));
    QA_RUN(c, launch_rvq_search(emb, (long long)B * N25, h->cb_a, h->e2_a, Q, sp.codebook_size, sp.code_dim, ia, nullptr, 0, rvq_ws, c.stream));
    QA_RUN(c, launch_rvq_search(sem, (long long)B * N25, h->cb_s, h->e2_s, Q, sp.codebook_size, sp.code_dim, is, nullptr, 0, rvq_ws, c.stream));
    QA_RUN(c, launch_codes_to_bqn(ia, ac_out, B, N25, Q, c.stream, tw.rl.n));  // ragged: -1 behind a clip's last code frame
    QA_RUN(c, launch_codes_to_bqn(is, sc_out, B, N25, Q, c.stream, tw.rl.n));
    return QA_OK;
}

// CodecDecoder.forward (codec_decoder.py:58-67) from the concatenated [acoustic | semantic] embeddings [B, N, 2*code_dim]; tc: the code
// frames' axis.  Ragged calls (H-Codec 1.0 / 2.0, non-causal): clip b has tc.rl.n[b] of the N code frames, geom.dec times as many decoder
// frames (2; H-Codec 2.0: frame_stride).
int decode_tail(qa_hcodec* h, Ctx& c, const float* cat, const TimeAxis& tc, float* wav_out) {
    const qa_hcodec_spec& sp = h->spec;
    const int d = sp.dec_dim, B = tc.B, N = tc.T;
    const int64_t rows25 = tc.rows();
    const TimeAxis t = tc.at(h->geom.dec * N, h->geom.dec);  // the decoder's frames
    const int64_t rows = t.rows();
    float* x = c.arena.alloc<float>(rows * d);
    if (sp.version == 20) {
        // H-Codec 2.0 (codec_decoder.py:30-31,64-65): x.repeat_interleave(s) -> Conv1d k = s + 1, "same" zero padding.  The
        // repetition is folded into the implicit-GEMM gather (frame r reads row r / s), nothing is materialised.
        const int k = h->dec_embed20.ksize;
        ConvOpt o = conv_geom(1, zpad_left(k, t.causal), zpad_right(k, t.causal));
        o.in_rep = sp.frame_stride;
        o.rl = t.rl;  // ragged: the clip ends at geom.dec * frames[b] VIRTUAL (repeated) frames, so a tap behind it reads the zero padding
        QA_TRY(conv_op(c, cat, 2 * sp.code_dim, B, N, h->dec_embed20, x, d, t.T, o));
    } else {
        // sub-pixel upsampler: 1x1 conv to 2*d channels; in channel-last layout the pixel shuffle (vq/conv.py:86-88) is a
        // pure reinterpretation [B, N, 2, d] -> [B, 2N, d]
        float* up = c.arena.alloc<float>(rows25 * 2 * d);
        QA_TRY(linear_op(c, cat, rows25, h->up, up));
        QA_TRY(dwconv_op(c, up, h->up_dw, h->up_dwb, nullptr, nullptr, x, B, t.T, d, 5, 0.f, zpad_left(5, t.causal), t.rl));
    }
    c.tap("dec.embed", x, rows * d);
    QA_TRY(dec_resblock_op(c, h->dres[0], x, t, d, sp.gn_groups));
    QA_TRY(dec_resblock_op(c, h->dres[1], x, t, d, sp.gn_groups));
    c.tap("dec.prior_res1", x, rows * d);
    QA_TRY(transformer_op(c, h->dec_tr, x, t, "decoder.prior_net.3"));
    c.tap("dec.transformer", x, rows * d);
    QA_TRY(dec_resblock_op(c, h->dres[2], x, t, d, sp.gn_groups));
    QA_TRY(dec_resblock_op(c, h->dres[3], x, t, d, sp.gn_groups));
    float* t1 = c.arena.alloc<float>(rows * d);
    float* u = c.arena.alloc<float>(rows * sp.dec_inter);
    QA_TRY(groupnorm_op(c, x, h->gn_w, h->gn_b, t1, t, d, sp.gn_groups, 0));
    QA_TRY(layernorm_op(c, t1, h->norm_w, h->norm_b, x, rows, d, 1e-6f));
    c.tap("dec.prior", x, rows * d);
    for (const ConvNeXtW& w : h->cnx) QA_TRY(convnext_op(c, w, x, t1, u, t, d));
    QA_TRY(layernorm_op(c, x, h->fnorm_w, h->fnorm_b, t1, rows, d, 1e-6f));
    c.tap("dec.backbone", t1, rows * d);
    // ISTFT head
    const int nb = sp.n_fft / 2 + 1;
    float* y = c.arena.alloc<float>(rows * 2 * nb);
    float* S = c.arena.alloc<float>(rows * h->spec_ld);
    float* frames = c.arena.alloc<float>(rows * sp.n_fft);
    QA_TRY(linear_op(c, t1, rows, h->head, y));
    QA_RUN(c, launch_istft_spec(y, S, rows, nb, 2 * nb, h->spec_ld, c.stream));
    c.tap("dec.spec", S, rows * h->spec_ld);
    QA_TRY(linear_op(c, S, rows, h->basis, frames));
    QA_RUN(c, launch_istft_ola(frames, h->window, wav_out, B, t.T, sp.n_fft, sp.hop, c.stream, t.rl));
    return QA_OK;
}

int decode_graph(qa_hcodec* h, Ctx& c, const long long* ac, const long long* scodes, const TimeAxis& tc, float* wav_out) {
    const qa_hcodec_spec& sp = h->spec;
    const int Q = sp.num_quantizers, D = sp.code_dim, B = tc.B, N = tc.T;
    const int64_t rows25 = tc.rows();
    long long* ia = c.arena.alloc<long long>(rows25 * Q);
    long long* is = c.arena.alloc<long long>(rows25 * Q);
    float* cat = c.arena.alloc<float>(rows25 * 2 * D);
    QA_RUN(c, launch_codes_from_bqn(ac, ia, B, N, Q, c.stream, tc.rl.n));  // ragged: entries behind a clip's end are read as dropped codes
    QA_RUN(c, launch_codes_from_bqn(scodes, is, B, N, Q, c.stream, tc.rl.n));
    QA_RUN(c, launch_rvq_lookup(ia, rows25, h->cb_a, Q, sp.codebook_size, D, cat, 2 * D, c.stream));
    QA_RUN(c, launch_rvq_lookup(is, rows25, h->cb_s, Q, sp.codebook_size, D, cat + D, 2 * D, c.stream));
    return decode_tail(h, c, cat, tc, wav_out);
}

// ---- H-Codec 1.5 (codec_adaptive.py:150-199)

int read_scalar(Ctx& c, qa_hcodec* h, const int* dev, int* out) {
    QA_HIP(hipMemcpyAsync(h->host_sync, dev, sizeof(int), hipMemcpyDeviceToHost, c.stream));
    QA_HIP(hipStreamSynchronize(c.stream));  // data-dependent shape: the reference syncs here too (modeling_flexicodec_new.py:910)
    lstm_call_note_sync();                   // ... which also puts every recurrence launched so far behind a host synchronisation
    *out = *h->host_sync;
    return QA_OK;
}

// Per-clip calls (tw.rl.n: the clips' code-frame counts): clip b is aligned over its own frames, its interleaved row
// holds its own frames and groups and nothing else is a visible key, so row b is the call on that clip alone; codes behind its groups are -1.
int encode_adaptive_graph(qa_hcodec* h, Ctx& c, const float* wav, const TimeAxis& tw, const FeatView& f, long long* ac_out,
                          long long* sc_out, int* G_out, float threshold) {
    const qa_hcodec_spec& sp = h->spec;
    const int D = sp.code_dim, Q = sp.num_quantizers, B = tw.B;
    float *emb = nullptr, *sem = nullptr;
    int N = 0;
    QA_TRY(encode_front(h, c, wav, tw, f, &emb, &sem, &N));
    const int* lens = tw.rl.n;  // code frames per clip, or null
    int* seg = c.arena.alloc<int>((size_t)B * N);
    int* start = c.arena.alloc<int>((size_t)B * N);
    int* len = c.arena.alloc<int>((size_t)B * N);
    int* nseg = c.arena.alloc<int>(B);
    int* gmax = c.arena.alloc<int>(1);
    int G = N;  // planning pass: worst case, every frame its own group
    if (!c.dry) {  // real pass only, more than launches: the group count is read back and checked
        QA_TRY(launch_align(sem, B, N, D, threshold, sp.max_tokens_per_group, seg, start, len, nseg, gmax, lens, c.stream));
        QA_TRY(read_scalar(c, h, gmax, &G));
        QA_REQUIRE(G >= 1 && G <= N, "encode: alignment produced %d groups for %d frames", G, N);
    }
    *G_out = G;
    const int S = N + G;
    float* inter_s = c.arena.alloc<float>((size_t)B * S * D);
    float* inter_a = c.arena.alloc<float>((size_t)B * S * D);
    float* agg_a = c.arena.alloc<float>((size_t)B * G * D);
    float* agg_s = c.arena.alloc<float>((size_t)B * G * D);
    // semantic_aggregator(sem), acoustic_aggregator(emb): both use the alignment of the semantic stream and are otherwise
    // independent, so the two 32-layer stacks run concurrently on two streams (fork / join with events; no host sync)
    hipStream_t side = serial_mode() ? c.stream : h->side;  // qa_set_serial(1): one stream
    QA_RUN(c, launch_agg_build(sem, seg, start, len, nseg, h->qemb_sem, inter_s, B, N, G, D, lens, c.stream));
    QA_RUN(c, launch_agg_build(emb, seg, start, len, nseg, h->qemb_ac, inter_a, B, N, G, D, lens, c.stream));
    unsigned char* kvalid = nullptr;  // the aggregators' key mask: in front of the fork, so both streams see it
    if (lens) {
        kvalid = c.arena.alloc<unsigned char>((size_t)B * S);
        QA_RUN(c, launch_agg_key_mask(kvalid, B, N, G, lens, nseg, c.stream));
    }
    if (!c.dry) {  // real pass only: the event fork
        QA_HIP(hipEventRecord(h->ev_fork, c.stream));
        QA_HIP(hipStreamWaitEvent(side, h->ev_fork, 0));
    }
    // QA_AGG_LAST_ROWS: the last layer of each stack on the query rows only, read-out included (non-causal aggregators)
    if (knob(K_AGG_LAST_ROWS) != 0 && !h->agg_sem.causal && !h->agg_ac.causal && !h->agg_sem.layers.empty()) {
        const AggReadout rs{start, len, nseg, N, G, agg_s}, ra{start, len, nseg, N, G, agg_a};
        QA_TRY(mimi_pair_op(c, side, MimiStack{h->agg_sem, inter_s, B, kvalid, &rs}, MimiStack{h->agg_ac, inter_a, B, kvalid, &ra}, S));
    } else {
        QA_TRY(mimi_pair_op(c, side, MimiStack{h->agg_sem, inter_s, B, kvalid, nullptr}, MimiStack{h->agg_ac, inter_a, B, kvalid, nullptr}, S));
        QA_RUN(c, launch_agg_gather(inter_s, start, len, nseg, agg_s, B, N, G, D, c.stream));
        QA_RUN(c, launch_agg_gather(inter_a, start, len, nseg, agg_a, B, N, G, D, side));
    }
    if (!c.dry) {  // real pass only: the event join
        QA_HIP(hipEventRecord(h->ev_join, side));
        QA_HIP(hipStreamWaitEvent(c.stream, h->ev_join, 0));
    }
    c.tap("enc.emb_agg", agg_a, (int64_t)B * G * D);
    c.tap("enc.sem_agg", agg_s, (int64_t)B * G * D);
    long long* ia = c.arena.alloc<long long>((size_t)B * G * Q);
    long long* is = c.arena.alloc<long long>((size_t)B * G * Q);
    float* rvq_ws = c.arena.alloc<float>(rvq_scratch_floats((long long)B * G, sp.codebook_size, D));
    QA_RUN(c, launch_rvq_search(agg_a, (long long)B * G, h->cb_a, h->e2_a, Q, sp.codebook_size, D, ia, nullptr, 0, rvq_ws, c.stream));
    QA_RUN(c, launch_rvq_search(agg_s, (long long)B * G, h->cb_s, h->e2_s, Q, sp.codebook_size, D, is, nullptr, 0, rvq_ws, c.stream));
    QA_RUN(c, launch_codes_inject(ia, len, ac_out, B, N, G, Q, sp.codebook_size, lens != nullptr, c.stream));
    QA_RUN(c, launch_codes_inject(is, len, sc_out, B, N, G, Q, sp.codebook_size, lens != nullptr, c.stream));
    return QA_OK;
}

// tc: the axis of the N de-aggregated code frames; G groups per clip in the codes.  Per-clip calls (tc.rl.n): clip b de-aggregates at most
// tc.rl.n[b] frames, and its bottleneck transformer and decoder see that many.
int decode_adaptive_graph(qa_hcodec* h, Ctx& c, const long long* ac, const long long* scodes, const TimeAxis& tc, int G, float* wav_out) {
    const qa_hcodec_spec& sp = h->spec;
    const int Q = sp.num_quantizers, D = sp.code_dim, B = tc.B, N = tc.T;
    const int64_t rows = tc.rows();
    long long* ia = c.arena.alloc<long long>(rows * Q);
    long long* is = c.arena.alloc<long long>(rows * Q);
    float* cat = c.arena.alloc<float>(rows * 2 * D);
    // token lengths: the reference keeps the ones extracted from the SEMANTIC codes for both streams (codec_adaptive.py:185-186)
    QA_RUN(c, launch_deaggregate(ac, scodes, ia, B, Q, G, N, sp.codebook_size, tc.rl.n, c.stream));
    QA_RUN(c, launch_deaggregate(scodes, scodes, is, B, Q, G, N, sp.codebook_size, tc.rl.n, c.stream));
    QA_RUN(c, launch_rvq_lookup(ia, rows, h->cb_a, Q, sp.codebook_size, D, cat, 2 * D, c.stream));
    QA_RUN(c, launch_rvq_lookup(is, rows, h->cb_s, Q, sp.codebook_size, D, cat + D, 2 * D, c.stream));
    unsigned char* kvalid = nullptr;
    if (tc.rl.n) {
        kvalid = c.arena.alloc<unsigned char>(rows);
        QA_RUN(c, launch_len_mask(kvalid, B, N, ClipLens{tc.rl.n, 1}, c.stream));
    }
    // QA_BATCH_SPLIT bit 1: the stack over the two halves of the batch, clips [0, ceil(B / 2)) on the caller's stream and the rest on
    // `side`, layer-interleaved like the aggregators - one half's LayerNorms and attention run beside the other half's GEMMs, and the
    // partly filled last round of a GEMM's tiles is covered.  One lane, as before, for a single clip, under
    // qa_set_serial(1), with taps on, or when the smaller half has fewer than QA_BATCH_SPLIT_MIN_ROWS rows.
    const int B0 = (B + 1) / 2, B1 = B - B0;
    if ((knob(K_BATCH_SPLIT) & 1) != 0 && B1 >= 1 && !serial_mode() && !c.capture && (int64_t)B1 * N >= knob(K_BATCH_SPLIT_MIN_ROWS)) {
        const int64_t r0 = (int64_t)B0 * N;
        if (!c.dry) {  // real pass only: the event fork
            QA_HIP(hipEventRecord(h->ev_fork, c.stream));
            QA_HIP(hipStreamWaitEvent(h->side, h->ev_fork, 0));
            g_split_regions.fetch_add(1, std::memory_order_relaxed);
        }
        QA_TRY(mimi_pair_op(c, h->side, MimiStack{h->bottleneck, cat, B0, kvalid, nullptr},
                            MimiStack{h->bottleneck, cat + r0 * 2 * D, B1, kvalid ? kvalid + r0 : nullptr, nullptr}, N, 2));
        if (!c.dry) {  // real pass only: the event join, in front of decode_tail - its recurrences find the device empty
            QA_HIP(hipEventRecord(h->ev_join, h->side));
            QA_HIP(hipStreamWaitEvent(c.stream, h->ev_join, 0));
        }
    } else {
        QA_TRY(mimi_op(c, h->bottleneck, cat, B, N, kvalid));
    }
    c.tap("dec.bottleneck", cat, rows * 2 * D);
    return decode_tail(h, c, cat, tc, wav_out);
}

// ---- Codec.forward (codec.py:138-162, codec_adaptive.py:100-148): encode -> RVQ -> decode with the codes kept on the device, and the
// semantic decoder on the looked-up semantic embedding

// SemanticDecoder.forward (semantic_module.py:294-299) on the channel-last summed semantic code vectors z [B, N, code_dim] (row
// stride ldz) -> pred [B, output_channels, N * prod(strides)], channel-first like the reference.
int semantic_decoder_op(const qa_hcodec::SemDec& sd, Ctx& c, const float* z, int64_t ldz, int B, int N, float* pred) {
    const qa_semantic_decoder_spec& sp = sd.spec;
    int L = N, C = sp.channels;
    float* x = c.arena.alloc<float>((size_t)B * L * C);
    QA_TRY(conv_op(c, z, ldz, B, L, sd.conv1, x, C, L, conv_geom(1, 1, 1)));
    for (const auto& blk : sd.blocks) {
        const int s = blk.stride, co = blk.c_out, To = L * s;
        const TimeAxis to{B, To, false, ClipLens()};
        float* y = c.arena.alloc<float>((size_t)B * To * co);
        if (s == 1) {
            QA_TRY(conv_same(c, x, to, blk.conv, y));
        } else {  // ConvTranspose1d: phase phi writes rows q * s + phi (row stride s * co)
            for (int phi = 0; phi < s; ++phi) {
                const ConvW& w = blk.phase[phi];
                QA_TRY(conv_op(c, x, C, B, L, w, y + (size_t)phi * co, (int64_t)s * co, L,
                               conv_geom(1, blk.pad_left[phi], w.ksize - 1 - blk.pad_left[phi])));
            }
        }
        float* t = c.arena.alloc<float>((size_t)B * To * co);
        for (int u = 0; u < 2; ++u) {
            QA_TRY(conv_same(c, y, to, blk.u1[u], t, elu_conv_elu()));      // ELU(conv1(ELU(y)))
            QA_TRY(conv_same(c, t, to, blk.u2[u], y, epi(ACT_NONE, y)));  // y + conv2(.)
        }
        x = y;
        L = To;
        C = co;
    }
    const int O = sp.output_channels;
    float* o = c.arena.alloc<float>((size_t)B * L * O);
    QA_TRY(conv_same(c, x, TimeAxis{B, L, false, ClipLens()}, sd.conv2, o));
    c.tap("sem_dec.out", o, (int64_t)B * L * O);
    // [B, L, O] read as a [B, C' = L, T' = O] tensor with strides (L O, O, 1): its channel-last form is [B, O, L]
    return to_channel_last_op(c, o, (long long)L * O, O, 1, pred, B, L, O);
}

// the semantic decoder from device-resident semantic indices [B*N, Q]: the look-up decode makes, then semantic_decoder_op.  It runs on
// the caller's stream behind the codec decoder: on a second stream next to it the call measured no faster.
int semantic_decoder_from_codes(qa_hcodec* h, Ctx& c, const long long* is_rows, int B, int N, float* pred) {
    const qa_hcodec_spec& sp = h->spec;
    const int64_t rows = (int64_t)B * N;
    float* z = c.arena.alloc<float>(rows * sp.code_dim);
    QA_RUN(c, launch_rvq_lookup(is_rows, rows, h->cb_s, sp.num_quantizers, sp.codebook_size, sp.code_dim, z, sp.code_dim, c.stream));
    return semantic_decoder_op(*h->sdec, c, z, sp.code_dim, B, N, pred);
}

// tw: the waveform's axis; N = tw.T / h->geom.samples code frames
int forward_graph(qa_hcodec* h, Ctx& c, const float* wav, const TimeAxis& tw, const FeatView& f, int N, float* recon, float* pred) {
    const int Q = h->spec.num_quantizers, B = tw.B;
    const TimeAxis tc = tw.at(N, 1);
    long long* ac = c.arena.alloc<long long>((size_t)B * Q * N);
    long long* sc = c.arena.alloc<long long>((size_t)B * Q * N);
    QA_TRY(encode_graph(h, c, wav, tw, f, ac, sc));
    // the decoder's own path from the codes (decode_graph), so recon is decode(encode()) bit for bit
    long long* is = c.arena.alloc<long long>((size_t)B * N * Q);
    QA_RUN(c, launch_codes_from_bqn(sc, is, B, N, Q, c.stream));
    QA_TRY(decode_graph(h, c, ac, sc, tc, recon));
    return semantic_decoder_from_codes(h, c, is, B, N, pred);
}

int forward_adaptive_graph(qa_hcodec* h, Ctx& c, const float* wav, const TimeAxis& tw, const FeatView& f, int N, float* recon, float* pred,
                           long long* token_lengths, int* G_out) {
    const qa_hcodec_spec& sp = h->spec;
    const int Q = sp.num_quantizers, K = sp.codebook_size, B = tw.B;
    long long* ac = c.arena.alloc<long long>((size_t)B * Q * N);
    long long* sc = c.arena.alloc<long long>((size_t)B * Q * N);
    int G = 0;
    QA_TRY(encode_adaptive_graph(h, c, wav, tw, f, ac, sc, &G, sp.threshold));
    *G_out = G;
    // every item's groups cover all N frames (x_lens = T for the whole batch, codec_adaptive.py:106-107): decode at N frames
    long long* is = c.arena.alloc<long long>((size_t)B * N * Q);
    QA_RUN(c, launch_token_lengths(sc, token_lengths, B, Q, G, K, c.stream));
    QA_RUN(c, launch_deaggregate(sc, sc, is, B, Q, G, N, K, nullptr, c.stream));  // codec_adaptive.py:134-135
    QA_TRY(decode_adaptive_graph(h, c, ac, sc, tw.at(N, 1), G, recon));
    return semantic_decoder_from_codes(h, c, is, B, N, pred);
}

// semantic_decoder.* of the reference's state_dict: every key checked in module order first (the error names the FIRST missing or
// mis-shaped one), then folded into a store of its own
int build_semantic_decoder(qa_hcodec* h, const qa_semantic_decoder_spec& sp, const HostTable& tab, std::unique_ptr<qa_hcodec::SemDec>* out) {
    QA_REQUIRE(sp.n_blocks >= 1 && sp.n_blocks <= 4, "semantic decoder: n_blocks %d outside [1, 4]", sp.n_blocks);
    QA_REQUIRE(sp.code_dim == h->spec.code_dim, "semantic decoder: code_dim %d != the codec's %d", sp.code_dim, h->spec.code_dim);
    QA_REQUIRE(sp.channels > 0 && sp.channels % 32 == 0 && sp.output_channels > 0 && sp.output_channels % 32 == 0,
               "semantic decoder: channels %d / output_channels %d must be positive multiples of 32", sp.channels, sp.output_channels);
    for (int i = 0; i < sp.n_blocks; ++i) {
        QA_REQUIRE(sp.widths[i] > 0 && sp.widths[i] % 32 == 0, "semantic decoder: block %d width %d must be a positive multiple of 32", i,
                   sp.widths[i]);
        // ConvTranspose1d(k = 2 s, padding (s + 1) // 2, output_padding s % 2) (semantic_module.py:86-104): for even s the padding is
        // (k - s) / 2 and the output exactly s frames per input frame; odd strides are not implemented
        QA_REQUIRE(sp.strides[i] == 1 || (sp.strides[i] >= 2 && sp.strides[i] % 2 == 0),
                   "semantic decoder: block %d stride %d: only stride 1 and even strides are supported", i, sp.strides[i]);
    }
    const std::string p = "semantic_decoder.";
    std::vector<std::pair<std::string, int64_t>> keys;
    keys.push_back({p + "conv1.conv.weight", (int64_t)sp.channels * sp.code_dim * 3});
    for (int i = 0, ci = sp.channels; i < sp.n_blocks; ci = sp.widths[i], ++i) {
        const std::string bp = p + "conv_blocks." + std::to_string(i);
        const int s = sp.strides[i], co = sp.widths[i];
        const std::string cp = bp + (s == 1 ? ".conv.conv" : ".conv.deconv");
        keys.push_back({cp + ".weight", (int64_t)co * ci * (s == 1 ? 3 : 2 * s)});
        keys.push_back({cp + ".bias", co});
        for (int u = 0; u < 2; ++u) {
            keys.push_back({bp + ".res_units." + std::to_string(u) + ".conv1.conv.weight", (int64_t)co * co * 3});
            keys.push_back({bp + ".res_units." + std::to_string(u) + ".conv2.weight", (int64_t)co * co});
        }
    }
    keys.push_back({p + "conv2.conv.weight", (int64_t)sp.output_channels * sp.widths[sp.n_blocks - 1] * 3});
    for (const auto& k : keys)
        if (!tab.get(k.first, k.second)) return QA_ERR_MISSING;  // HostTable::get has set the error message
    std::unique_ptr<qa_hcodec::SemDec> sd(new qa_hcodec::SemDec());
    sd->spec = sp;
    Loader b(tab, sd->store);
    b.conv(&sd->conv1, p + "conv1.conv", sp.channels, sp.code_dim, 3, false);
    sd->blocks.resize(sp.n_blocks);
    for (int i = 0, ci = sp.channels; i < sp.n_blocks; ci = sp.widths[i], ++i) {
        auto& blk = sd->blocks[i];
        const std::string bp = p + "conv_blocks." + std::to_string(i);
        const int s = sp.strides[i], co = sp.widths[i];
        blk.stride = s;
        blk.c_out = co;
        if (s == 1) {
            b.conv(&blk.conv, bp + ".conv.conv", co, ci, 3);
        } else {  // weight [C_in][C_out][2 s], padding s / 2
            const float* w = b.need(bp + ".conv.deconv.weight", (int64_t)ci * co * 2 * s);
            blk.phase.resize(s);
            blk.pad_left.resize(s);
            for (int phi = 0; phi < s; ++phi) {
                PolyphaseFilter pf;
                QA_TRY(polyphase_filter(w, ci, co, 2 * s, s, s / 2, phi, &pf));
                ConvW& cw = blk.phase[phi];
                cw.N = co; cw.C_in = ci; cw.ksize = pf.ntaps;
                b.raw(&cw.w, pf.filter);
                b.vec(&cw.b, bp + ".conv.deconv.bias", co);
                blk.pad_left[phi] = pf.pad_left;
            }
        }
        for (int u = 0; u < 2; ++u) {
            const std::string up = bp + ".res_units." + std::to_string(u);
            b.conv(&blk.u1[u], up + ".conv1.conv", co, co, 3, false);
            b.conv(&blk.u2[u], up + ".conv2", co, co, 1, false);
        }
    }
    b.conv(&sd->conv2, p + "conv2.conv", sp.output_channels, sp.widths[sp.n_blocks - 1], 3, false);
    QA_TRY(b.upload());
    *out = std::move(sd);
    return QA_OK;
}

int build(qa_hcodec* h, const HostTable& tab) {
    const qa_hcodec_spec& sp = h->spec;
    const bool v20 = sp.version == 20;
    QA_REQUIRE(sp.version == 0 || sp.version == 10 || sp.version == 15 || v20, "spec: unknown version %d", sp.version);
    QA_REQUIRE(!(v20 && sp.adaptive), "spec: H-Codec 2.0 has no adaptive frame rate");
    QA_REQUIRE(sp.n_sem_strides >= 1 && sp.n_sem_strides <= 4, "spec: bad counts");
    QA_REQUIRE(v20 || (sp.n_ratios >= 1 && sp.n_ratios <= 8 && sp.n_filters % 32 == 0), "spec: bad SEANet ladder");
    QA_REQUIRE((v20 ? sp.enc_dim : sp.dimension) % 128 == 0 && sp.dec_dim % 128 == 0, "spec: transformer widths must be multiples of 128");
    auto tr_inter = [&](int d) { return sp.tr_inter_cap > 0 ? std::min(4 * d, sp.tr_inter_cap) : 4 * d; };
    QA_REQUIRE(sp.sem_in % 32 == 0 && sp.sem_ch % 32 == 0 && sp.code_dim % 32 == 0 && sp.dec_inter % 32 == 0,
               "spec: channel counts must be multiples of 32");
    QA_REQUIRE(sp.n_fft % 2 == 0 && sp.hop > 0 && sp.n_fft > sp.hop && (sp.n_fft - sp.hop) % 2 == 0, "spec: bad STFT geometry");
    QA_REQUIRE(sp.dec_dim % sp.gn_groups == 0, "spec: dec_dim %% gn_groups != 0");
    qa_hcodec::Geom& geom = h->geom;
    geom.sem.assign(sp.n_sem_strides + 1, 1);
    for (int i = sp.n_sem_strides - 1; i >= 0; --i) geom.sem[i] = geom.sem[i + 1] * sp.sem_strides[i];
    geom.feat = geom.sem[0];
    geom.dec = v20 ? sp.frame_stride : 2;
    if (v20) geom.enc = {2 * sp.frame_stride, sp.frame_stride};  // hop = 2 blocks (checked below), frame_stride frames per code frame
    if (!v20) geom.enc = seanet_rates(sp);
    geom.samples = v20 ? sp.hop * sp.frame_stride : geom.enc[0];
    Loader b(tab, h->store);
    auto dw_fold_c = [&](const float** dst, const std::string& name, int k, int ch) {
        std::vector<float> w((size_t)k * ch, 0.f);
        const float* p = b.need(name, (int64_t)ch * k);
        if (p)
            for (int c = 0; c < ch; ++c)
                for (int j = 0; j < k; ++j) w[(size_t)j * ch + c] = p[c * k + j];
        b.raw(dst, w);
    };
    auto fold_convnext = [&](ConvNeXtW& w, const std::string& cp, int ch, int inter) {
        dw_fold_c(&w.dw, cp + ".dwconv.conv.weight", 7, ch);
        b.vec(&w.dwb, cp + ".dwconv.conv.bias", ch);
        b.norm(&w.lnw, &w.lnb, cp + ".norm", ch);
        b.vec(&w.gamma, cp + ".gamma", ch);
        b.linear(&w.pw1, cp + ".pwconv1.linear.weight", cp + ".pwconv1.linear.bias", inter, ch);
        b.linear(&w.pw2, cp + ".pwconv2.linear.weight", cp + ".pwconv2.linear.bias", ch, inter);
    };
    if (v20) {
        // --- H-Codec 2.0 encoder (HCodec-2.0/vq/codec_encoder.py:12-79)
        const int Nf = sp.n_fft, nbins = Nf / 2 + 1, blk = (Nf - sp.hop) / 2, de = sp.enc_dim;
        QA_REQUIRE(sp.hop == 2 * blk && Nf == 4 * blk && blk % 32 == 0, "spec: H-Codec 2.0 needs n_fft = 2 * hop and hop %% 64 == 0");
        QA_REQUIRE(de % 64 == 0 && sp.enc_inter % 32 == 0 && sp.frame_stride >= 1, "spec: bad H-Codec 2.0 encoder widths");
        {   // torchaudio Spectrogram(n_fft, hop, center=False, power=None): X[k] = sum_n hann[n] x[n] e^{-2 pi i k n / N}
            std::vector<float> basis((size_t)2 * nbins * Nf);
            for (int k = 0; k < nbins; ++k)
                for (int n = 0; n < Nf; ++n) {
                    const double wn = 0.5 - 0.5 * std::cos(2.0 * M_PI * n / Nf);
                    const double ang = 2.0 * M_PI * (double)(((int64_t)k * n) % Nf) / Nf;
                    basis[(size_t)k * Nf + n] = (float)(wn * std::cos(ang));
                    // DC and Nyquist bins are purely real: keep their imaginary rows at exactly +0 so that angle() of a negative
                    // real value is +pi, as torch.stft's rfft returns it (a -0 / 1e-17 there flips the phase to -pi)
                    basis[(size_t)(nbins + k) * Nf + n] = (k == 0 || 2 * k == Nf) ? 0.f : (float)(-wn * std::sin(ang));
                }
            h->stft_basis.N = 2 * nbins; h->stft_basis.C_in = blk; h->stft_basis.ksize = 4;
            b.raw(&h->stft_basis.w, basis);  // [2*nb][4][blk] == [2*nb][n_fft]
        }
        h->stft_ld = pad32(2 * nbins);
        b.conv(&h->enc_embed, "encoder.embed.conv", de, 2 * nbins, 3, true, 1.f, de, h->stft_ld);
        b.norm(&h->enc_norm_w, &h->enc_norm_b, "encoder.norm", de);
        h->enc_cnx.resize(sp.enc_convnext_layers);
        for (int i = 0; i < sp.enc_convnext_layers; ++i) fold_convnext(h->enc_cnx[i], "encoder.prior_net." + std::to_string(i), de, sp.enc_inter);
        build_transformer(b, &h->enc_tr, "encoder.post_net.1", de, sp.enc_layers, de / 64, tr_inter(de));
        b.norm(&h->enc_fnorm_w, &h->enc_fnorm_b, "encoder.final_layer_norm", de);
        b.conv(&h->enc_out20, "encoder.out.conv", sp.code_dim, de, 2 * sp.frame_stride + 1);
    } else {
        // --- SEANet encoder (seanet.py:121-187)
        const std::string em = "encoder.model.";
        b.wn = WN_FOLD;  // every SEANet convolution is weight-normed (seanet.py)
        {   // conv0 (C_in = 1) as [7][n_filters] for launch_conv_in / launch_seanet_front
            std::vector<float> w, w0((size_t)7 * sp.n_filters, 0.f);
            if (b.weight(em + "0.conv.conv", sp.n_filters, 7, &w))
                for (int n = 0; n < sp.n_filters; ++n)
                    for (int j = 0; j < 7; ++j) w0[(size_t)j * sp.n_filters + n] = w[n * 7 + j];
            b.raw(&h->conv0_w, w0);
            b.vec(&h->conv0_b, em + "0.conv.conv.bias", sp.n_filters);
        }
        h->res.resize(sp.n_ratios);
        h->down.resize(sp.n_ratios);
        int C = sp.n_filters;
        for (int i = 0; i < sp.n_ratios; ++i) {
            const std::string rp = em + std::to_string(1 + 3 * i);
            const int hid = C / 2, hp = pad32(hid);
            b.conv(&h->res[i].k3, rp + ".block.1.conv.conv", hid, C, 3, true, 1.f, hp, C);
            b.conv(&h->res[i].pw, rp + ".block.3.conv.conv", C, hid, 1, true, 1.f, C, hp);
            b.conv(&h->res[i].sc, rp + ".shortcut.conv.conv", C, C, 1);
            b.conv(&h->down[i], em + std::to_string(3 + 3 * i) + ".conv.conv", 2 * C, C, 2 * sp.ratios[i]);
            C *= 2;
        }
        QA_REQUIRE(C == sp.dimension, "spec: n_filters * 2^n_ratios = %d != dimension %d", C, sp.dimension);
        build_transformer(b, &h->enc_tr, em + std::to_string(3 * sp.n_ratios + 2), sp.dimension, sp.enc_layers, sp.enc_heads);
        b.conv(&h->enc_out, em + std::to_string(3 * sp.n_ratios + 5) + ".conv.conv", sp.dimension, sp.dimension, 4);
        b.wn = WN_NONE;
        QA_REQUIRE(sp.code_dim == sp.dimension, "spec: code_dim must equal dimension");
    }
    // --- semantic encoder (semantic_module.py:157-201)
    const std::string se = "semantic_encoder.";
    b.conv(&h->sem_in, se + "conv.conv", sp.sem_ch, sp.sem_in, 3, false);
    h->sem_blocks.resize(sp.n_sem_strides);
    for (int i = 0; i < sp.n_sem_strides; ++i) {
        auto& blk = h->sem_blocks[i];
        const std::string bp = se + "conv_blocks." + std::to_string(i);
        for (int u = 0; u < 2; ++u) {
            b.conv(&blk.u1[u], bp + ".res_units." + std::to_string(u) + ".conv1.conv", sp.sem_ch, sp.sem_ch, 3, false);
            b.conv(&blk.u2[u], bp + ".res_units." + std::to_string(u) + ".conv2", sp.sem_ch, sp.sem_ch, 1, false);
        }
        blk.stride = sp.sem_strides[i];
        b.conv(&blk.conv, bp + ".conv.conv", sp.sem_ch, sp.sem_ch, blk.stride == 1 ? 3 : 2 * blk.stride);
    }
    b.conv(&h->sem_out, se + "conv2.conv", sp.code_dim, sp.sem_ch, 3, false);
    // --- codebooks (vector_quantize_pytorch layout: layers.{q}._codebook.embed [1, K, D])
    {
        const int64_t kd = (int64_t)sp.codebook_size * sp.code_dim;
        std::vector<float> cba((size_t)sp.num_quantizers * kd), cbs((size_t)sp.num_quantizers * kd);
        for (int q = 0; q < sp.num_quantizers; ++q) {
            const float* a = b.need("quantizer.layers." + std::to_string(q) + "._codebook.embed", kd);
            const float* s = b.need("semantic_quantizer.layers." + std::to_string(q) + "._codebook.embed", kd);
            if (a) std::memcpy(&cba[(size_t)q * kd], a, sizeof(float) * kd);
            if (s) std::memcpy(&cbs[(size_t)q * kd], s, sizeof(float) * kd);
        }
        b.raw(&h->cb_a, cba);
        b.raw(&h->cb_s, cbs);
    }
    // --- decoder (codec_decoder.py:14-67)
    const int d = sp.dec_dim;
    if (v20) {
        b.conv(&h->dec_embed20, "decoder.embed.conv", d, 2 * sp.code_dim, sp.frame_stride + 1);
    } else {
        b.conv(&h->up, "decoder.embed.up", 2 * d, 2 * sp.code_dim, 1);
        dw_fold_c(&h->up_dw, "decoder.embed.dw.weight", 5, d);
        b.vec(&h->up_dwb, "decoder.embed.dw.bias", d);
    }
    const int ridx[4] = {0, 1, 5, 6};
    for (int i = 0; i < 4; ++i) {
        const std::string rp = "decoder.prior_net." + std::to_string(ridx[i]);
        b.norm(&h->dres[i].n1w, &h->dres[i].n1b, rp + ".norm1", d);
        b.norm(&h->dres[i].n2w, &h->dres[i].n2b, rp + ".norm2", d);
        b.conv(&h->dres[i].c1, rp + ".conv1.conv", d, d, 3);
        b.conv(&h->dres[i].c2, rp + ".conv2.conv", d, d, 3);
    }
    build_transformer(b, &h->dec_tr, "decoder.prior_net.3", d, sp.dec_layers, sp.dec_heads, tr_inter(d));
    b.norm(&h->gn_w, &h->gn_b, "decoder.prior_net.7", d);
    b.norm(&h->norm_w, &h->norm_b, "decoder.norm", d);
    b.norm(&h->fnorm_w, &h->fnorm_b, "decoder.final_layer_norm", d);
    h->cnx.resize(sp.convnext_layers);
    for (int i = 0; i < sp.convnext_layers; ++i) fold_convnext(h->cnx[i], "decoder.post_net." + std::to_string(i), d, sp.dec_inter);
    const int nb = sp.n_fft / 2 + 1;
    b.linear(&h->head, "decoder.head.out.weight", "decoder.head.out.bias", 2 * nb, d);
    // inverse real DFT (norm="backward") with the synthesis window folded in (spectral_ops.py:55-56):
    //   frame[n] = w[n]/N * sum_k c_k (Re_k cos(2 pi k n / N) - Im_k sin(2 pi k n / N)),  c_0 = c_{N/2} = 1, else 2
    {
        const int Nf = sp.n_fft;
        h->spec_ld = pad32(2 * nb);
        std::vector<float> win(Nf);
        if (tab.has("decoder.head.istft.window")) {
            const float* wp = b.need("decoder.head.istft.window", Nf);
            if (wp) std::memcpy(win.data(), wp, sizeof(float) * Nf);
        } else {
            for (int n = 0; n < Nf; ++n) win[n] = (float)(0.5 - 0.5 * std::cos(2.0 * M_PI * n / Nf));
        }
        std::vector<float> basis((size_t)Nf * h->spec_ld, 0.f);
        for (int n = 0; n < Nf; ++n)
            for (int k = 0; k < nb; ++k) {
                const double ck = (k == 0 || k == Nf / 2) ? 1.0 : 2.0;
                const double ang = 2.0 * M_PI * (double)(((int64_t)k * n) % Nf) / Nf;
                basis[(size_t)n * h->spec_ld + k] = (float)(win[n] * ck * std::cos(ang) / Nf);
                basis[(size_t)n * h->spec_ld + nb + k] = (k == 0 || k == Nf / 2) ? 0.f : (float)(-win[n] * ck * std::sin(ang) / Nf);
            }
        h->basis.N = Nf; h->basis.C_in = h->spec_ld; h->basis.ksize = 1;
        b.raw(&h->basis.w, basis);
        b.raw(&h->window, win);
    }
    if (sp.adaptive) {
        QA_REQUIRE(sp.agg_heads > 0 && sp.bt_heads > 0 && sp.code_dim % sp.agg_heads == 0 && (2 * sp.code_dim) % sp.bt_heads == 0,
                   "spec: bad head counts for the adaptive stacks");
        QA_REQUIRE(sp.agg_ff % 32 == 0 && sp.bt_ff % 32 == 0 && sp.max_tokens_per_group >= 1, "spec: bad adaptive widths");
        QA_REQUIRE(sp.agg_context >= 0 && sp.bt_context >= 0, "spec: negative attention context");
        build_mimi(b, &h->agg_sem, "semantic_aggregator.transformer.transformer", sp.code_dim, sp.agg_layers, sp.agg_heads, sp.agg_ff,
                   sp.agg_causal, sp.agg_context);
        build_mimi(b, &h->agg_ac, "acoustic_aggregator.transformer.transformer", sp.code_dim, sp.agg_layers, sp.agg_heads, sp.agg_ff,
                   sp.agg_causal, sp.agg_context);
        build_mimi(b, &h->bottleneck, "bottleneck_transformer.transformer", 2 * sp.code_dim, sp.bt_layers, sp.bt_heads, sp.bt_ff,
                   sp.bt_causal, sp.bt_context);
        b.vec(&h->qemb_sem, "semantic_aggregator.query_embedding", sp.code_dim);
        b.vec(&h->qemb_ac, "acoustic_aggregator.query_embedding", sp.code_dim);
    }
    QA_TRY(b.upload());
    QA_HIP(hipHostMalloc(reinterpret_cast<void**>(&h->host_sync), sizeof(int) * 4));
    QA_HIP(hipStreamCreateWithFlags(&h->side, hipStreamNonBlocking));
    QA_HIP(hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming));
    QA_HIP(hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming));
    // |e|^2 tables
    const int QK = sp.num_quantizers * sp.codebook_size;
    QA_TRY(h->e2_dev.allocate(2 * (size_t)QK));
    QA_TRY(launch_rvq_norms(h->cb_a, h->e2_dev.ptr, QK, sp.code_dim, nullptr));
    QA_TRY(launch_rvq_norms(h->cb_s, h->e2_dev.ptr + QK, QK, sp.code_dim, nullptr));
    QA_HIP(hipDeviceSynchronize());
    h->e2_a = h->e2_dev.ptr;
    h->e2_s = h->e2_dev.ptr + QK;
    return QA_OK;
}

}  // namespace
}  // namespace qa

// plan the call on the handle's workspace, then its real pass
template <typename F>
static int run(Handle* h, void* stream, F&& graph) {
    QA_TRY(plan(h->device, static_cast<hipStream_t>(stream), h->ctx, h->ws, graph));
    return run_graph_checked(h, graph);
}

// ---- what the two stream families share: the streaming H-Codec encoder (qa_hcodec_stream_*) and the codec
// Transformer on its own (qa_transformer_stream_*) are one TrStream each and step through one front.  What differs is named here.
struct StreamFamily {
    const char *unit, *begin, *cap_arg, *reset_rows;  // the words of a message: what an offset counts, the entry points and the argument it points to
    int first_min, unit_samples;            // the fewest units of a first chunk (1: none), and the samples of a unit for its message
};
static StreamFamily codec_stream(const qa_hcodec* h) {
    return {"code frames", "qa_hcodec_stream_begin", "max_frames", "qa_hcodec_stream_reset_rows", h->strm ? h->strm->first_min : 1, h->geom.samples};
}
constexpr StreamFamily TRANSFORMER_STREAM = {"frames", "qa_transformer_stream_begin", "capacity", "qa_transformer_stream_reset_rows", 1, 0};

// the stream of a handle, null when it is not streaming (or null itself); of a const Transformer handle, a const stream
static TrStream* stream_of(const qa_hcodec* h) { return h && h->strm ? &h->strm->tr : nullptr; }
template <typename H> static auto stream_of(H* h) -> decltype(&h->st) { return h && h->st.B > 0 ? &h->st : nullptr; }

static int require_streaming(const char* fn, const TrStream* st, const char* begin) {
    QA_REQUIRE(st, "%s: not streaming (call %s first)", fn, begin);
    return QA_OK;
}

// _begin_ring of both: max_chunk units of `rate` Transformer frames under the window left_context
static int ring_begin_check(const char* fn, const char* chunk_name, const char* unit, int64_t B, int left_context, int64_t max_chunk,
                            int first_min, int rate) {
    QA_REQUIRE(B > 0 && B < (1 << 20) && max_chunk >= first_min && max_chunk <= MAX_POS / rate, "%s: batch %lld, %s %lld (%s, %d .. %d%s)", fn,
               (long long)B, chunk_name, (long long)max_chunk, unit, first_min, MAX_POS / rate, first_min > 1 ? ": a first chunk needs that many" : "");
    const int64_t rows = ring::capacity(left_context, rate * max_chunk);
    QA_REQUIRE(rows <= MAX_POS, "%s: left_context %d with %s %lld needs a ring of %lld rows, above the %d a cache may have", fn, left_context,
               chunk_name, (long long)max_chunk, (long long)rows, MAX_POS);
    return QA_OK;
}

// _reset: every row takes a first step next.  Host state alone (TrStream::off)
static int stream_reset(const char* fn, TrStream* st, const char* begin) {
    QA_TRY(require_streaming(fn, st, begin));
    std::fill(st->off.begin(), st->off.end(), 0);
    return QA_OK;
}

// _reset_rows: the named rows back to offset 0; an index out of range or named twice is refused and nothing changes
static int stream_reset_rows(const char* fn, TrStream* st, const char* begin, const int64_t* rows, int64_t n_rows) {
    QA_TRY(require_streaming(fn, st, begin));
    const int64_t B = st->B;
    QA_REQUIRE(rows && n_rows >= 1 && n_rows <= B, "%s: %lld rows to reset of a stream of %lld (1 .. %lld distinct row indices)", fn,
               (long long)n_rows, (long long)B, (long long)B);
    std::vector<char> seen((size_t)B, 0);
    for (int64_t i = 0; i < n_rows; ++i) {
        QA_REQUIRE(rows[i] >= 0 && rows[i] < B, "%s: rows[%lld] = %lld is outside 0 .. %lld, the rows of this stream", fn, (long long)i,
                   (long long)rows[i], (long long)B - 1);
        QA_REQUIRE(!seen[(size_t)rows[i]], "%s: row %lld is named twice - name every row to reset once", fn, (long long)rows[i]);
        seen[(size_t)rows[i]] = 1;
    }
    for (int64_t i = 0; i < n_rows; ++i) st->off[(size_t)rows[i]] = 0;
    return QA_OK;
}

// _offsets: out [B]
static int stream_offsets(const char* fn, const TrStream* st, const char* begin, int64_t* out) {
    QA_TRY(require_streaming(fn, st, begin));
    QA_REQUIRE(out, "%s: null out", fn);
    for (size_t b = 0; b < st->off.size(); ++b) out[b] = st->off[b];
    return QA_OK;
}

// the long-chunk attention has its per-item form without a window only (attention.hip, section 34), and nothing else runs in its place: a
// step of n Transformer frames x B rows with per-row lengths under a window is refused unless it takes the short kernel
static int rows_under_window_check(const char* fn, int left_context, int B, int64_t n) {
    if (n <= ATTN_SHORT_MAX_Q && tr_short_chunk(B, (int)n)) return QA_OK;
    const long long mode = knob(K_TR_SHORT_ATTN);
    const char* why = n > ATTN_SHORT_MAX_Q ? "this step has more frames" : mode == 0 ? "QA_TR_SHORT_ATTN = 0 turns that kernel off"
                                                                                    : "QA_TR_SHORT_ATTN = 1 stops at 256 query rows";
    set_error("%s: a step with per-row lengths under a sliding window (left_context = %d) runs on the short-chunk attention alone (at "
              "most %d frames per step) and %s; this step has %lld frames x %d rows - step fewer frames, set QA_TR_SHORT_ATTN = 2, or "
              "move the rows together", fn, left_context, ATTN_SHORT_MAX_Q, why, (long long)n, B);
    return QA_ERR_UNSUPPORTED;
}

// the message of a step that plan_step refused (st.plan.row: the offending row); n and frames as the caller passed them
static int step_refuse(const char* fn, const TrStream& st, const StreamFamily& fam, StepFault fault, const int64_t* frames, int64_t n) {
    const long long row = st.plan.row, at = row >= 0 ? st.off[(size_t)row] : 0, take = row >= 0 && frames ? frames[row] : n;
    const int cap = st.cap_units(), fmin = fam.first_min;
    const char* all = st.plan.together ? " (and every row with it: they move together)" : "";
    switch (fault) {
    case STEP_COUNT_RANGE:
        set_error("%s: frames[%lld] = %lld is outside 0 .. %lld, the %s of this step's rectangle (0: the row idles) - pass a wider rectangle "
                  "or fewer frames", fn, row, take, (long long)n, fam.unit);
        break;
    case STEP_RING_CHUNK:
        set_error("%s: row %lld takes %lld %s in this step, above the max_chunk %d this ring stream was begun for (a ring of %d rows holds "
                  "no longer chunk under its window of %d) - step fewer frames or begin the stream with a larger max_chunk", fn, row, take,
                  fam.unit, st.max_chunk / st.rate, st.cap, st.window);
        break;
    case STEP_RING_POSITIONS:
        set_error("%s: row %lld has %lld streamed + %lld new %s, which passes 2^24 = %lld Transformer positions, the last a float holds "
                  "exactly - reset that row", fn, row, at, take, fam.unit, (long long)ring::MAX_POSITIONS);
        break;
    case STEP_FIRST_SHORT:
        set_error("%s: row %lld%s starts its stream with %lld %s, a first chunk needs at least %d (%d samples): its left padding is the "
                  "reflection of its own frames, which a shorter chunk cannot fill the way the offline encoder does - buffer %d frames "
                  "first (among rows that run, let this one idle meanwhile: frames = 0)", fn, row, all, take, fam.unit, fmin,
                  fmin * fam.unit_samples, fmin);
        break;
    case STEP_OVER_CAPACITY:
        set_error("%s: row %lld%s has %lld streamed + %lld new %s, beyond the capacity %d of this stream (%s of %s, at most %d); "
                  "reset that row (%s) or begin a longer stream", fn, row, all, at, take, fam.unit, cap, fam.cap_arg, fam.begin, MAX_POS / st.rate,
                  fam.reset_rows);
        break;
    default:
        set_error("%s: every row idles (frames all 0) - a step needs at least one row with frames; skip the call instead", fn);
    }
    return QA_ERR_INVALID;
}

// One step of a stream: n units per row, or frames[b] of them (frames null: all n).  Every refusal comes before any launch and leaves the
// state and all offsets as they were.  When every row sits at one offset and takes all n the step is the rectangular one - no row arrays,
// (h, c) zeroed here if the rows start - whichever entry point it came through (section 45); otherwise the plan's four vectors go to the
// device and st.rows is set around the graph.  left_context: the window the attention runs under; misaligned: null, or what a step with
// per-row lengths needs 16-byte aligned and is not; run(): the family's graph, which reads `st`.  The offsets advance behind run() alone.
// In order: the plan, the window and alignment rules of row arrays, the capture rule, then the device, the state, the run.
template <typename Run>
static int stream_step(const char* fn, const Handle& h, TrStream& st, const StreamFamily& fam, int left_context, const int64_t* frames,
                       int64_t n, const char* misaligned, hipStream_t s, Run&& run) {
    StepPlan& p = st.plan;
    const StepFault fault = plan_step(st.view(fam.first_min), frames, n, &p);
    if (fault != STEP_OK) return step_refuse(fn, st, fam, fault, frames, n);
    const bool rows = !p.together;
    if (rows && left_context > 0) QA_TRY(rows_under_window_check(fn, left_context, st.B, st.rate * n));
    QA_REQUIRE(!rows || !misaligned, "%s: %s", fn, misaligned);
    QA_TRY(refuse_capture(fn, s, rows ? LENGTHS_ARE_HOST_DATA : CACHE_IS_HOST_STATE));
    QA_HIP(hipSetDevice(h.device));
    if (rows) QA_TRY(st.ints.upload({&p.cnt, &p.first, &p.pos0, &p.nq}, s, st.dev));
    else if (st.offset() == 0) QA_TRY(st.zero_lstm(s));
    st.rows = rows;
    const int rc = run();
    st.rows = false;
    QA_TRY(rc);
    for (size_t b = 0; b < st.off.size(); ++b) st.off[b] += p.cnt[b];
    return QA_OK;
}

extern "C" {

int qa_hcodec_create(qa_hcodec** out, const qa_hcodec_spec* spec, const qa_tensor* tensors, int64_t n_tensors, int device) {
    QA_REQUIRE(out && spec && tensors, "qa_hcodec_create: null argument");
    *out = nullptr;
    QA_HIP(hipSetDevice(device));
    std::unique_ptr<qa_hcodec> h(new qa_hcodec());
    h->spec = *spec;
    h->device = device;
    QA_TRY(build(h.get(), HostTable(tensors, n_tensors)));
    *out = h.release();
    return QA_OK;
}

void qa_hcodec_destroy(qa_hcodec* h) { destroy_handle(h); }

// ---- what the entry points share, all of it before anything is launched.  `fn` is the entry point the caller called; every message
// names it and the offending values.

// The front of every entry point that takes a waveform [B, T]: a whole number of code frames, few enough samples for 32-bit row indices.
// Returns the code-frame count, or the (negative) status.
static int64_t wav_code_frames(const qa_hcodec* h, const char* fn, int64_t B, int64_t T) {
    const int hop = h->geom.samples;
    QA_REQUIRE(B > 0 && T > 0 && T % hop == 0, "%s: wav is [%lld, %lld]; T must be a positive multiple of %d (HCodecTokenizer.pad_wav)", fn,
               (long long)B, (long long)T, hop);
    QA_REQUIRE(B * T < (1LL << 31), "%s: batch of %lld x %lld samples is too large", fn, (long long)B, (long long)T);
    return T / hop;
}

// the plain entry points serve H-Codec 1.0 / 2.0, their _adaptive twins H-Codec 1.5
static int family_check(const qa_hcodec* h, const char* fn, bool adaptive) {
    QA_REQUIRE(!adaptive || h->spec.adaptive, "%s: this handle is not an H-Codec 1.5 model", fn);
    QA_REQUIRE(adaptive || !h->spec.adaptive, "%s: this handle is an H-Codec 1.5 model, use %s_adaptive", fn, fn);
    return QA_OK;
}

// the axis of B clips of T frames at `rate` frames per code frame; lens: the clips' code-frame counts (device) of a ragged call, or null
static TimeAxis clip_axis(const qa_hcodec* h, int64_t B, int64_t T, int rate, const int* lens) {
    return TimeAxis{(int)B, (int)T, h->spec.causal != 0, ClipLens{lens, lens ? rate : 0}};
}

// ragged_refuse: the models that qa_hcodec_encode_ragged / _decode_ragged do not serve.  H-Codec 1.5 has per-clip entry points of its own
// (qa_hcodec_encode_adaptive_ragged / _decode_adaptive_ragged): its codes are [B, Q, G] with a group count the call
// reports, which the 1.0 signatures cannot carry.  ragged_lengths: the lengths themselves (HOST memory, code frames, 1 .. N each;
// the error names the row).  *lens = nullptr when every clip has N frames and the caller does not ask for the masked path whatever the
// lengths (always_masked): the call is then the rectangular one as it is - fused stage 0, no key mask, nothing uploaded.  Otherwise
// *lens = the handle's device array (h->lens), the lengths on their way to it in stream order in front of the call's kernels.
static int ragged_refuse(qa_hcodec* h, const char* fn) {
    const qa_hcodec_spec& sp = h->spec;
    const char* why = sp.adaptive ? "an H-Codec 1.5 model (spec.adaptive): its per-clip calls are qa_hcodec_encode_adaptive_ragged / "
                                    "qa_hcodec_decode_adaptive_ragged (Codec.encode_ragged / decode_ragged)"
                      : sp.causal ? (sp.version == 20 ? "a causal H-Codec 2.0 model (spec.causal)" : "a causal model (spec.causal)")
                                  : nullptr;
    if (why) {
        set_error("%s: per-clip lengths are implemented for non-causal H-Codec 1.0 / 2.0; this handle is %s", fn, why);
        return QA_ERR_UNSUPPORTED;
    }
    return QA_OK;
}
static int ragged_lengths(qa_hcodec* h, const char* fn, int64_t B, int64_t N, const int64_t* frames, bool always_masked, void* stream,
                          const int** lens) {
    QA_REQUIRE(B > 0 && N > 0 && B < (1 << 20), "%s: %lld clips of %lld code frames", fn, (long long)B, (long long)N);
    std::vector<int> len;
    bool full = true;
    const int64_t bad = check_row_lengths(frames, B, 1, N, &len, &full);
    QA_REQUIRE(bad < 0, "%s: frames[%lld] = %lld is outside 1 .. N = %lld", fn, (long long)bad, (long long)frames[bad], (long long)N);
    *lens = nullptr;
    if (full && !always_masked) return QA_OK;
    QA_HIP(hipSetDevice(h->device));
    return h->lens.upload({&len}, static_cast<hipStream_t>(stream), lens);
}

// qa_hcodec_encode (frames == nullptr) and qa_hcodec_encode_ragged
static int encode_call(qa_hcodec* h, const char* fn, const float* wav, int64_t B, int64_t T, const int64_t* frames, const FeatView& f,
                       int64_t* ac, int64_t* sc, void* stream) {
    if (frames) QA_TRY(ragged_refuse(h, fn));
    const int64_t N = wav_code_frames(h, fn, B, T);
    if (N < 0) return (int)N;
    QA_TRY(family_check(h, fn, false));
    const int* lens = nullptr;
    if (frames) {
        QA_REQUIRE(f.n == N * h->geom.feat, "%s: feat has %lld frames, %lld code frames need %lld", fn, (long long)f.n, (long long)N,
                   (long long)(N * h->geom.feat));
        QA_TRY(ragged_lengths(h, fn, B, N, frames, false, stream, &lens));
    }
    const TimeAxis tw = clip_axis(h, B, T, h->geom.samples, lens);
    return run(h, stream, [&] { return encode_graph(h, h->ctx, wav, tw, f, (long long*)ac, (long long*)sc); });
}

// qa_hcodec_decode (frames == nullptr) and qa_hcodec_decode_ragged
static int decode_call(qa_hcodec* h, const char* fn, const int64_t* ac, const int64_t* sc, int64_t B, int64_t N, const int64_t* frames,
                       float* wav_out, void* stream) {
    if (frames) QA_TRY(ragged_refuse(h, fn));
    QA_REQUIRE(B > 0 && N > 0, "%s: codes are [%lld, Q, %lld]", fn, (long long)B, (long long)N);
    QA_REQUIRE(B * N * h->geom.dec * (int64_t)h->spec.hop < (1LL << 31), "%s: output too large for codes [%lld, Q, %lld]", fn, (long long)B,
               (long long)N);
    QA_TRY(family_check(h, fn, false));
    const int* lens = nullptr;
    if (frames) QA_TRY(ragged_lengths(h, fn, B, N, frames, false, stream, &lens));
    const TimeAxis tc = clip_axis(h, B, N, 1, lens);
    return run(h, stream, [&] { return decode_graph(h, h->ctx, (const long long*)ac, (const long long*)sc, tc, wav_out); });
}

int qa_hcodec_encode(qa_hcodec* h, const float* wav, int64_t B, int64_t T, const float* feat, int64_t fsb, int64_t fsc,
                     int64_t fst, int64_t n_feat, int64_t* ac, int64_t* sc, void* stream) {
    QA_REQUIRE(h && wav && feat && ac && sc, "qa_hcodec_encode: null argument");
    return encode_call(h, "qa_hcodec_encode", wav, B, T, nullptr, FeatView{feat, fsb, fsc, fst, (int)n_feat}, ac, sc, stream);
}

int qa_hcodec_encode_ragged(qa_hcodec* h, const float* wav, int64_t B, int64_t T, const int64_t* frames, const float* feat, int64_t fsb,
                            int64_t fsc, int64_t fst, int64_t n_feat, int64_t* ac, int64_t* sc, void* stream) {
    QA_REQUIRE(h && wav && frames && feat && ac && sc, "qa_hcodec_encode_ragged: null argument");
    return encode_call(h, "qa_hcodec_encode_ragged", wav, B, T, frames, FeatView{feat, fsb, fsc, fst, (int)n_feat}, ac, sc, stream);
}

int qa_hcodec_decode(qa_hcodec* h, const int64_t* ac, const int64_t* sc, int64_t B, int64_t N, float* wav_out, void* stream) {
    QA_REQUIRE(h && ac && sc && wav_out, "qa_hcodec_decode: null argument");
    return decode_call(h, "qa_hcodec_decode", ac, sc, B, N, nullptr, wav_out, stream);
}

int qa_hcodec_decode_ragged(qa_hcodec* h, const int64_t* ac, const int64_t* sc, int64_t B, int64_t N, const int64_t* frames, float* wav_out,
                            void* stream) {
    QA_REQUIRE(h && ac && sc && frames && wav_out, "qa_hcodec_decode_ragged: null argument");
    return decode_call(h, "qa_hcodec_decode_ragged", ac, sc, B, N, frames, wav_out, stream);
}

/* ---- the causal H-Codec 1.0 acoustic encoder as a stream ---------------------------------------------- */

int qa_hcodec_stream_geometry(const qa_hcodec_spec* spec, int64_t* samples_per_frame, int64_t* first_min_frames, int32_t* ctx, int32_t cap,
                              int32_t* n_ctx) {
    QA_REQUIRE(spec, "qa_hcodec_stream_geometry: null spec");
    QA_TRY(stream_refuse(*spec, "qa_hcodec_stream_geometry"));
    const StreamGeom g = stream_geometry(*spec);
    if (samples_per_frame) *samples_per_frame = g.samples;
    if (first_min_frames) *first_min_frames = g.first_min;
    if (n_ctx) *n_ctx = (int32_t)g.ctx.size();
    if (ctx) {
        QA_REQUIRE(cap >= (int32_t)g.ctx.size(), "qa_hcodec_stream_geometry: ctx holds %d entries, the encoder has %zu stateful convolutions",
                   cap, g.ctx.size());
        for (size_t i = 0; i < g.ctx.size(); ++i) ctx[i] = g.ctx[i];
    }
    return QA_OK;
}

// left_context > 0: a ring stream for chunks of up to max_frames code frames under that window; else a linear one
// of max_frames code frames.  The arguments are checked by the two entry points
static int hcodec_stream_begin(qa_hcodec* h, const StreamGeom& g, int64_t B, int64_t max_frames, int left_context) {
    QA_HIP(hipSetDevice(h->device));
    h->strm.reset();  // a handle that is already streaming: its buffers wait for the steps that still read them
    std::unique_ptr<CodecStream> st(new CodecStream());
    // the convolutions' states: two buffers [B, ctx, C] each, 64-float aligned, one allocation
    st->convs.resize(g.ctx.size());
    size_t total = 0;
    int C = h->spec.n_filters;
    for (size_t i = 0; i < g.ctx.size(); ++i) {
        StreamConv& sc = st->convs[i];
        sc.ctx = g.ctx[i];
        sc.C = i == 0 ? 1 : C;
        if (i >= 2 && i % 2 == 0) C *= 2;  // behind a down conv (convs 2, 4, ...) the ladder doubles
        if (i + 1 == g.ctx.size()) sc.C = h->spec.dimension;
        total += 2 * (size_t)round_up((int64_t)B * sc.ctx * sc.C, 64);
    }
    QA_TRY(st->conv_mem.allocate(total));
    float* p = st->conv_mem.ptr;
    for (StreamConv& sc : st->convs)
        for (int k = 0; k < 2; ++k) {
            sc.st[k] = p;
            p += round_up((int64_t)B * sc.ctx * sc.C, 64);
        }
    // offsets in code frames, two Transformer frames each; the capacity of a linear stream is max_frames of them
    if (left_context > 0) QA_TRY(st->tr.begin_ring(h->enc_tr, B, left_context, 2 * max_frames, 2));
    else QA_TRY(st->tr.begin(h->enc_tr, B, 2 * max_frames, 2));
    st->first_min = g.first_min;
    h->strm = std::move(st);
    return QA_OK;
}

int qa_hcodec_stream_begin(qa_hcodec* h, int64_t B, int64_t max_frames) {
    QA_REQUIRE(h, "qa_hcodec_stream_begin: null handle");
    QA_TRY(stream_refuse(h->spec, "qa_hcodec_stream_begin"));
    const StreamGeom g = stream_geometry(h->spec);
    QA_REQUIRE(B > 0 && B < (1 << 20) && max_frames >= g.first_min && max_frames <= MAX_POS / 2,
               "qa_hcodec_stream_begin: batch %lld, max_frames %lld (code frames, %d .. %d: the Transformer holds %d positions at 2 per code "
               "frame, and the first chunk alone needs %d)", (long long)B, (long long)max_frames, g.first_min, MAX_POS / 2, MAX_POS, g.first_min);
    return hcodec_stream_begin(h, g, B, max_frames, 0);
}

// The stream under a sliding window of left_context Transformer frames (two per code frame), as a ring without an end.  This is NOT the
// shipped full-causal encoder: it is the SEANet encoder whose Transformer was built with use_sliding_window=True, left_context=W
int qa_hcodec_stream_begin_ring(qa_hcodec* h, int64_t B, int32_t left_context, int64_t max_chunk_frames) {
    QA_REQUIRE(h, "qa_hcodec_stream_begin_ring: null handle");
    QA_TRY(stream_refuse(h->spec, "qa_hcodec_stream_begin_ring"));
    const StreamGeom g = stream_geometry(h->spec);
    QA_REQUIRE(left_context > 0, "qa_hcodec_stream_begin_ring: left_context %d - a ring needs a sliding window of at least 1 Transformer frame "
               "(without a window a query sees its whole history, which no ring holds; qa_hcodec_stream_begin is the full-causal stream)",
               (int)left_context);
    QA_TRY(ring_begin_check("qa_hcodec_stream_begin_ring", "max_chunk_frames", "code frames", B, left_context, max_chunk_frames, g.first_min, 2));
    return hcodec_stream_begin(h, g, B, max_chunk_frames, left_context);
}

int64_t qa_hcodec_stream_capacity(const qa_hcodec* h) { return stream_of(h) ? stream_of(h)->cap_units() : -1; }

// One step of the stream; frames null: every row takes all n code frames (qa_hcodec_stream_encode).  The codec's own checks, then the
// shared front (stream_step), which reads the convolutions' current buffers and flips them behind a step that ran
static int stream_encode_call(qa_hcodec* h, const char* fn, const float* wav, int64_t n_samples, const int64_t* frames, int64_t* acoustic_codes,
                              float* emb, void* stream) {
    QA_REQUIRE(h, "%s: null handle", fn);
    const StreamFamily fam = codec_stream(h);
    QA_TRY(require_streaming(fn, stream_of(h), fam.begin));
    QA_REQUIRE(wav && (acoustic_codes || emb), "%s: null wav, or neither acoustic_codes nor emb asked for", fn);
    TrStream& st = h->strm->tr;
    const int hop = h->geom.samples;
    QA_REQUIRE(n_samples > 0 && n_samples % hop == 0, "%s: a step of %lld samples; it must be a positive multiple of the "
               "%d samples of a code frame (zero-pad a trailing partial frame, as HCodecTokenizer.pad_wav does)", fn, (long long)n_samples, hop);
    const int64_t n = n_samples / hop;
    QA_REQUIRE(st.B * n_samples < (1LL << 31), "%s: a step of %d x %lld samples is too large", fn, st.B, (long long)n_samples);
    const bool aligned = !emb || ((reinterpret_cast<uintptr_t>(emb) & 15) == 0 && h->spec.code_dim % 4 == 0);
    const char* misaligned = aligned ? nullptr : "emb must be 16-byte aligned (and code_dim a multiple of 4) in a step with per-row lengths: "
                                                 "the rows behind a length are written as float4";
    // under a ring's window alone: a linear stream runs its Transformer without one
    QA_TRY(stream_step(fn, *h, st, fam, st.window, frames, n, misaligned, static_cast<hipStream_t>(stream), [&] {
        return run_planned(*h, stream, [&] { return stream_encode_graph(h, h->ctx, wav, (int)n, (long long*)acoustic_codes, emb); });
    }));
    h->strm->cur ^= 1;
    return QA_OK;
}

int qa_hcodec_stream_encode(qa_hcodec* h, const float* wav, int64_t n_samples, int64_t* acoustic_codes, float* emb, void* stream) {
    return stream_encode_call(h, "qa_hcodec_stream_encode", wav, n_samples, nullptr, acoustic_codes, emb, stream);
}

int qa_hcodec_stream_encode_rows(qa_hcodec* h, const float* wav, int64_t n_samples, const int64_t* frames, int64_t* acoustic_codes, float* emb,
                                 void* stream) {
    QA_REQUIRE(h, "qa_hcodec_stream_encode_rows: null handle");
    QA_REQUIRE(frames, "qa_hcodec_stream_encode_rows: null frames (qa_hcodec_stream_encode is the call without per-row lengths)");
    return stream_encode_call(h, "qa_hcodec_stream_encode_rows", wav, n_samples, frames, acoustic_codes, emb, stream);
}

// a row at offset 0 takes a first step next: reflect fill instead of the convolutions' states, on top of what TrStream::off says
int qa_hcodec_stream_reset(qa_hcodec* h) { return stream_reset("qa_hcodec_stream_reset", stream_of(h), "qa_hcodec_stream_begin"); }

int qa_hcodec_stream_reset_rows(qa_hcodec* h, const int64_t* rows, int64_t n_rows) {
    return stream_reset_rows("qa_hcodec_stream_reset_rows", stream_of(h), "qa_hcodec_stream_begin", rows, n_rows);
}

int qa_hcodec_stream_offsets(const qa_hcodec* h, int64_t* out) {
    return stream_offsets("qa_hcodec_stream_offsets", stream_of(h), "qa_hcodec_stream_begin", out);
}

int qa_hcodec_stream_end(qa_hcodec* h) {
    if (!h || !h->strm) return QA_OK;  // nothing to end: harmless, like free(NULL)
    (void)hipSetDevice(h->device);
    h->strm.reset();
    return QA_OK;
}

int64_t qa_hcodec_stream_offset(const qa_hcodec* h) { return stream_of(h) ? stream_of(h)->offset() : -1; }

// The per-clip H-Codec 1.5 calls serve the non-causal model only: a causal aggregator or bottleneck attends by position, and their
// attention takes no key-padding mask.
static int adaptive_ragged_refuse(qa_hcodec* h, const char* fn) {
    const qa_hcodec_spec& sp = h->spec;
    const char* why = sp.causal ? "a causal model (spec.causal)"
                      : (h->agg_sem.causal || h->agg_ac.causal) ? "causal aggregators (spec.agg_causal)"
                      : h->bottleneck.causal ? "a causal bottleneck transformer (spec.bt_causal)"
                                             : nullptr;
    if (why) {
        set_error("%s: per-clip lengths are implemented for the non-causal H-Codec 1.5; this handle has %s", fn, why);
        return QA_ERR_UNSUPPORTED;
    }
    return QA_OK;
}

// qa_hcodec_encode_adaptive (frames == nullptr) and qa_hcodec_encode_adaptive_ragged.  With lengths the call always takes the masked
// path, also when every length is N: rows may still differ in group count, and a row that is the clip alone is what the caller asked for.
static int encode_adaptive_call(qa_hcodec* h, const char* fn, const float* wav, int64_t B, int64_t T, const int64_t* frames, const FeatView& f,
                                int64_t* ac, int64_t* sc, int64_t* n_groups, float threshold, void* stream) {
    QA_TRY(family_check(h, fn, true));
    if (frames) QA_TRY(adaptive_ragged_refuse(h, fn));
    const int64_t N = wav_code_frames(h, fn, B, T);
    if (N < 0) return (int)N;
    QA_REQUIRE(threshold >= 0.f && threshold <= 1.f, "%s: threshold %g outside [0, 1] (codec_adaptive.py:151)", fn, threshold);
    const float thr = threshold <= 0.f ? h->spec.threshold : threshold;  // codec_adaptive.py:158
    const int* lens = nullptr;
    if (frames) {
        QA_REQUIRE(f.n == N * h->geom.feat, "%s: feat has %lld frames, %lld code frames need %lld", fn, (long long)f.n, (long long)N,
                   (long long)(N * h->geom.feat));
        QA_TRY(ragged_lengths(h, fn, B, N, frames, true, stream, &lens));
    }
    const TimeAxis tw = clip_axis(h, B, T, h->geom.samples, lens);
    int G = 0;
    QA_TRY(run(h, stream, [&] { return encode_adaptive_graph(h, h->ctx, wav, tw, f, (long long*)ac, (long long*)sc, &G, thr); }));
    *n_groups = G;
    return QA_OK;
}

int qa_hcodec_encode_adaptive(qa_hcodec* h, const float* wav, int64_t B, int64_t T, const float* feat, int64_t fsb, int64_t fsc,
                              int64_t fst, int64_t n_feat, int64_t* ac, int64_t* sc, int64_t* n_groups, float threshold, void* stream) {
    const char* fn = "qa_hcodec_encode_adaptive";
    QA_REQUIRE(h && wav && feat && ac && sc && n_groups, "%s: null argument", fn);
    return encode_adaptive_call(h, fn, wav, B, T, nullptr, FeatView{feat, fsb, fsc, fst, (int)n_feat}, ac, sc, n_groups, threshold, stream);
}

int qa_hcodec_encode_adaptive_ragged(qa_hcodec* h, const float* wav, int64_t B, int64_t T, const int64_t* frames, const float* feat,
                                     int64_t fsb, int64_t fsc, int64_t fst, int64_t n_feat, int64_t* ac, int64_t* sc, int64_t* n_groups,
                                     float threshold, void* stream) {
    const char* fn = "qa_hcodec_encode_adaptive_ragged";
    QA_REQUIRE(h && wav && frames && feat && ac && sc && n_groups, "%s: null argument", fn);
    return encode_adaptive_call(h, fn, wav, B, T, frames, FeatView{feat, fsb, fsc, fst, (int)n_feat}, ac, sc, n_groups, threshold, stream);
}

// qa_hcodec_adaptive_frames (the maximum) and qa_hcodec_adaptive_clip_frames (every row's total): one launch, one synchronisation.  The
// per-row totals come back in the same copy as the maximum, through a pageable host buffer (the pinned scalar holds one int).
static int adaptive_frames_call(qa_hcodec* h, const char* fn, const int64_t* semantic_codes, int64_t B, int64_t G, int64_t* max_out,
                                int64_t* rows_out, void* stream) {
    QA_REQUIRE(h->spec.adaptive && B > 0 && G > 0 && B < (1 << 20), "%s: bad argument", fn);
    QA_HIP(hipSetDevice(h->device));
    QA_TRY(h->ws.ensure((size_t)(B + 64) * sizeof(int)));
    Ctx& c = h->ctx;
    c.stream = static_cast<hipStream_t>(stream);
    int* totals = reinterpret_cast<int*>(h->ws.ptr);
    int* tmax = totals + B;
    QA_TRY(launch_adaptive_frames((const long long*)semantic_codes, (int)B, h->spec.num_quantizers, (int)G, h->spec.codebook_size,
                                  totals, tmax, c.stream));
    if (!rows_out) {
        int n = 0;
        QA_TRY(read_scalar(c, h, tmax, &n));
        *max_out = n;
        return QA_OK;
    }
    std::vector<int> host((size_t)B);
    QA_HIP(hipMemcpyAsync(host.data(), totals, sizeof(int) * (size_t)B, hipMemcpyDeviceToHost, c.stream));
    QA_HIP(hipStreamSynchronize(c.stream));  // the one synchronisation qa_hcodec_adaptive_frames makes
    lstm_call_note_sync();
    for (int64_t b = 0; b < B; ++b) rows_out[b] = host[(size_t)b];
    return QA_OK;
}

int qa_hcodec_adaptive_frames(qa_hcodec* h, const int64_t* semantic_codes, int64_t B, int64_t G, int64_t* frames, void* stream) {
    QA_REQUIRE(h && semantic_codes && frames, "qa_hcodec_adaptive_frames: null argument");
    return adaptive_frames_call(h, "qa_hcodec_adaptive_frames", semantic_codes, B, G, frames, nullptr, stream);
}

int qa_hcodec_adaptive_clip_frames(qa_hcodec* h, const int64_t* semantic_codes, int64_t B, int64_t G, int64_t* frames_out, void* stream) {
    QA_REQUIRE(h && semantic_codes && frames_out, "qa_hcodec_adaptive_clip_frames: null argument");
    return adaptive_frames_call(h, "qa_hcodec_adaptive_clip_frames", semantic_codes, B, G, nullptr, frames_out, stream);
}

// qa_hcodec_decode_adaptive (frames == nullptr: every clip has N frames) and qa_hcodec_decode_adaptive_ragged
static int decode_adaptive_call(qa_hcodec* h, const char* fn, const int64_t* ac, const int64_t* sc, int64_t B, int64_t G, int64_t N,
                                const int64_t* frames, float* wav_out, void* stream) {
    QA_TRY(family_check(h, fn, true));
    if (frames) QA_TRY(adaptive_ragged_refuse(h, fn));
    QA_REQUIRE(B > 0 && G > 0 && N > 0 && B * N * h->geom.dec * (int64_t)h->spec.hop < (1LL << 31),
               "%s: bad shape: %lld clips, %lld groups, %lld frames", fn, (long long)B, (long long)G, (long long)N);
    const int* lens = nullptr;
    if (frames) QA_TRY(ragged_lengths(h, fn, B, N, frames, true, stream, &lens));
    const TimeAxis tc = clip_axis(h, B, N, 1, lens);
    return run(h, stream, [&] { return decode_adaptive_graph(h, h->ctx, (const long long*)ac, (const long long*)sc, tc, (int)G, wav_out); });
}

int qa_hcodec_decode_adaptive(qa_hcodec* h, const int64_t* ac, const int64_t* sc, int64_t B, int64_t G, int64_t frames,
                              float* wav_out, void* stream) {
    QA_REQUIRE(h && ac && sc && wav_out, "qa_hcodec_decode_adaptive: null argument");
    return decode_adaptive_call(h, "qa_hcodec_decode_adaptive", ac, sc, B, G, frames, nullptr, wav_out, stream);
}

int qa_hcodec_decode_adaptive_ragged(qa_hcodec* h, const int64_t* ac, const int64_t* sc, int64_t B, int64_t G, int64_t N, const int64_t* frames,
                                     float* wav_out, void* stream) {
    QA_REQUIRE(h && ac && sc && frames && wav_out, "qa_hcodec_decode_adaptive_ragged: null argument");
    return decode_adaptive_call(h, "qa_hcodec_decode_adaptive_ragged", ac, sc, B, G, N, frames, wav_out, stream);
}

int qa_hcodec_load_semantic_decoder(qa_hcodec* h, const qa_semantic_decoder_spec* spec, const qa_tensor* tensors, int64_t n_tensors) {
    QA_REQUIRE(h && spec && tensors, "qa_hcodec_load_semantic_decoder: null argument");
    QA_HIP(hipSetDevice(h->device));
    HostTable tab(tensors, n_tensors);
    std::unique_ptr<qa_hcodec::SemDec> sd;
    QA_TRY(build_semantic_decoder(h, *spec, tab, &sd));
    if (h->sdec) QA_HIP(hipDeviceSynchronize());  // the old weights may still be read by an earlier forward
    h->sdec = std::move(sd);
    return QA_OK;
}

int qa_hcodec_has_semantic_decoder(const qa_hcodec* h) {
    if (!h) {
        set_error("qa_hcodec_has_semantic_decoder: null handle");
        return QA_ERR_INVALID;
    }
    return h->sdec ? 1 : 0;
}

// the front of the two forward entry points: forward's own checks (the semantic decoder is attached, pred_feat is small enough for 32-bit
// row indices) around the shared ones; the code-frame count through *n25
static int forward_checks(qa_hcodec* h, const char* fn, const float* wav, int64_t B, int64_t T, const float* feat, const float* recon,
                          const float* pred, bool adaptive, int* n25) {
    QA_REQUIRE(h && wav && feat && recon && pred, "%s: null argument", fn);
    QA_REQUIRE(h->sdec, "%s: no semantic decoder is attached (qa_hcodec_load_semantic_decoder: the checkpoint's semantic_decoder.* "
               "weights)", fn);
    QA_TRY(family_check(h, fn, adaptive));
    const int64_t N = wav_code_frames(h, fn, B, T);
    if (N < 0) return (int)N;
    int64_t up = 1;
    for (int i = 0; i < h->sdec->spec.n_blocks; ++i) up *= h->sdec->spec.strides[i];
    QA_REQUIRE(B * N * up * std::max(h->sdec->spec.output_channels, h->sdec->spec.widths[0]) < (1LL << 31), "%s: pred_feat too large", fn);
    *n25 = (int)N;
    return QA_OK;
}

int qa_hcodec_forward(qa_hcodec* h, const float* wav, int64_t B, int64_t T, const float* feat, int64_t fsb, int64_t fsc, int64_t fst,
                      int64_t n_feat, float* recon, float* pred_feat, void* stream) {
    int N = 0;
    QA_TRY(forward_checks(h, "qa_hcodec_forward", wav, B, T, feat, recon, pred_feat, false, &N));
    const TimeAxis tw = clip_axis(h, B, T, h->geom.samples, nullptr);
    const FeatView f{feat, fsb, fsc, fst, (int)n_feat};
    return run(h, stream, [&] { return forward_graph(h, h->ctx, wav, tw, f, N, recon, pred_feat); });
}

int qa_hcodec_forward_adaptive(qa_hcodec* h, const float* wav, int64_t B, int64_t T, const float* feat, int64_t fsb, int64_t fsc,
                               int64_t fst, int64_t n_feat, float* recon, float* pred_feat, int64_t* token_lengths, int64_t* n_groups,
                               void* stream) {
    int N = 0;
    QA_TRY(forward_checks(h, "qa_hcodec_forward_adaptive", wav, B, T, feat, recon, pred_feat, true, &N));
    QA_REQUIRE(token_lengths && n_groups, "qa_hcodec_forward_adaptive: null argument");
    const TimeAxis tw = clip_axis(h, B, T, h->geom.samples, nullptr);
    const FeatView f{feat, fsb, fsc, fst, (int)n_feat};
    int G = 0;
    QA_TRY(run(h, stream, [&] { return forward_adaptive_graph(h, h->ctx, wav, tw, f, N, recon, pred_feat, (long long*)token_lengths, &G); }));
    *n_groups = G;
    return QA_OK;
}

// diagnostics (tests): regions of all H-Codec calls of the process that ran as two half-batch lanes (QA_BATCH_SPLIT) so far
long long qa_debug_batch_split_regions(void) { return qa::g_split_regions.load(std::memory_order_relaxed); }

int qa_hcodec_enable_taps(qa_hcodec* h, int on) { return taps_enable(h ? &h->ctx : nullptr, "qa_hcodec_enable_taps", on); }

int64_t qa_hcodec_tap(qa_hcodec* h, const char* name, float* dst, int64_t cap, void* stream) {
    return tap_read(h ? &h->ctx : nullptr, "qa_hcodec_tap", name, dst, cap, stream);
}

/* ---- mimi StreamingTransformer ----------------------------------------------------------------------------------------- */

int qa_mimi_create(qa_mimi** out, const qa_mimi_spec* spec, const qa_tensor* tensors, int64_t n_tensors, const char* prefix,
                   int device) {
    QA_REQUIRE(out && spec && tensors && prefix, "qa_mimi_create: null argument");
    *out = nullptr;
    const qa_mimi_spec& sp = *spec;
    QA_REQUIRE(sp.d_model > 0 && sp.num_heads > 0 && sp.d_model % sp.num_heads == 0 && sp.num_layers > 0 && sp.dim_feedforward > 0,
               "qa_mimi_create: bad sizes");
    const int hd = sp.d_model / sp.num_heads;
    QA_REQUIRE(hd == 32 || hd == 64 || hd == 96 || hd == 128, "qa_mimi_create: head_dim %d unsupported (32/64/96/128)", hd);
    QA_REQUIRE(sp.d_model % 32 == 0 && sp.dim_feedforward % 32 == 0, "qa_mimi_create: widths must be multiples of 32");
    QA_REQUIRE(sp.context >= 0 && sp.context <= MAX_POS, "qa_mimi_create: context %d outside [0, %d]", sp.context, MAX_POS);
    QA_HIP(hipSetDevice(device));
    std::unique_ptr<qa_mimi> m(new qa_mimi());
    m->spec = sp;
    m->device = device;
    HostTable tab(tensors, n_tensors);
    Loader b(tab, m->store);
    build_mimi(b, &m->w, prefix, sp.d_model, sp.num_layers, sp.num_heads, sp.dim_feedforward, sp.causal, sp.context);
    QA_TRY(b.upload());
    *out = m.release();
    return QA_OK;
}

void qa_mimi_destroy(qa_mimi* m) { destroy_handle(m); }

static int mimi_run(qa_mimi* m, const float* x, int B, int T, float* y, hipStream_t stream, bool streaming) {
    Ctx& c = m->ctx;
    const int64_t rows = (int64_t)B * T;
    auto graph = [&]() -> int {
        const MimiTemps t = mimi_temps(c, m->w, rows);
        if (c.dry) return QA_OK;  // real-pass-only remainder (the copy and the layers), below the graph's only allocations
        if (y != x) QA_HIP(hipMemcpyAsync(y, x, sizeof(float) * rows * m->w.d, hipMemcpyDeviceToDevice, stream));
        for (size_t l = 0; l < m->w.layers.size(); ++l)
            QA_TRY(mimi_layer(c, m->w, m->w.layers[l], y, t, B, T, nullptr, streaming ? &m->st : nullptr, l));
        return QA_OK;
    };
    return run_planned(*m, stream, graph);
}

int qa_mimi_forward(qa_mimi* m, const float* x, int64_t B, int64_t T, float* y, void* stream) {
    QA_REQUIRE(m && x && y, "qa_mimi_forward: null argument");
    QA_REQUIRE(B > 0 && T > 0 && T <= MAX_POS && B * T < (1LL << 31), "qa_mimi_forward: x is [%lld, %lld, d] (T <= %d)", (long long)B,
               (long long)T, MAX_POS);
    QA_REQUIRE(m->st.B == 0, "qa_mimi_forward: the handle is in streaming mode, use qa_mimi_stream_step");
    return mimi_run(m, x, (int)B, (int)T, y, static_cast<hipStream_t>(stream), false);
}

int qa_mimi_stream_begin(qa_mimi* m, int64_t B) {
    QA_REQUIRE(m, "qa_mimi_stream_begin: null handle");
    QA_REQUIRE(m->spec.causal, "qa_mimi_stream_begin: Streaming only available for causal (mimi/transformer.py:382)");
    QA_REQUIRE(m->spec.context > 0, "qa_mimi_stream_begin: Cannot create a streaming KVCache without a context to estimate capacity "
               "(mimi/transformer.py:349-353)");
    QA_REQUIRE(B > 0 && B < (1 << 20), "qa_mimi_stream_begin: batch %lld", (long long)B);
    QA_HIP(hipSetDevice(m->device));
    const size_t L = m->w.layers.size(), per = (size_t)B * m->spec.context * m->w.d;
    QA_TRY(m->ring.allocate(2 * L * per));  // in place of the ring of a handle that is already streaming
    QA_HIP(hipMemset(m->ring.ptr, 0, sizeof(float) * 2 * L * per));  // RingKVCache.__init__: zeros
    m->st.kc.resize(L);
    m->st.vc.resize(L);
    for (size_t l = 0; l < L; ++l) {
        m->st.kc[l] = m->ring.ptr + (2 * l) * per;
        m->st.vc[l] = m->ring.ptr + (2 * l + 1) * per;
    }
    m->st.B = (int)B;
    m->st.cap = m->spec.context;
    m->st.offset = 0;
    m->st.rope_len = 0;
    return QA_OK;
}

int qa_mimi_stream_step(qa_mimi* m, const float* x, int64_t T, float* y, void* stream) {
    QA_REQUIRE(m && x && y, "qa_mimi_stream_step: null argument");
    QA_REQUIRE(m->st.B > 0, "qa_mimi_stream_step: not streaming (call qa_mimi_stream_begin)");
    QA_REQUIRE(T >= 1 && T <= m->st.cap, "qa_mimi_stream_step: a chunk of %lld frames does not fit the ring of %d (RingKVCache.complete "
               "would write one slot twice)", (long long)T, m->st.cap);
    QA_REQUIRE((int64_t)m->st.offset + T < (1LL << 31), "qa_mimi_stream_step: offset %d + %lld overflows", m->st.offset, (long long)T);
    QA_HIP(hipSetDevice(m->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    // positions beyond the static table (QA_MIMI_ROPE_WINDOW shrinks it, for tests): a rolling window of the same table
    MimiStream& st = m->st;
    const int table = (int)std::min<long long>(MAX_POS, std::max<long long>(st.cap, knob(K_MIMI_ROPE_WINDOW)));
    const long long end = (long long)st.offset + T;
    if (end <= table) {
        st.rope_len = 0;
    } else if (st.rope_len == 0 || st.offset < st.rope_base || end > (long long)st.rope_base + st.rope_len) {
        const int hd = m->w.d / m->w.heads;
        if (!st.rope_win.ptr) QA_TRY(st.rope_win.allocate((size_t)MAX_POS * hd));
        std::vector<float> cs;
        mimi_rope_table(hd, st.offset, table, &cs);
        QA_HIP(hipStreamSynchronize(s));  // earlier steps may still read the old window; `cs` is a stack-lifetime host buffer
        QA_HIP(hipMemcpy(st.rope_win.ptr, cs.data(), sizeof(float) * cs.size(), hipMemcpyHostToDevice));
        st.rope_base = st.offset;
        st.rope_len = table;
    }
    QA_TRY(mimi_run(m, x, m->st.B, (int)T, y, s, true));
    m->st.offset += (int)T;
    return QA_OK;
}

int qa_mimi_stream_reset(qa_mimi* m) {
    QA_REQUIRE(m, "qa_mimi_stream_reset: null handle");
    QA_REQUIRE(m->st.B > 0, "qa_mimi_stream_reset: Trying to reset streaming, but the transformer wasn't streaming (streaming.py:118-121)");
    m->st.offset = 0;  // RingKVCache.reset(): the caches keep their contents, end_offset = 0 alone invalidates them
    m->st.rope_len = 0;
    return QA_OK;
}

int qa_mimi_stream_end(qa_mimi* m) {
    QA_REQUIRE(m, "qa_mimi_stream_end: null handle");
    (void)hipSetDevice(m->device);
    m->ring.release();
    m->st.rope_win.release();
    m->st.kc.clear();
    m->st.vc.clear();
    m->st.B = m->st.cap = m->st.offset = m->st.rope_base = m->st.rope_len = 0;
    return QA_OK;
}

int64_t qa_mimi_stream_offset(const qa_mimi* m) { return (m && m->st.B > 0) ? m->st.offset : -1; }

/* ---- codec Transformer: offline, cache mode, streaming state ------------------------------------------ */

int qa_transformer_create(qa_transformer** out, const qa_transformer_spec* spec, const qa_tensor* tensors, int64_t n_tensors,
                          const char* prefix, int device) {
    QA_REQUIRE(out && spec && tensors && prefix, "qa_transformer_create: null argument");
    *out = nullptr;
    const qa_transformer_spec& sp = *spec;
    QA_REQUIRE(sp.hidden_size > 0 && sp.num_attention_heads > 0 && sp.hidden_size % sp.num_attention_heads == 0 && sp.num_hidden_layers > 0 &&
                   sp.intermediate_size > 0,
               "qa_transformer_create: bad sizes");
    const int hd = sp.hidden_size / sp.num_attention_heads;
    QA_REQUIRE(hd == 64 || hd == 96 || hd == 128, "qa_transformer_create: head_dim %d unsupported (64/96/128)", hd);
    QA_REQUIRE(sp.hidden_size % 128 == 0, "qa_transformer_create: hidden_size %d must be a multiple of 128 (the LSTM recurrence)", sp.hidden_size);
    QA_REQUIRE(sp.intermediate_size % 32 == 0, "qa_transformer_create: intermediate_size %d must be a multiple of 32", sp.intermediate_size);
    QA_REQUIRE(sp.left_context >= 0 && sp.left_context <= MAX_POS, "qa_transformer_create: left_context %d outside [0, %d]", sp.left_context,
               MAX_POS);
    QA_REQUIRE(sp.left_context == 0 || sp.causal, "qa_transformer_create: left_context (use_sliding_window) needs causal");
    QA_HIP(hipSetDevice(device));
    std::unique_ptr<qa_transformer> h(new qa_transformer());
    h->spec = sp;
    h->device = device;
    HostTable tab(tensors, n_tensors);
    Loader b(tab, h->store);
    build_transformer(b, &h->w, prefix, sp.hidden_size, sp.num_hidden_layers, sp.num_attention_heads, sp.intermediate_size);
    QA_TRY(b.upload());
    *out = h.release();
    return QA_OK;
}

void qa_transformer_destroy(qa_transformer* h) { destroy_handle(h); }

static int transformer_check_io(const char* fn, const qa_transformer* h, const float* x, const float* y, int64_t B, int64_t n) {
    QA_REQUIRE(h && x && y, "%s: null argument", fn);
    QA_REQUIRE(x != y, "%s: x and y must be different buffers", fn);
    QA_REQUIRE(B > 0 && n > 0 && n <= MAX_POS && B * n < (1LL << 31), "%s: x is [%lld, %lld, d] (at most %d frames)", fn, (long long)B,
               (long long)n, MAX_POS);
    return QA_OK;
}

// y = the Transformer over x [B, n, d]: the copy on the real pass, then transformer_op in place on y; ch as in transformer_op
static int transformer_run(qa_transformer* h, const float* x, int B, int n, float* y, void* stream, const TrChunk* ch) {
    Ctx& c = h->ctx;
    auto graph = [&]() -> int {
        // per-row lengths: x behind a row's frames is never read (zeros enter instead), and y there is written as exact zeros
        const int* row_nq = ch ? ch->row_nq : nullptr;
        if (row_nq) QA_RUN(c, launch_lm_rows_masked_copy(y, x, B, n, h->w.d, row_nq, c.stream));
        else if (!c.dry) QA_HIP(hipMemcpyAsync(y, x, sizeof(float) * B * n * h->w.d, hipMemcpyDeviceToDevice, c.stream));
        QA_TRY(transformer_op(c, h->w, y, TimeAxis{B, n, h->spec.causal != 0, ClipLens()}, "", h->spec.left_context, ch));
        if (row_nq) QA_RUN(c, launch_lm_rows_zero_pad(y, 0, 1, B, n, h->w.d, row_nq, c.stream));
        return QA_OK;
    };
    // a stream step carries its LSTM state through the per-step kernels alone; every other call's launch_lstm may be the persistent kernel
    // and needs the ticket of run_graph_checked
    return ch && ch->hs ? run_planned(*h, stream, graph) : run(h, stream, graph);
}

int qa_transformer_forward(qa_transformer* h, const float* x, int64_t B, int64_t T, float* y, void* stream) {
    QA_TRY(transformer_check_io("qa_transformer_forward", h, x, y, B, T));
    QA_REQUIRE(h->st.B == 0, "qa_transformer_forward: the handle is in streaming mode, use qa_transformer_stream_step");
    return transformer_run(h, x, (int)B, (int)T, y, stream, nullptr);
}

int qa_transformer_cache_create(qa_transformer* h, int64_t B, int64_t capacity, qa_transformer_cache** out) {
    QA_REQUIRE(h && out, "qa_transformer_cache_create: null argument");
    *out = nullptr;
    QA_REQUIRE(B > 0 && B < (1 << 20) && capacity >= 1 && capacity <= MAX_POS, "qa_transformer_cache_create: batch %lld, capacity %lld (1 .. %d)",
               (long long)B, (long long)capacity, MAX_POS);
    QA_HIP(hipSetDevice(h->device));
    std::unique_ptr<qa_transformer_cache> c(new qa_transformer_cache());
    const size_t L = h->w.layers.size(), per = (size_t)B * capacity * h->w.d;
    // never cleared: no kernel reads a cache row at or behind the key count of its call
    QA_TRY(c->mem.allocate(2 * L * per));
    transformer_kv_views(c->mem.ptr, L, 0, per, &c->kc, &c->vc);
    c->owner = h;
    c->device = h->device;
    c->B = (int)B;
    c->cap = (int)capacity;
    *out = c.release();
    return QA_OK;
}

void qa_transformer_cache_destroy(qa_transformer_cache* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    delete c;  // c->mem waits for the calls that still read it
}

int64_t qa_transformer_cache_length(const qa_transformer_cache* c) { return c ? c->len : -1; }

int qa_transformer_cache_reset(qa_transformer_cache* c) {
    QA_REQUIRE(c, "qa_transformer_cache_reset: null cache");
    c->len = 0;  // the rows stay and become invisible
    return QA_OK;
}

int qa_transformer_forward_cached(qa_transformer* h, qa_transformer_cache* cache, const float* x, int64_t B, int64_t n, float* y,
                                  void* stream) {
    QA_TRY(transformer_check_io("qa_transformer_forward_cached", h, x, y, B, n));
    QA_REQUIRE(cache, "qa_transformer_forward_cached: null cache");
    QA_REQUIRE(cache->owner == h, "qa_transformer_forward_cached: the cache was created for another Transformer");
    QA_REQUIRE(B == cache->B, "qa_transformer_forward_cached: the cache holds %d sequences, x has %lld", cache->B, (long long)B);
    QA_REQUIRE(!(h->spec.causal && cache->len > 0),
               "qa_transformer_forward_cached: a causal Transformer cannot extend a cache that already holds %d frames - the reference builds a "
               "(T, T) mask for the chunk alone and raises against the cached keys (transformer.py:469-475); stream a causal Transformer with "
               "qa_transformer_stream_begin / qa_transformer_stream_step", cache->len);
    QA_REQUIRE((int64_t)cache->len + n <= cache->cap, "qa_transformer_forward_cached: %d cached + %lld new frames exceed the capacity %d",
               cache->len, (long long)n, cache->cap);
    QA_TRY(refuse_capture("qa_transformer_forward_cached", static_cast<hipStream_t>(stream), CACHE_IS_HOST_STATE));
    TrChunk ch;
    ch.kc = cache->kc.data(); ch.vc = cache->vc.data();
    ch.cap = cache->cap; ch.pos0 = cache->len;
    QA_TRY(transformer_run(h, x, (int)B, (int)n, y, stream, &ch));
    cache->len += (int)n;
    return QA_OK;
}

int qa_transformer_stream_begin(qa_transformer* h, int64_t B, int64_t capacity) {
    QA_REQUIRE(h, "qa_transformer_stream_begin: null handle");
    QA_REQUIRE(h->spec.causal, "qa_transformer_stream_begin: streaming needs a causal Transformer (a non-causal query sees frames that have "
               "not arrived yet)");
    QA_REQUIRE(B > 0 && B < (1 << 20) && capacity >= 1 && capacity <= MAX_POS, "qa_transformer_stream_begin: batch %lld, capacity %lld (1 .. %d)",
               (long long)B, (long long)capacity, MAX_POS);
    QA_HIP(hipSetDevice(h->device));
    return h->st.begin(h->w, B, capacity, 1);  // in place of the state of a handle that is already streaming
}

// A ring stream: the K / V rows are rings of ring::capacity(left_context, max_chunk) rows and the stream has no end
int qa_transformer_stream_begin_ring(qa_transformer* h, int64_t B, int64_t max_chunk) {
    QA_REQUIRE(h, "qa_transformer_stream_begin_ring: null handle");
    QA_REQUIRE(h->spec.causal && h->spec.left_context > 0, "qa_transformer_stream_begin_ring: a ring needs a causal Transformer with a sliding "
               "window (causal = %d, left_context = %d): without a window a query sees its whole history, which no ring holds", h->spec.causal,
               h->spec.left_context);
    QA_TRY(ring_begin_check("qa_transformer_stream_begin_ring", "max_chunk", "frames", B, h->spec.left_context, max_chunk, 1, 1));
    QA_HIP(hipSetDevice(h->device));
    return h->st.begin_ring(h->w, B, h->spec.left_context, max_chunk, 1);  // in place of the state of a handle that is already streaming
}

int64_t qa_transformer_stream_capacity(const qa_transformer* h) { return stream_of(h) ? stream_of(h)->cap_units() : -1; }

// One step; frames null: every row takes all n frames (qa_transformer_stream_step).  Its own argument check, then the shared front
static int transformer_stream_call(qa_transformer* h, const char* fn, const float* x, int64_t n, const int64_t* frames, float* y, void* stream) {
    QA_TRY(require_streaming(fn, stream_of(h), TRANSFORMER_STREAM.begin));
    QA_TRY(transformer_check_io(fn, h, x, y, h->st.B, n));
    const bool aligned = (reinterpret_cast<uintptr_t>(x) & 15) == 0 && (reinterpret_cast<uintptr_t>(y) & 15) == 0;
    const char* misaligned = aligned ? nullptr : "x and y must be 16-byte aligned in a step with per-row lengths (the rows behind a length are "
                                                 "written as float4)";
    // under the handle's window, on a linear stream too
    return stream_step(fn, *h, h->st, TRANSFORMER_STREAM, h->spec.left_context, frames, n, misaligned, static_cast<hipStream_t>(stream), [&] {
        const TrChunk ch = stream_chunk(h->st);
        return transformer_run(h, x, h->st.B, (int)n, y, stream, &ch);
    });
}

int qa_transformer_stream_step(qa_transformer* h, const float* x, int64_t n, float* y, void* stream) {
    return transformer_stream_call(h, "qa_transformer_stream_step", x, n, nullptr, y, stream);
}

int qa_transformer_stream_step_rows(qa_transformer* h, const float* x, int64_t n, const int64_t* frames, float* y, void* stream) {
    QA_REQUIRE(h, "qa_transformer_stream_step_rows: null handle");
    QA_REQUIRE(frames, "qa_transformer_stream_step_rows: null frames (qa_transformer_stream_step is the call without per-row lengths)");
    return transformer_stream_call(h, "qa_transformer_stream_step_rows", x, n, frames, y, stream);
}

int qa_transformer_stream_reset(qa_transformer* h) { return stream_reset("qa_transformer_stream_reset", stream_of(h), TRANSFORMER_STREAM.begin); }

int qa_transformer_stream_reset_rows(qa_transformer* h, const int64_t* rows, int64_t n_rows) {
    return stream_reset_rows("qa_transformer_stream_reset_rows", stream_of(h), TRANSFORMER_STREAM.begin, rows, n_rows);
}

int qa_transformer_stream_offsets(const qa_transformer* h, int64_t* out) {
    return stream_offsets("qa_transformer_stream_offsets", stream_of(h), TRANSFORMER_STREAM.begin, out);
}

int qa_transformer_stream_end(qa_transformer* h) {
    QA_REQUIRE(h, "qa_transformer_stream_end: null handle");
    (void)hipSetDevice(h->device);
    h->st.release();
    return QA_OK;
}

int64_t qa_transformer_stream_offset(const qa_transformer* h) { return stream_of(h) ? stream_of(h)->offset() : -1; }

}  // extern "C"
