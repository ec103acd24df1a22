// ssl.cpp - SSL front-end graph behind qa_ssl_*: HuBERT / wav2vec 2.0 feature extraction as HCodecTokenizer uses it
// (QuarkAudio-HCodec/HCodec-1.0/audio_tokenizer.py:35-48; HCodec-1.5/audio_tokenizer.py:53-67).  SURVEY.md 8f-1.
//
// Layout: channel-last [B, frames, C] throughout, so every Conv1d of the feature extractor (k3/k2, stride 2, no padding),
// every Linear and the grouped positional convolution (k128, one implicit GEMM per group over a 48/64-channel slice of the
// same buffer: ldx = ldy = hidden) is a conv_gemm launch with bias / GELU / residual fused; only layer 0 (C_in = 1) and the
// per-channel GroupNorm over time have their own kernel (ssl_kernels.hip).  Attention = the codec's flash kernel over a
// fused QKV buffer (q, k, v projections concatenated at load time).
//
// Per-clip lengths (qa_ssl_forward_ragged): row b of a [B, T] batch behaves as its first lengths[b] samples alone.
// Three layers of the graph see past a clip's end and take its length: layer 0 (the zero padding behind the clip's own last sample, and
// the GroupNorm over time), the "same"-padded positional convolution and the attention (a key-padding mask).  The extractor layers
// 1 .. n_conv-1 are valid convolutions - an output frame below the clip's count reads only input frames below the clip's count - and
// everything else is row-wise.  Frames behind a clip's end are computed from valid samples and zeros, stay finite, and are read by no
// valid frame; the output rows behind the end are written as 0.
#include <cmath>
#include <memory>

#include "host_util.h"
#include "row_lengths.h"

using namespace qa;

namespace {
struct SslLayer {
    ConvW qkv, o, ff1, ff2;
    const float *ln1w = nullptr, *ln1b = nullptr, *ln2w = nullptr, *ln2b = nullptr;
    const float *gate_w = nullptr, *gate_b = nullptr, *gate_c = nullptr;  // WavLM: folded gru_rel_pos_linear [2][hd], [2]; const [H]
};
}  // namespace

struct qa_ssl : Handle {
    qa_ssl_spec spec{};
    // feature extractor
    const float *conv0_w = nullptr, *conv0_b = nullptr, *gn_w = nullptr, *gn_b = nullptr;
    std::vector<ConvW> convs;                      // layers 1..n_conv-1
    std::vector<const float*> cln_w, cln_b;        // "layer" flavour: LayerNorm after every conv (index = layer)
    const float *fp_ln_w = nullptr, *fp_ln_b = nullptr;
    ConvW fp;
    std::vector<ConvW> pos;                        // one per group
    const float *enc_ln_w = nullptr, *enc_ln_b = nullptr;
    const float* relbias = nullptr;  // WavLM: [H][2R+1] relative position bias by clamped distance, R = rel_pos_max_distance
    std::vector<SslLayer> layers;
    std::vector<int> select;
    // ragged calls: the clips' lengths [3][B] - in samples, in layer-0 frames, in output frames - as ONE vector of 3 B ints (one upload, one
    // launch up to B = 85), written on the call's stream
    DeviceInts lens;
};

namespace {

// the lengths of a ragged call at the three stages that read them (device, [B] each); all null: every clip fills its row
struct SslLens {
    const int *samples = nullptr, *l0 = nullptr, *n = nullptr;
};

int64_t frames_of(const qa_ssl_spec& sp, int64_t T) {
    int64_t L = T + 2 * (int64_t)sp.pad;
    for (int i = 0; i < sp.n_conv; ++i) {
        if (L < sp.conv_kernel[i]) return -1;
        L = (L - sp.conv_kernel[i]) / sp.conv_stride[i] + 1;
    }
    return L;
}

int build(qa_ssl* h, const HostTable& tab) {
    const qa_ssl_spec& sp = h->spec;
    QA_REQUIRE(sp.n_conv >= 2 && sp.n_conv <= 8, "ssl spec: n_conv = %d", sp.n_conv);
    const int d = sp.hidden, H = sp.n_heads, I = sp.intermediate;
    QA_REQUIRE(H > 0 && d % H == 0 && (d / H == 32 || d / H == 64 || d / H == 96 || d / H == 128), "ssl spec: head_dim %d unsupported",
               H > 0 ? d / H : 0);
    QA_REQUIRE(d % 32 == 0 && I % 32 == 0, "ssl spec: hidden / intermediate must be multiples of 32");
    QA_REQUIRE(sp.pos_groups > 0 && d % sp.pos_groups == 0 && (d / sp.pos_groups) % 16 == 0 && d / sp.pos_groups > 32,
               "ssl spec: %d channels per positional-conv group unsupported", sp.pos_groups > 0 ? d / sp.pos_groups : 0);
    for (int i = 0; i < sp.n_conv; ++i)
        QA_REQUIRE(sp.conv_dim[i] % 32 == 0 && sp.conv_kernel[i] >= 1 && sp.conv_stride[i] >= 1, "ssl spec: conv layer %d", i);
    QA_REQUIRE(sp.n_select >= 0 && sp.n_select <= 32, "ssl spec: n_select");
    if (sp.n_select == 0)
        for (int i = 0; i <= sp.n_layers; ++i) h->select.push_back(i);
    else
        for (int i = 0; i < sp.n_select; ++i) {
            QA_REQUIRE(sp.select[i] >= 0 && sp.select[i] <= sp.n_layers, "ssl spec: hidden state %d does not exist", sp.select[i]);
            h->select.push_back(sp.select[i]);
        }

    Loader L(tab, h->store);

    // ---- feature extractor
    const int C0 = sp.conv_dim[0], k0 = sp.conv_kernel[0];
    {   // layer 0 (C_in = 1) as [k][C0] for launch_ssl_conv0
        std::vector<float> w, t((size_t)k0 * C0);
        if (L.weight("feature_extractor.conv_layers.0.conv", C0, k0, &w))
            for (int cc = 0; cc < C0; ++cc)
                for (int j = 0; j < k0; ++j) t[(size_t)j * C0 + cc] = w[(size_t)cc * k0 + j];
        L.raw(&h->conv0_w, t);
        if (sp.conv_bias) L.vec(&h->conv0_b, "feature_extractor.conv_layers.0.conv.bias", C0);
    }
    h->cln_w.assign(sp.n_conv, nullptr);
    h->cln_b.assign(sp.n_conv, nullptr);
    if (sp.feat_norm_layer) {
        for (int i = 0; i < sp.n_conv; ++i) {
            L.norm(&h->cln_w[i], &h->cln_b[i], "feature_extractor.conv_layers." + std::to_string(i) + ".layer_norm", sp.conv_dim[i]);
        }
    } else {
        L.norm(&h->gn_w, &h->gn_b, "feature_extractor.conv_layers.0.layer_norm", C0);
    }
    h->convs.resize(sp.n_conv - 1);
    for (int i = 1; i < sp.n_conv; ++i)
        L.conv(&h->convs[i - 1], "feature_extractor.conv_layers." + std::to_string(i) + ".conv", sp.conv_dim[i], sp.conv_dim[i - 1],
               sp.conv_kernel[i], sp.conv_bias != 0);
    const int CL = sp.conv_dim[sp.n_conv - 1];
    // ---- feature projection
    L.norm(&h->fp_ln_w, &h->fp_ln_b, "feature_projection.layer_norm", CL);
    L.conv(&h->fp, "feature_projection.projection", d, CL, 1);
    // ---- positional convolution: weight_norm(dim = 2) folded, then one [cg][k][cg] filter bank per group
    {
        const int G = sp.pos_groups, cg = d / G, k = sp.pos_kernel;
        const std::string pre = "encoder.pos_conv_embed.conv.";
        std::vector<float> wfull((size_t)d * cg * k);
        const int64_t n = (int64_t)d * cg * k;
        const float *g = nullptr, *v = nullptr;
        const bool wn = L.tab.has(pre + "parametrizations.weight.original0") || L.tab.has(pre + "weight_g");
        if (L.tab.has(pre + "parametrizations.weight.original0")) {
            g = L.need(pre + "parametrizations.weight.original0", k);
            v = L.need(pre + "parametrizations.weight.original1", n);
        } else if (wn) {
            g = L.need(pre + "weight_g", k);
            v = L.need(pre + "weight_v", n);
        } else {
            v = L.need(pre + "weight", n);
        }
        const float* bias = L.need(pre + "bias", d);
        h->pos.resize(G);
        if (v && bias && (g || !wn)) {
            std::vector<double> scale(k, 1.0);
            if (g)
                for (int j = 0; j < k; ++j) {  // norm over (out, in) for every kernel position
                    double ss = 0.0;
                    for (int64_t e = 0; e < (int64_t)d * cg; ++e) ss += (double)v[e * k + j] * v[e * k + j];
                    scale[j] = (double)g[j] / std::sqrt(ss);
                }
            for (int gi = 0; gi < G; ++gi) {
                std::vector<float> t((size_t)cg * k * cg);
                for (int o = 0; o < cg; ++o)
                    for (int ci = 0; ci < cg; ++ci)
                        for (int j = 0; j < k; ++j)
                            t[((size_t)o * k + j) * cg + ci] = (float)(v[((size_t)(gi * cg + o) * cg + ci) * k + j] * scale[j]);
                ConvW& w = h->pos[gi];
                w.N = cg; w.C_in = cg; w.ksize = k;
                L.raw(&w.w, t);
                L.raw(&w.b, std::vector<float>(bias + (size_t)gi * cg, bias + (size_t)(gi + 1) * cg));
            }
        }
    }
    L.norm(&h->enc_ln_w, &h->enc_ln_b, "encoder.layer_norm", d);
    // ---- encoder layers
    h->layers.resize(sp.n_layers);
    for (int i = 0; i < sp.n_layers; ++i) {
        SslLayer& Lw = h->layers[i];
        const std::string pre = "encoder.layers." + std::to_string(i) + ".";
        {  // q, k, v projections concatenated -> one [3d, d] GEMM
            std::vector<float> w((size_t)3 * d * d), b((size_t)3 * d);
            const char* nm[3] = {"q_proj", "k_proj", "v_proj"};
            for (int j = 0; j < 3; ++j) {
                const float* ws_ = L.need(pre + "attention." + nm[j] + ".weight", (int64_t)d * d);
                const float* bs_ = L.need(pre + "attention." + nm[j] + ".bias", d);
                if (!ws_ || !bs_) break;
                std::memcpy(w.data() + (size_t)j * d * d, ws_, sizeof(float) * (size_t)d * d);
                std::memcpy(b.data() + (size_t)j * d, bs_, sizeof(float) * d);
            }
            Lw.qkv.N = 3 * d; Lw.qkv.C_in = d; Lw.qkv.ksize = 1;
            L.raw(&Lw.qkv.w, w);
            L.raw(&Lw.qkv.b, b);
        }
        L.conv(&Lw.o, pre + "attention.out_proj", d, d, 1);
        L.norm(&Lw.ln1w, &Lw.ln1b, pre + "layer_norm", d);
        L.conv(&Lw.ff1, pre + "feed_forward.intermediate_dense", I, d, 1);
        L.conv(&Lw.ff2, pre + "feed_forward.output_dense", d, I, 1);
        L.norm(&Lw.ln2w, &Lw.ln2b, pre + "final_layer_norm", d);
        if (sp.rel_pos_buckets > 0) {  // gate = f(sum of 4 outputs): fold rows 0..3 and 4..7 of the 8 x hd projection
            const int hd = d / H;
            const float* gw = L.need(pre + "attention.gru_rel_pos_linear.weight", (int64_t)8 * hd);
            const float* gb = L.need(pre + "attention.gru_rel_pos_linear.bias", 8);
            if (gw && gb) {
                std::vector<float> w2((size_t)2 * hd, 0.f), b2(2, 0.f);
                for (int r = 0; r < 8; ++r) {
                    for (int e = 0; e < hd; ++e) w2[(size_t)(r / 4) * hd + e] += gw[(size_t)r * hd + e];
                    b2[r / 4] += gb[r];
                }
                L.raw(&Lw.gate_w, w2);
                L.raw(&Lw.gate_b, b2);
            }
            L.vec(&Lw.gate_c, pre + "attention.gru_rel_pos_const", H);
        }
    }
    if (sp.rel_pos_buckets > 0) {
        // WavLMAttention.compute_bias / _relative_positions_bucket, tabulated by relative distance r = key - query (float32
        // arithmetic like the reference).  For |r| >= max_distance the bucket is saturated, so clamping r is exact.
        QA_REQUIRE(sp.rel_pos_buckets % 4 == 0 && sp.rel_pos_max_distance > sp.rel_pos_buckets / 4, "ssl spec: relative position buckets");
        const float* emb = L.need("encoder.layers.0.attention.rel_attn_embed.weight", (int64_t)sp.rel_pos_buckets * H);
        if (emb) {
            const int R = sp.rel_pos_max_distance, nb = sp.rel_pos_buckets / 2, max_exact = nb / 2;
            std::vector<float> t((size_t)H * (2 * R + 1));
            const float denom = (float)std::log((double)sp.rel_pos_max_distance / max_exact);
            for (int r = -R; r <= R; ++r) {
                int bucket = r > 0 ? nb : 0;
                const int a = r < 0 ? -r : r;
                if (a < max_exact) {
                    bucket += a;
                } else {
                    float v = std::log((float)a / (float)max_exact);
                    v = v / denom;
                    v = v * (float)(nb - max_exact);
                    long long big = (long long)((float)max_exact + v);
                    if (big > nb - 1) big = nb - 1;
                    bucket += (int)big;
                }
                for (int hh = 0; hh < H; ++hh) t[(size_t)hh * (2 * R + 1) + (r + R)] = emb[(size_t)bucket * H + hh];
            }
            L.raw(&h->relbias, t);
        }
    }
    return L.upload();
}

int forward_graph(qa_ssl* h, Ctx& c, const float* wav, int B, int T, const SslLens& lens, float* feats) {
    const qa_ssl_spec& sp = h->spec;
    const int d = sp.hidden, H = sp.n_heads, hd = d / H, I = sp.intermediate;
    const float eps = sp.layer_norm_eps;
    // ---- feature extractor (HubertFeatureEncoder): conv -> [GroupNorm | LayerNorm] -> GELU
    int L = (int)((T + 2 * (int64_t)sp.pad - sp.conv_kernel[0]) / sp.conv_stride[0] + 1);
    int C = sp.conv_dim[0];
    float* x = c.arena.alloc<float>((size_t)B * L * C);
    {
        const size_t mark = c.arena.mark();
        char* scratch = c.arena.alloc<char>(ssl_conv0_scratch_bytes(B, L, C));
        QA_RUN(c, launch_ssl_conv0(wav, h->conv0_w, h->conv0_b, h->gn_w, h->gn_b, x, scratch, B, T, L, C, sp.conv_kernel[0], sp.conv_stride[0],
                                   sp.pad, sp.feat_norm_layer ? 0 : 1, 1e-5f, sp.feat_norm_layer ? ACT_NONE : ACT_GELU, c.stream, lens.samples, lens.l0));
        c.arena.release(mark);
        if (sp.feat_norm_layer) {
            QA_TRY(layernorm_op(c, x, h->cln_w[0], h->cln_b[0], x, (int64_t)B * L, C, 1e-5f));
            QA_RUN(c, launch_ssl_act(x, (long long)B * L * C, ACT_GELU, c.stream));
        }
    }
    c.tap("ssl.conv0", x, (int64_t)B * L * C);
    for (int i = 1; i < sp.n_conv; ++i) {
        const ConvW& w = h->convs[i - 1];
        const int Lo = (L - w.ksize) / sp.conv_stride[i] + 1;
        QA_REQUIRE(Lo >= 1, "ssl: input too short at conv layer %d", i);
        float* y = c.arena.alloc<float>((size_t)B * Lo * w.N);
        ConvOpt o = conv_geom(sp.conv_stride[i], 0, 0);
        o.act = sp.feat_norm_layer ? ACT_NONE : ACT_GELU;
        QA_TRY(conv_op(c, x, C, B, L, w, y, w.N, Lo, o));
        if (sp.feat_norm_layer) {
            QA_TRY(layernorm_op(c, y, h->cln_w[i], h->cln_b[i], y, (int64_t)B * Lo, w.N, 1e-5f));
            QA_RUN(c, launch_ssl_act(y, (long long)B * Lo * w.N, ACT_GELU, c.stream));
        }
        x = y;
        L = Lo;
        C = w.N;
    }
    c.tap("ssl.extract", x, (int64_t)B * L * C);
    const int N = L;
    const int64_t rows = (int64_t)B * N;
    // ---- feature projection: LayerNorm -> Linear
    float* t0 = c.arena.alloc<float>((size_t)rows * std::max(C, d));
    float* hcur = c.arena.alloc<float>((size_t)rows * d);
    float* hnext = c.arena.alloc<float>((size_t)rows * d);
    float* tmp = c.arena.alloc<float>((size_t)rows * d);
    float* qkv = c.arena.alloc<float>((size_t)rows * 3 * d);
    float* att = c.arena.alloc<float>((size_t)rows * d);
    float* ffu = c.arena.alloc<float>((size_t)rows * I);
    float* acc = c.arena.alloc<float>((size_t)rows * d);
    const bool rel = sp.rel_pos_buckets > 0;
    float* gate = rel ? c.arena.alloc<float>((size_t)rows * H) : nullptr;
    QA_TRY(layernorm_op(c, x, h->fp_ln_w, h->fp_ln_b, t0, rows, C, eps));
    QA_TRY(linear_op(c, t0, rows, h->fp, hcur));
    // ---- encoder front: h = h + GELU(pos_conv(h))  (HubertPositionalConvEmbedding; the even kernel's extra output frame is
    // never computed), then LayerNorm for the post-LN flavour
    {
        const int G = sp.pos_groups, cg = d / G, k = sp.pos_kernel;
        ConvOpt o = conv_geom(1, k / 2, k - 1 - k / 2);
        o.act = ACT_GELU;
        o.ldr = d;
        if (lens.n) o.rl = ClipLens{lens.n, 1};  // zeros behind the clip's own last frame, as the "same" padding of the clip alone
        for (int g = 0; g < G; ++g) {
            o.res = hcur + (size_t)g * cg;
            QA_TRY(conv_op(c, hcur + (size_t)g * cg, d, B, N, h->pos[g], hnext + (size_t)g * cg, d, N, o));
        }
        if (!sp.stable_layer_norm) {
            QA_TRY(layernorm_op(c, hnext, h->enc_ln_w, h->enc_ln_b, hcur, rows, d, eps));
        } else {
            std::swap(hcur, hnext);
        }
    }
    c.tap("ssl.hidden0", hcur, rows * d);
    int n_acc = 0;
    auto maybe_accumulate = [&](int index, const float* hs) -> int {
        for (int sidx : h->select)
            if (sidx == index) {
                QA_RUN(c, launch_ssl_accumulate(acc, hs, (long long)rows * d, n_acc == 0, c.stream));
                ++n_acc;
            }
        return QA_OK;
    };
    QA_TRY(maybe_accumulate(0, hcur));
    AttnArgs at = attn_packed_qkv(qkv, att, B, N, H, hd);
    at.gate = gate;  // WavLM's gated relative position bias (gate is null without it)
    at.relbias = rel ? h->relbias : nullptr;
    at.R = sp.rel_pos_max_distance;
    if (lens.n) {  // the keys behind a clip's end are invisible to its queries
        unsigned char* kvalid = c.arena.alloc<unsigned char>((size_t)rows);
        QA_RUN(c, launch_len_mask(kvalid, B, N, ClipLens{lens.n, 1}, c.stream));
        at.kvalid = kvalid;
    }
    for (int i = 0; i < sp.n_layers; ++i) {
        const SslLayer& Lw = h->layers[i];
        if (!sp.stable_layer_norm) {  // HubertEncoderLayer: x = LN(x + Attn(x)); x = LN(x + FFN(x))
            QA_TRY(linear_op(c, hcur, rows, Lw.qkv, qkv));
            if (rel) QA_RUN(c, launch_ssl_gate(hcur, Lw.gate_w, Lw.gate_b, Lw.gate_c, gate, B, N, H, hd, c.stream));
            QA_TRY(attention_op(c, at));
            QA_TRY(linear_op(c, att, rows, Lw.o, tmp, epi(ACT_NONE, hcur)));
            QA_TRY(layernorm_op(c, tmp, Lw.ln1w, Lw.ln1b, hnext, rows, d, eps));
            QA_TRY(linear_op(c, hnext, rows, Lw.ff1, ffu, epi(ACT_GELU)));
            QA_TRY(linear_op(c, ffu, rows, Lw.ff2, tmp, epi(ACT_NONE, hnext)));
            QA_TRY(layernorm_op(c, tmp, Lw.ln2w, Lw.ln2b, hcur, rows, d, eps));
            QA_TRY(maybe_accumulate(i + 1, hcur));
        } else {  // HubertEncoderLayerStableLayerNorm: x = x + Attn(LN(x)); x = x + FFN(LN(x)); final LN after the last layer
            QA_TRY(layernorm_op(c, hcur, Lw.ln1w, Lw.ln1b, tmp, rows, d, eps));
            QA_TRY(linear_op(c, tmp, rows, Lw.qkv, qkv));
            if (rel) QA_RUN(c, launch_ssl_gate(tmp, Lw.gate_w, Lw.gate_b, Lw.gate_c, gate, B, N, H, hd, c.stream));
            QA_TRY(attention_op(c, at));
            QA_TRY(linear_op(c, att, rows, Lw.o, hcur, epi(ACT_NONE, hcur)));
            QA_TRY(layernorm_op(c, hcur, Lw.ln2w, Lw.ln2b, tmp, rows, d, eps));
            QA_TRY(linear_op(c, tmp, rows, Lw.ff1, ffu, epi(ACT_GELU)));
            QA_TRY(linear_op(c, ffu, rows, Lw.ff2, hcur, epi(ACT_NONE, hcur)));
            if (i == sp.n_layers - 1) {
                QA_TRY(layernorm_op(c, hcur, h->enc_ln_w, h->enc_ln_b, tmp, rows, d, eps));
                QA_TRY(maybe_accumulate(i + 1, tmp));
            } else {
                QA_TRY(maybe_accumulate(i + 1, hcur));
            }
        }
    }
    QA_REQUIRE(n_acc > 0, "ssl: no hidden state selected");
    QA_RUN(c, launch_ssl_compress(acc, feats, (long long)rows * d, 1.0f / (float)n_acc, sp.compress_exponent, c.stream, lens.n, N, d));
    return QA_OK;
}

}  // namespace

extern "C" {

int qa_ssl_create(qa_ssl** out, const qa_ssl_spec* spec, const qa_tensor* tensors, int64_t n_tensors, int device) {
    if (!out || !spec || !tensors) {
        set_error("qa_ssl_create: null argument");
        return QA_ERR_INVALID;
    }
    *out = nullptr;
    QA_HIP(hipSetDevice(device));
    std::unique_ptr<qa_ssl> h(new qa_ssl());
    h->spec = *spec;
    h->device = device;
    QA_TRY(build(h.get(), HostTable(tensors, n_tensors)));
    *out = h.release();
    return QA_OK;
}

void qa_ssl_destroy(qa_ssl* h) { destroy_handle(h); }

int64_t qa_ssl_frames(const qa_ssl* h, int64_t T) {
    if (!h) {
        set_error("qa_ssl_frames: null handle");
        return QA_ERR_INVALID;
    }
    const int64_t n = frames_of(h->spec, T);
    if (n < 1) {
        set_error("qa_ssl_frames: %lld samples are too short for the feature extractor", (long long)T);
        return QA_ERR_INVALID;
    }
    return n;
}

// qa_ssl_forward (lengths == nullptr) and qa_ssl_forward_ragged.  Everything is checked before the first launch; a call whose clips all
// fill their rows is the rectangular call as it is: nothing uploaded, no mask, the same launches.
static int forward_call(qa_ssl* h, const char* fn, const float* wav, int64_t B, int64_t T, const int64_t* lengths, float* feats, void* stream) {
    const qa_ssl_spec& sp = h->spec;
    const int64_t N = frames_of(sp, T);
    QA_REQUIRE(B > 0 && N >= 1, "%s: wav is [%lld, %lld]: too short for the feature extractor", fn, (long long)B, (long long)T);
    const int64_t L0 = (T + 2 * (int64_t)sp.pad - sp.conv_kernel[0]) / sp.conv_stride[0] + 1;
    QA_REQUIRE(B * L0 < (1LL << 31) && L0 * sp.conv_dim[0] < (1LL << 31), "%s: batch of %lld x %lld samples is too large", fn, (long long)B,
               (long long)T);
    SslLens lens;
    int64_t min_len = 1;  // the shortest input that yields one frame
    for (int i = sp.n_conv - 1; i >= 0; --i) min_len = (min_len - 1) * sp.conv_stride[i] + sp.conv_kernel[i];
    min_len = std::max<int64_t>(1, min_len - 2 * (int64_t)sp.pad);
    std::vector<int> v;
    bool full = true;
    const int64_t bad = lengths ? check_row_lengths(lengths, B, min_len, T, &v, &full) : -1;
    if (!full) {
        QA_REQUIRE(B < (1 << 20) && T < (1LL << 31), "%s: %lld clips of %lld samples", fn, (long long)B, (long long)T);
        QA_REQUIRE(bad < 0, "%s: lengths[%lld] = %lld is outside %lld .. T = %lld samples", fn, (long long)bad, (long long)lengths[bad],
                   (long long)min_len, (long long)T);
        // host vectors [3][B]: samples, layer-0 frames (the valid-conv floor rule of the graph), output frames
        v.resize((size_t)3 * B);
        for (int64_t b = 0; b < B; ++b) {
            v[(size_t)(B + b)] = (int)((lengths[b] + 2 * (int64_t)sp.pad - sp.conv_kernel[0]) / sp.conv_stride[0] + 1);
            v[(size_t)(2 * B + b)] = (int)frames_of(sp, lengths[b]);
        }
        const int* dev = nullptr;
        QA_HIP(hipSetDevice(h->device));
        QA_TRY(h->lens.upload({&v}, static_cast<hipStream_t>(stream), &dev));
        lens = SslLens{dev, dev + B, dev + 2 * B};
    }
    return run_planned(*h, stream, [&] { return forward_graph(h, h->ctx, wav, (int)B, (int)T, lens, feats); });
}

int qa_ssl_forward(qa_ssl* h, const float* wav, int64_t B, int64_t T, float* feats, void* stream) {
    if (!h || !wav || !feats) {
        set_error("qa_ssl_forward: null argument");
        return QA_ERR_INVALID;
    }
    return forward_call(h, "qa_ssl_forward", wav, B, T, nullptr, feats, stream);
}

int qa_ssl_forward_ragged(qa_ssl* h, const float* wav, int64_t B, int64_t T, const int64_t* lengths, float* feats, void* stream) {
    if (!h || !wav || !feats) {
        set_error("qa_ssl_forward_ragged: null argument");
        return QA_ERR_INVALID;
    }
    return forward_call(h, "qa_ssl_forward_ragged", wav, B, T, lengths, feats, stream);
}

}  // extern "C"
