// bicodec.cpp - BiCodec.detokenize on the HIP kernels (host orchestration, C-ABI handle): semantic tokens [B, T] + global tokens
// [B, token_num] -> waveform [B, T * prod(rates)], the stage the reference's UniSE test path ends with
// (QuarkAudio-UniSE/model/bicodec/bicodec.py:182-199, called at model/model.py:193,223).  SURVEY.md 8f-2.
// The encoder side (qa_bicodec_enc, further down): BiCodec.tokenize (bicodec.py:151-180) - XLSR-53 features -> Encoder -> factorized
// VQ -> semantic tokens, and reference clip -> mel -> ECAPA-TDNN latent -> PerceiverResampler -> FSQ -> global tokens.
//
//   z_q      FactorizedVectorQuantize.detokenize  (vq/factorized_vector_quantize.py:154-172)  one gather: codebook x out_project folded
//   d_vector SpeakerEncoder.detokenize            (speaker/speaker_encoder.py:111-116)        gather of (FSQ code x project_out) + Linear
//   prenet   Decoder.forward, ratios [1, 1]       (encoder_decoder/feat_decoder.py:79-96)     linears / k7 convs on conv_gemm, AdaLN kernel
//   x += d   bicodec.py:196
//   decoder  WaveGenerator.forward                (encoder_decoder/wave_generator.py:61-91)   every conv on conv_gemm:
//            * ConvTranspose1d(k, stride s, padding (k - s) / 2) as s polyphase stride-1 convolutions of ceil((k - j0) / s) taps that
//              write interleaved rows of the output (row stride s * C_out): no zero-stuffed input, no scatter;
//            * dilated k7 convolutions through the tap table (dilation 1 / 3 / 9);
//            * Snake never costs a pass over HBM: it is the epilogue activation of the producing convolution, and where a tensor is
//              needed both raw (residual skip) and activated (next unit's first conv) the epilogue writes both (ConvParams::y2).
// Layout: channel-last [B, frames, C] everywhere; weights arrive with the reference's state_dict keys (weight_g / weight_v folded here).
#include <memory>

#include "clip_lengths.h"
#include "host_util.h"

using namespace qa;

namespace {

struct VocosLayerW {
    const float *dw = nullptr, *dwb = nullptr, *lnw = nullptr, *lnb = nullptr, *gamma = nullptr;  // lnw == nullptr: AdaLN
    ConvW pw1, pw2;
};
struct VocosW {
    ConvW embed;
    const float *nw = nullptr, *nb = nullptr, *fw = nullptr, *fb = nullptr;
    std::vector<VocosLayerW> layers;
};
struct UnitW {
    const float *a1 = nullptr, *a2 = nullptr;  // Snake alphas in front of the k7 and the k1 convolution
    ConvW c7, c1;
    int dilation = 1;
};
struct GenBlockW {
    const float* a_in = nullptr;    // Snake in front of the ConvTranspose1d
    std::vector<ConvW> phase;       // stride polyphase filters, output phase phi
    std::vector<int> pad_left;      // per phase
    int stride = 1, c_in = 0, c_out = 0;
    UnitW unit[3];
};

}  // namespace

struct qa_bicodec : Handle {
    qa_bicodec_spec spec{};
    int n_glob = 0, hop = 1, n_ada = 0;
    const float *sem_table = nullptr, *glob_table = nullptr;
    ConvW project, ada, linear_pre, linear_out, gen_in, gen_out;
    VocosW down[2], backbone;
    std::vector<GenBlockW> blocks;
    const float* a_final = nullptr;
    // postnet (feat_decoder.Decoder without condition): attached by qa_bicodec_load_forward, read by qa_bicodec_forward only
    struct Postnet {
        WeightStore store;
        qa_bicodec_forward_spec spec{};
        ConvW linear_pre, linear_out;
        VocosW down[2], backbone;
    };
    std::unique_ptr<Postnet> post;
    DeviceInts lens;  // qa_bicodec_detokenize_ragged: the clips' token counts
};

// Conv1dReluBn (ecapa_tdnn.py): the convolution with BN(ReLU(.)) as the epilogue  relu(acc + b) * s + t
struct ConvBnW {
    ConvW conv;
    const float *s = nullptr, *t = nullptr;
};
struct SeRes2W {
    ConvBnW c0, c2;
    const float *res2_w = nullptr, *res2_bst = nullptr;  // [7][3][W][W] (step, tap, in, out) and [7][3][W] (bias, BN scale, BN shift)
    const float *se_w1 = nullptr, *se_b1 = nullptr, *se_w2 = nullptr, *se_b2 = nullptr;
    int dilation = 1;
};
struct PerceiverLayerW {
    ConvW to_q, to_kv, to_out, ff1, ff2;  // ff2's K is zero-padded from the odd GEGLU width to a multiple of 32
};

// BiCodec.get_semantic_tokens (bicodec.py:167-172): Encoder + FactorizedVectorQuantize.tokenize; BiCodec.get_global_tokens
// (bicodec.py:174-178): mel spectrogram + ECAPA-TDNN latent + PerceiverResampler + ResidualFSQ
struct qa_bicodec_enc : Handle {
    qa_bicodec_enc_spec spec{};
    VocosW backbone, down[2];
    ConvW project, in_project;
    const float *codebook = nullptr, *e2 = nullptr;  // F.normalize(codebook) [K, D] and its squared norms
    // global tokens
    int nb = 0, nbp = 0, kp = 0, ff = 0, ffp = 0;  // DFT bins, bins padded to 4, filterbank K padded to 32, GEGLU width and its padding
    ConvW dft, fbank, ecapa_out, proj_context, fsq_in;
    ConvBnW layer1;
    SeRes2W blocks[3];
    std::vector<PerceiverLayerW> perceiver;
    const float *latents = nullptr, *norm_gamma = nullptr;
    // the ECAPA x-vector head (ASTP pooling, BatchNorm1d, Linear): attached by qa_bicodec_load_forward, read by qa_bicodec_forward only
    struct XvecHead {
        WeightStore store;
        // pool.linear1 [128, 3 x 1536] split by its input: the frames (lin1x) and the global context [mean; std] (lin1c, with the bias)
        ConvW lin1x, lin1c, lin2, linear;
        const float *bn_s = nullptr, *bn_t = nullptr;  // BatchNorm1d(3072) in eval as y = v * s + t
    };
    std::unique_ptr<XvecHead> xvec;
    DeviceInts lens{2};  // the _ragged entry points: the clips' feature frames and their samples, whichever the call carries
};

namespace {

// ---------------------------------------------------------------- weight folding (host)

void build_vocos(Loader& L, VocosW* v, const std::string& p, int C, int I, int n_layers, bool ada, float embed_gain, int C_in = 0) {
    L.conv(&v->embed, p + ".embed", C, C_in > 0 ? C_in : C, 7, true, embed_gain);
    if (!ada) {
        L.norm(&v->nw, &v->nb, p + ".norm", C);
    }
    v->layers.resize(n_layers);
    for (int i = 0; i < n_layers; ++i) {
        VocosLayerW& w = v->layers[i];
        const std::string q = p + ".convnext." + std::to_string(i);
        // depthwise filter [C][1][7] -> [7][C]
        const float* dw = L.need(q + ".dwconv.weight", (int64_t)C * 7);
        std::vector<float> kc((size_t)7 * C, 0.f);
        if (dw)
            for (int c = 0; c < C; ++c)
                for (int j = 0; j < 7; ++j) kc[(size_t)j * C + c] = dw[(size_t)c * 7 + j];
        L.raw(&w.dw, kc);
        L.vec(&w.dwb, q + ".dwconv.bias", C);
        if (!ada) L.norm(&w.lnw, &w.lnb, q + ".norm", C);
        L.vec(&w.gamma, q + ".gamma", C);
        L.conv(&w.pw1, q + ".pwconv1", I, C, 1);
        L.conv(&w.pw2, q + ".pwconv2", C, I, 1);
    }
    L.norm(&v->fw, &v->fb, p + ".final_layer_norm", C);
}

int build(qa_bicodec* h, const HostTable& tab) {
    const qa_bicodec_spec& sp = h->spec;
    const int Ld = sp.latent_dim, C = sp.vocos_dim, I = sp.vocos_inter;
    QA_REQUIRE(sp.n_levels >= 1 && sp.n_levels <= 8 && sp.n_rates >= 1 && sp.n_rates <= 8, "bicodec spec: bad level / rate count");
    QA_REQUIRE(Ld % 32 == 0 && C % 32 == 0 && I % 32 == 0 && sp.gen_channels % (32 << sp.n_rates) == 0,
               "bicodec spec: latent %d, vocos %d / %d must be multiples of 32 and gen_channels %d of 32 * 2^n_rates", Ld, C, I, sp.gen_channels);
    QA_REQUIRE((sp.spk_latent_dim * sp.token_num) % 32 == 0 && sp.codebook_dim >= 1 && sp.codebook_size >= 1, "bicodec spec: bad quantizer shape");
    h->n_glob = 1;
    h->hop = 1;
    for (int i = 0; i < sp.n_levels; ++i) h->n_glob *= sp.levels[i];
    for (int i = 0; i < sp.n_rates; ++i) {
        QA_REQUIRE(sp.rates[i] >= 1 && sp.kernel_sizes[i] >= sp.rates[i] && (sp.kernel_sizes[i] - sp.rates[i]) % 2 == 0,
                   "bicodec spec: ConvTranspose1d kernel %d / stride %d: length-exact up-sampling needs k - s even", sp.kernel_sizes[i], sp.rates[i]);
        h->hop *= sp.rates[i];
    }
    Loader L(tab, h->store, WN_DETECT);  // BiCodec mixes weight-normed and plain layers
    // ---- semantic tokens: table[v] = out_project(codebook[v]) + bias   (factorized_vector_quantize.py:154-172; k = 1 conv = Linear)
    {
        std::vector<float> w;
        const float* cb = L.need("quantizer.codebook.weight", (int64_t)sp.codebook_size * sp.codebook_dim);
        const float* b = L.need("quantizer.out_project.bias", Ld);
        std::vector<float> t((size_t)sp.codebook_size * Ld, 0.f);
        if (L.weight("quantizer.out_project", Ld, sp.codebook_dim, &w) && cb && b)
            for (int v = 0; v < sp.codebook_size; ++v)
                for (int n = 0; n < Ld; ++n) {
                    float acc = 0.f;  // fp32 products in k order, then the bias, like the convolution
                    for (int k = 0; k < sp.codebook_dim; ++k) acc = std::fmaf(cb[(size_t)v * sp.codebook_dim + k], w[(size_t)n * sp.codebook_dim + k], acc);
                    t[(size_t)v * Ld + n] = acc + b[n];
                }
        L.raw(&h->sem_table, t);
    }
    // ---- global tokens: table[v] = project_out(fsq_code(v)) + bias   (residual_fsq.py:112-156, finite_scalar_quantization.py:165-183)
    {
        const int Ls = sp.spk_latent_dim, nl = sp.n_levels;
        const float* w = L.need("speaker_encoder.quantizer.project_out.weight", (int64_t)Ls * nl);
        const float* b = L.need("speaker_encoder.quantizer.project_out.bias", Ls);
        std::vector<float> t((size_t)h->n_glob * Ls, 0.f);
        if (w && b)
            for (int v = 0; v < h->n_glob; ++v) {
                float code[8];
                int rem = v;
                for (int d = 0; d < nl; ++d) {  // least-significant digit first: basis = cumprod([1] + levels[:-1])
                    const int digit = rem % sp.levels[d], half = sp.levels[d] / 2;
                    rem /= sp.levels[d];
                    code[d] = (float)(digit - half) / (float)half;
                }
                for (int n = 0; n < Ls; ++n) {
                    float acc = 0.f;
                    for (int d = 0; d < nl; ++d) acc = std::fmaf(code[d], w[(size_t)n * nl + d], acc);
                    t[(size_t)v * Ls + n] = acc + b[n];
                }
            }
        L.raw(&h->glob_table, t);
    }
    L.conv(&h->project, "speaker_encoder.project", Ld, sp.spk_latent_dim * sp.token_num, 1);
    // ---- prenet (feat_decoder.py:48-96).  SamplingBlock with both scales 1 returns 3 x (samper.py:78-95): folded into the embed filters
    L.conv(&h->linear_pre, "prenet.linear_pre", C, Ld, 1);
    for (int i = 0; i < 2; ++i) build_vocos(L, &h->down[i], "prenet.downsample." + std::to_string(i) + ".1", C, I, 2, false, 3.0f);
    build_vocos(L, &h->backbone, "prenet.vocos_backbone", C, I, sp.vocos_layers, true, 1.0f);
    L.conv(&h->linear_out, "prenet.linear", Ld, C, 1);
    // every AdaLayerNorm's scale / shift Linear stacked into one [n_ada * 2 * C, latent] matrix: one GEMV per call
    h->n_ada = sp.vocos_layers + 1;
    {
        std::vector<float> w((size_t)h->n_ada * 2 * C * Ld, 0.f), b((size_t)h->n_ada * 2 * C, 0.f);
        for (int a = 0; a < h->n_ada; ++a) {
            const std::string p = a == 0 ? "prenet.vocos_backbone.norm" : "prenet.vocos_backbone.convnext." + std::to_string(a - 1) + ".norm";
            const char* part[2] = {".scale", ".shift"};
            for (int k = 0; k < 2; ++k) {
                const float* wp = L.need(p + part[k] + ".weight", (int64_t)C * Ld);
                const float* bp = L.need(p + part[k] + ".bias", C);
                if (wp) std::memcpy(&w[((size_t)a * 2 + k) * C * Ld], wp, sizeof(float) * (size_t)C * Ld);
                if (bp) std::memcpy(&b[((size_t)a * 2 + k) * C], bp, sizeof(float) * C);
            }
        }
        h->ada.N = h->n_ada * 2 * C; h->ada.C_in = Ld; h->ada.ksize = 1;
        L.raw(&h->ada.w, w);
        L.raw(&h->ada.b, b);
    }
    // ---- wave generator (wave_generator.py:61-91)
    int ch = sp.gen_channels;
    L.conv(&h->gen_in, "decoder.model.0", ch, Ld, 7);
    h->blocks.resize(sp.n_rates);
    for (int i = 0; i < sp.n_rates; ++i) {
        GenBlockW& g = h->blocks[i];
        const std::string p = "decoder.model." + std::to_string(i + 1) + ".block";
        const int cin = ch, cout = ch / 2, k = sp.kernel_sizes[i], s = sp.rates[i], pad = (k - s) / 2;
        g.stride = s; g.c_in = cin; g.c_out = cout;
        L.vec(&g.a_in, p + ".0.alpha", cin);
        // ConvTranspose1d weight [C_in][C_out][k] (weight_norm over dim 0 = C_in) as s polyphase stride-1 filters (host_util.h)
        std::vector<float> w;
        const bool have = L.weight(p + ".1", cin, (int64_t)cout * k, &w);
        g.phase.resize(s);
        g.pad_left.resize(s);
        for (int phi = 0; phi < s; ++phi) {
            PolyphaseFilter pf;
            QA_TRY(polyphase_filter(have ? w.data() : nullptr, cin, cout, k, s, pad, phi, &pf));
            ConvW& cw = g.phase[phi];
            cw.N = cout; cw.C_in = cin; cw.ksize = pf.ntaps;
            L.raw(&cw.w, pf.filter);
            L.vec(&cw.b, p + ".1.bias", cout);
            g.pad_left[phi] = pf.pad_left;
        }
        const int dil[3] = {1, 3, 9};
        for (int j = 0; j < 3; ++j) {
            UnitW& u = g.unit[j];
            const std::string up = p + "." + std::to_string(j + 2) + ".block";
            u.dilation = dil[j];
            L.vec(&u.a1, up + ".0.alpha", cout);
            L.conv(&u.c7, up + ".1", cout, cout, 7);
            L.vec(&u.a2, up + ".2.alpha", cout);
            L.conv(&u.c1, up + ".3", cout, cout, 1);
        }
        ch = cout;
    }
    L.vec(&h->a_final, "decoder.model." + std::to_string(sp.n_rates + 1) + ".alpha", ch);
    L.conv(&h->gen_out, "decoder.model." + std::to_string(sp.n_rates + 2), 1, ch, 7);
    return L.upload();
}

// ---------------------------------------------------------------- graph helpers
// One row per batch item (d-vector, AdaLN conditions): the weight-streaming skinny GEMM, 32 rows per launch, so that an
// item's arithmetic does not depend on how many items share the call (a row-count rule - skinny up to 32 rows, implicit GEMM above -
// made batches of more than 32 segments differ from smaller ones by 1e-5: found by the pipelined UniSE driver at 64 segments per batch)
int linear_per_item(Ctx& c, const float* x, int64_t rows, const ConvW& w, float* y) {
    if (c.dry) return QA_OK;  // real-pass-only function: it allocates nothing
    if (w.C_in % 256 != 0) return linear_op(c, x, rows, w, y);
    for (int64_t r0 = 0; r0 < rows; r0 += 32) {
        const int n = (int)std::min<int64_t>(32, rows - r0);
        QA_TRY(launch_skinny_gemm(x + r0 * w.C_in, w.C_in, w.w, w.b, nullptr, 0, nullptr, w.N, y + r0 * w.N, w.N, n, w.N, w.C_in, ACT_NONE,
                                  c.stream, 0.f, 0));
    }
    return QA_OK;
}

// VocosBackbone.forward (blocks/vocos.py:323-335) in place on x [B, T, C]; t1 [rows, C], u [rows, I] scratch.
// cond: AdaLN scale / shift rows of this backbone ([B, n_ada * 2 * C], entry a at offset a * 2 * C), or nullptr for plain LayerNorm.
// in: the embed convolution reads [B, T, embed.C_in] from here instead of x (the encoder's 1024 -> 384 input backbone)
// rl: the clips' lengths in frames of a per-clip call - the k7 embed and the depthwise k7 of every layer pad with zeros from a clip's own
// end; LayerNorm, AdaLN and the pointwise linears are row-wise
int vocos(Ctx& c, const VocosW& v, float* x, float* t1, float* u, int B, int T, int C, const float* cond, int64_t ld_cond, ClipLens rl,
          const float* in = nullptr) {
    const int64_t rows = (int64_t)B * T;
    ConvOpt same7;
    same7.pad_left = 3; same7.pad_right = 3; same7.rl = rl;
    QA_TRY(conv_op(c, in ? in : x, in ? v.embed.C_in : C, B, T, v.embed, t1, C, T, same7));
    if (cond) QA_RUN(c, launch_adaln(t1, cond, cond + C, ld_cond, x, B, T, C, 1e-6f, c.stream));
    else QA_TRY(layernorm_op(c, t1, v.nw, v.nb, x, rows, C, 1e-6f));
    for (size_t i = 0; i < v.layers.size(); ++i) {
        const VocosLayerW& w = v.layers[i];
        if (cond) {
            const float* sc = cond + (int64_t)(i + 1) * 2 * C;
            QA_TRY(dwconv_op(c, x, w.dw, w.dwb, nullptr, nullptr, u, B, T, C, 7, 0.f, -1, rl));  // u doubles as [rows, C] scratch
            QA_RUN(c, launch_adaln(u, sc, sc + C, ld_cond, t1, B, T, C, 1e-6f, c.stream));
        } else {
            QA_TRY(dwconv_op(c, x, w.dw, w.dwb, w.lnw, w.lnb, t1, B, T, C, 7, 1e-6f, -1, rl));
        }
        QA_TRY(linear_op(c, t1, rows, w.pw1, u, epi(ACT_GELU)));
        QA_TRY(linear_op(c, u, rows, w.pw2, x, epi(ACT_NONE, x, w.gamma)));
    }
    QA_TRY(layernorm_op(c, x, v.fw, v.fb, t1, rows, C, 1e-6f));
    // real pass only, more than a launch: the normalised rows go back into x
    if (!c.dry) QA_HIP(hipMemcpyAsync(x, t1, sizeof(float) * (size_t)rows * C, hipMemcpyDeviceToDevice, c.stream));
    return QA_OK;
}

// BiCodec.postnet (feat_decoder.py:79-96 without condition) on the prenet output px [B, T, latent] -> pred [B, out_channels, T],
// channel-first like the reference (bicodec.py:135)
int postnet_op(const qa_bicodec::Postnet& p, Ctx& c, const float* px, int B, int T, float* pred) {
    const qa_bicodec_forward_spec& sp = p.spec;
    const int C = sp.postnet_vocos_dim, I = sp.postnet_vocos_inter, O = sp.postnet_out_channels;
    const int64_t rows = (int64_t)B * T;
    float* x = c.arena.alloc<float>(rows * C);
    float* t1 = c.arena.alloc<float>(rows * C);
    float* u = c.arena.alloc<float>(rows * I);
    float* o = c.arena.alloc<float>(rows * O);
    QA_TRY(linear_op(c, px, rows, p.linear_pre, x));
    for (int i = 0; i < 2; ++i) QA_TRY(vocos(c, p.down[i], x, t1, u, B, T, C, nullptr, 0, ClipLens()));
    QA_TRY(vocos(c, p.backbone, x, t1, u, B, T, C, nullptr, 0, ClipLens()));
    QA_TRY(linear_op(c, x, rows, p.linear_out, o, epi(sp.postnet_tanh ? ACT_TANH : ACT_NONE)));
    c.tap("postnet.out", o, rows * O);
    // [B, T, O] read as a [B, C' = T, T' = O] tensor with strides (T O, O, 1): its channel-last form is [B, O, T]
    return to_channel_last_op(c, o, (long long)T * O, O, 1, pred, B, T, O);
}

// pred / dvec_out (forward only, else nullptr): the postnet's output from the prenet output BEFORE the d-vector add (bicodec.py:135-136),
// and a copy of the d-vector.
// rl (per-clip calls; rl.n null: the rectangular call): clip b holds rl.n[b] of the T tokens.  Every filter with a
// temporal footprint sees the clip's length at its own rate - tokens in the prenet, tokens x the strides so far in the wave generator,
// where a dilated k7 pads by up to 27 frames - and pads with zeros from the clip's own end; entries of `sem` behind it are never read
// and wav_out[b] is exactly 0 from sample rl.n[b] * hop on.
int detokenize_graph(qa_bicodec* h, Ctx& c, const long long* sem, const long long* glob, int B, int T, ClipLens rl, float* wav_out,
                     float* pred = nullptr, float* dvec_out = nullptr) {
    const qa_bicodec_spec& sp = h->spec;
    const int Ld = sp.latent_dim, C = sp.vocos_dim, I = sp.vocos_inter;
    const int64_t rows = (int64_t)B * T;
    // ---- tokens -> z_q [B, T, latent], d_vector [B, latent]
    float* zq = c.arena.alloc<float>(rows * Ld);
    float* gflat = c.arena.alloc<float>((size_t)B * sp.spk_latent_dim * sp.token_num);
    float* dvec = c.arena.alloc<float>((size_t)B * Ld);
    float* cond = c.arena.alloc<float>((size_t)B * h->ada.N);
    QA_RUN(c, launch_gather_rows(sem, h->sem_table, zq, rows, sp.codebook_size, Ld, c.stream, T, rl.n));
    QA_RUN(c, launch_gather_global(glob, h->glob_table, gflat, B, sp.token_num, h->n_glob, sp.spk_latent_dim, c.stream));
    QA_TRY(linear_per_item(c, gflat, B, h->project, dvec));
    QA_TRY(linear_per_item(c, dvec, B, h->ada, cond));
    c.tap("z_q", zq, rows * Ld);
    c.tap("d_vector", dvec, (int64_t)B * Ld);
    // ---- prenet
    float* x = c.arena.alloc<float>(rows * C);
    float* t1 = c.arena.alloc<float>(rows * C);
    float* u = c.arena.alloc<float>(rows * I);
    QA_TRY(linear_op(c, zq, rows, h->linear_pre, x));
    for (int i = 0; i < 2; ++i) QA_TRY(vocos(c, h->down[i], x, t1, u, B, T, C, nullptr, 0, rl));
    c.tap("prenet.down", x, rows * C);
    QA_TRY(vocos(c, h->backbone, x, t1, u, B, T, C, cond, h->ada.N, rl));
    c.tap("prenet.backbone", x, rows * C);
    float* px = zq;  // z_q is dead: reuse it for the prenet output [B, T, latent]
    QA_TRY(linear_op(c, x, rows, h->linear_out, px));
    if (pred) {
        const size_t m = c.arena.mark();  // the postnet's buffers are dead once pred is written
        QA_TRY(postnet_op(*h->post, c, px, B, T, pred));
        c.arena.release(m);
    }
    // real pass only, more than a launch: forward's copy of the d-vector
    if (dvec_out && !c.dry) QA_HIP(hipMemcpyAsync(dvec_out, dvec, sizeof(float) * (size_t)B * Ld, hipMemcpyDeviceToDevice, c.stream));
    QA_RUN(c, launch_add_rowvec(px, dvec, B, T, Ld, c.stream));
    c.tap("prenet.out", px, rows * Ld);
    // ---- wave generator
    int ch = sp.gen_channels, Tc = T;
    float* s_in = c.arena.alloc<float>((size_t)B * Tc * ch);  // snake(conv0(x)): the only form block 0 consumes
    {
        ConvOpt o;
        o.pad_left = 3; o.pad_right = 3; o.act = ACT_SNAKE; o.alpha = h->blocks[0].a_in; o.rl = rl;
        QA_TRY(conv_op(c, px, Ld, B, T, h->gen_in, s_in, ch, T, o));
    }
    for (size_t bi = 0; bi < h->blocks.size(); ++bi) {
        const GenBlockW& g = h->blocks[bi];
        const int s = g.stride, co = g.c_out, To = Tc * s;
        const ClipLens rl_in = rl.times(Tc / T), rl_out = rl.times(To / T);  // the clips at the block's input and output rates
        const size_t n = (size_t)B * To * co;
        float* raw0 = c.arena.alloc<float>(n);
        float* raw1 = c.arena.alloc<float>(n);
        float* snk = c.arena.alloc<float>(n);
        float* act = c.arena.alloc<float>(n);
        // ConvTranspose1d: phase phi writes rows q * s + phi (row stride s * co) of the raw tensor and of its Snake (unit 0's alpha)
        for (int phi = 0; phi < s; ++phi) {
            ConvOpt o;
            o.pad_left = g.pad_left[phi];
            o.pad_right = g.phase[phi].ksize - 1 - g.pad_left[phi];
            o.rl = rl_in;
            o.y2 = snk + (size_t)phi * co; o.alpha2 = g.unit[0].a1; o.ldy2 = (int64_t)s * co;
            QA_TRY(conv_op(c, s_in, g.c_in, B, Tc, g.phase[phi], raw0 + (size_t)phi * co, (int64_t)s * co, Tc, o));
        }
        float *cur = raw0, *nxt = raw1;
        const bool last_block = bi + 1 == h->blocks.size();
        const float* a_next_block = last_block ? h->a_final : h->blocks[bi + 1].a_in;
        for (int j = 0; j < 3; ++j) {
            const UnitW& un = g.unit[j];
            ConvOpt o7;  // Snake (input, already applied) -> dilated k7 -> Snake (epilogue)
            o7.pad_left = 3 * un.dilation; o7.pad_right = 3 * un.dilation; o7.dilation = un.dilation;
            o7.act = ACT_SNAKE; o7.alpha = un.a2; o7.rl = rl_out;
            QA_TRY(conv_op(c, snk, co, B, To, un.c7, act, co, To, o7));
            ConvOpt o1;  // k1 + skip; the sum leaves raw (for the next skip) and activated (for the next convolution)
            o1.res = cur; o1.ldr = co;
            if (j < 2) {
                o1.y2 = snk; o1.alpha2 = g.unit[j + 1].a1; o1.ldy2 = co;
                QA_TRY(conv_op(c, act, co, B, To, un.c1, nxt, co, To, o1));
            } else {  // the next consumer (next block's ConvTranspose1d / the output conv) only reads the activated sum
                o1.post_act = ACT_SNAKE; o1.alpha = a_next_block;
                QA_TRY(conv_op(c, act, co, B, To, un.c1, nxt, co, To, o1));
            }
            std::swap(cur, nxt);
        }
        c.tap("gen.block" + std::to_string(bi), cur, (int64_t)n);  // NOTE: the last unit's tensor is stored ACTIVATED (see above)
        s_in = cur;
        ch = co;
        Tc = To;
    }
    {
        ConvOpt o;
        o.pad_left = 3; o.pad_right = 3; o.act = ACT_TANH; o.rl = rl.times(Tc / T);
        QA_TRY(conv_op(c, s_in, ch, B, Tc, h->gen_out, wav_out, 1, Tc, o));
    }
    if (rl.n) QA_RUN(c, launch_zero_behind(wav_out, B, Tc, rl.times(Tc / T), c.stream));  // behind the last writer of the waveform
    return QA_OK;
}

int build_speaker(qa_bicodec_enc* h, Loader& L);

int build_encoder(qa_bicodec_enc* h, const HostTable& tab) {
    const qa_bicodec_enc_spec& sp = h->spec;
    const int Cin = sp.input_channels, C = sp.vocos_dim, I = sp.vocos_inter, Ld = sp.latent_dim, K = sp.codebook_size, D = sp.codebook_dim;
    QA_REQUIRE(Cin % 32 == 0 && C % 32 == 0 && I % 32 == 0 && Ld % 32 == 0 && sp.vocos_layers >= 1,
               "bicodec encoder spec: input %d, vocos %d / %d, latent %d must be multiples of 32", Cin, C, I, Ld);
    QA_REQUIRE(K >= 1 && D % 8 == 0 && D >= 8 && D <= 64, "bicodec encoder spec: codebook_dim %d must be a multiple of 8 in 8 .. 64", D);
    Loader L(tab, h->store, WN_DETECT);  // BiCodec mixes weight-normed and plain layers
    // Encoder (feat_encoder.py:29-92).  SamplingBlock with both scales 1 returns 3 x (samper.py:78-95): folded into the embed filters
    build_vocos(L, &h->backbone, "encoder.encoder", C, I, sp.vocos_layers, false, 1.0f, Cin);
    for (int i = 0; i < 2; ++i) build_vocos(L, &h->down[i], "encoder.downsample." + std::to_string(i) + ".1", C, I, 2, false, 3.0f);
    L.conv(&h->project, "encoder.project", Ld, C, 1);
    L.conv(&h->in_project, "quantizer.in_project", D, Ld, 1);
    QA_TRY(build_speaker(h, L));
    // F.normalize(codebook) once (factorized_vector_quantize.py:179): fp32 division by the clamped norm, like the reference
    {
        const float* cb = L.need("quantizer.codebook.weight", (int64_t)K * D);
        std::vector<float> cn((size_t)K * D, 0.f), e2((size_t)K, 0.f);
        if (cb)
            for (int k = 0; k < K; ++k) {
                float ss = 0.f;
                for (int d = 0; d < D; ++d) ss = std::fmaf(cb[(size_t)k * D + d], cb[(size_t)k * D + d], ss);
                const float n = std::max(std::sqrt(ss), 1e-12f);
                float q = 0.f;
                for (int d = 0; d < D; ++d) {
                    const float v = cb[(size_t)k * D + d] / n;
                    cn[(size_t)k * D + d] = v;
                    q = std::fmaf(v, v, q);
                }
                e2[k] = q;
            }
        L.raw(&h->codebook, cn);
        L.raw(&h->e2, e2);
    }
    return L.upload();
}

double hz_to_mel_slaney(double f) {  // torchaudio.functional._hz_to_mel(mel_scale="slaney")
    const double f_sp = 200.0 / 3, min_log_hz = 1000.0, min_log_mel = 15.0, logstep = std::log(6.4) / 27.0;
    return f >= min_log_hz ? min_log_mel + std::log(f / min_log_hz) / logstep : f / f_sp;
}
double mel_to_hz_slaney(double m) {
    const double f_sp = 200.0 / 3, min_log_hz = 1000.0, min_log_mel = 15.0, logstep = std::log(6.4) / 27.0;
    return m >= min_log_mel ? min_log_hz * std::exp(logstep * (m - min_log_mel)) : f_sp * m;
}

// BatchNorm1d (eval) after the ReLU: y = relu(conv) * s + t, s = w / sqrt(var + 1e-5), t = b - mean * s
void batchnorm(Loader& L, const std::string& p, int C, std::vector<float>* s, std::vector<float>* t) {
    const float* w = L.need(p + ".weight", C);
    const float* b = L.need(p + ".bias", C);
    const float* m = L.need(p + ".running_mean", C);
    const float* v = L.need(p + ".running_var", C);
    s->assign(C, 1.f);
    t->assign(C, 0.f);
    if (w && b && m && v)
        for (int c = 0; c < C; ++c) {
            (*s)[c] = (float)((double)w[c] / std::sqrt((double)v[c] + 1e-5));
            (*t)[c] = (float)((double)b[c] - (double)m[c] * (*s)[c]);
        }
}
void conv_bn(Loader& L, ConvBnW* dst, const std::string& p, int N, int C_in, int k) {
    L.conv(&dst->conv, p + ".conv", N, C_in, k);
    std::vector<float> s, t;
    batchnorm(L, p + ".bn", N, &s, &t);
    L.raw(&dst->s, s);
    L.raw(&dst->t, t);
}

int build_speaker(qa_bicodec_enc* h, Loader& L) {
    const qa_bicodec_enc_spec& sp = h->spec;
    const int hop = sp.hop_length, nfft = sp.n_fft, C = sp.ecapa_channels, W = C / 8, D = sp.spk_latent_dim;
    QA_REQUIRE(hop >= 16 && hop % 32 == 0 && sp.win_length == 2 * hop && nfft >= sp.win_length && (nfft - sp.win_length) % 2 == 0,
               "bicodec encoder spec: the mel front needs win_length = 2 * hop_length, hop a multiple of 32, n_fft >= win_length "
               "(got n_fft %d, win %d, hop %d)", nfft, sp.win_length, hop);
    QA_REQUIRE(sp.mel_dim % 32 == 0 && C % 32 == 0 && W <= 64 && D % 32 == 0 && D <= 256 && sp.token_num >= 1 && sp.n_levels >= 1 &&
               sp.n_levels <= 8 && sp.perceiver_depth >= 1 && sp.perceiver_heads >= 1,
               "bicodec encoder spec: mel %d, ECAPA channels %d, speaker latent %d unsupported", sp.mel_dim, C, D);
    for (int i = 0; i < sp.n_levels; ++i) QA_REQUIRE(sp.levels[i] >= 2, "bicodec encoder spec: FSQ level %d", sp.levels[i]);
    // ---- mel front: framed-signal DFT (window folded into the basis) and the slaney filterbank
    h->nb = nfft / 2 + 1;
    h->nbp = (int)round_up(h->nb, 4);
    h->kp = (int)round_up(h->nb, 32);
    {
        const int win = sp.win_length, off = (nfft - win) / 2;
        std::vector<float> w((size_t)2 * h->nbp * win, 0.f);
        const double two_pi = 6.283185307179586476925;
        for (int jj = 0; jj < win; ++jj) {
            const double wj = 0.5 - 0.5 * std::cos(two_pi * jj / win);  // periodic Hann (torch.hann_window)
            for (int k = 0; k < h->nb; ++k) {
                const long long ph = ((long long)k * (off + jj)) % nfft;  // exact phase reduction
                const double a = two_pi * (double)ph / nfft;
                w[(size_t)k * win + jj] = (float)(wj * std::cos(a));
                w[(size_t)(h->nbp + k) * win + jj] = (float)(-wj * std::sin(a));
            }
        }
        // library layout [N][ksize][C_in] with tap j, channel c <-> window sample j * hop + c: the row IS the window-ordered basis
        h->dft.N = 2 * h->nbp; h->dft.C_in = hop; h->dft.ksize = 2;
        L.raw(&h->dft.w, w);
    }
    {
        const double fmax = sp.mel_fmax > 0 ? sp.mel_fmax : sp.sample_rate / 2;
        const int M = sp.mel_dim;
        std::vector<double> fpts(M + 2);
        const double m0 = hz_to_mel_slaney(sp.mel_fmin), m1 = hz_to_mel_slaney(fmax);
        for (int i = 0; i < M + 2; ++i) fpts[i] = mel_to_hz_slaney(m0 + (m1 - m0) * i / (M + 1));
        std::vector<float> fb((size_t)M * h->kp, 0.f);  // [mel][bin], torchaudio.functional.melscale_fbanks(norm="slaney")
        for (int k = 0; k < h->nb; ++k) {
            const double f = (double)(sp.sample_rate / 2) * k / (h->nb - 1);
            for (int m = 0; m < M; ++m) {
                const double down = (f - fpts[m]) / (fpts[m + 1] - fpts[m]), up = (fpts[m + 2] - f) / (fpts[m + 2] - fpts[m + 1]);
                const double v = std::max(0.0, std::min(down, up)) * 2.0 / (fpts[m + 2] - fpts[m]);
                fb[(size_t)m * h->kp + k] = (float)v;
            }
        }
        h->fbank.N = M; h->fbank.C_in = h->kp; h->fbank.ksize = 1;
        L.raw(&h->fbank.w, fb);
    }
    // ---- ECAPA-TDNN up to the latent (ecapa_tdnn.py ECAPA_TDNN.forward)
    const std::string e = "speaker_encoder.speaker_encoder";
    conv_bn(L, &h->layer1, e + ".layer1", C, sp.mel_dim, 5);
    for (int bi = 0; bi < 3; ++bi) {
        SeRes2W& b = h->blocks[bi];
        const std::string p = e + ".layer" + std::to_string(bi + 2) + ".se_res2block";
        b.dilation = bi + 2;
        conv_bn(L, &b.c0, p + ".0", C, C, 1);
        conv_bn(L, &b.c2, p + ".2", C, C, 1);
        std::vector<float> wt((size_t)7 * 3 * W * W, 0.f), bst((size_t)7 * 3 * W, 0.f);
        for (int i = 0; i < 7; ++i) {
            const std::string q = p + ".1.convs." + std::to_string(i);
            const float* w = L.need(q + ".weight", (int64_t)W * W * 3);
            const float* bb = L.need(q + ".bias", W);
            std::vector<float> s, t;
            batchnorm(L, p + ".1.bns." + std::to_string(i), W, &s, &t);
            if (w && bb)
                for (int co = 0; co < W; ++co) {
                    for (int ci = 0; ci < W; ++ci)
                        for (int j = 0; j < 3; ++j) wt[(((size_t)i * 3 + j) * W + ci) * W + co] = w[((size_t)co * W + ci) * 3 + j];
                    bst[((size_t)i * 3 + 0) * W + co] = bb[co];
                    bst[((size_t)i * 3 + 1) * W + co] = s[co];
                    bst[((size_t)i * 3 + 2) * W + co] = t[co];
                }
        }
        L.raw(&b.res2_w, wt);
        L.raw(&b.res2_bst, bst);
        {  // SE Linears transposed: [C][128] and [128][C] (se_residual_kernel reads them across the threads of a wave)
            const float* w1 = L.need(p + ".3.linear1.weight", (int64_t)128 * C);
            const float* w2 = L.need(p + ".3.linear2.weight", (int64_t)C * 128);
            std::vector<float> t1((size_t)C * 128, 0.f), t2((size_t)128 * C, 0.f);
            if (w1 && w2)
                for (int o = 0; o < 128; ++o)
                    for (int ch = 0; ch < C; ++ch) {
                        t1[(size_t)ch * 128 + o] = w1[(size_t)o * C + ch];
                        t2[(size_t)o * C + ch] = w2[(size_t)ch * 128 + o];
                    }
            L.raw(&b.se_w1, t1);
            L.raw(&b.se_w2, t2);
        }
        L.vec(&b.se_b1, p + ".3.linear1.bias", 128);
        L.vec(&b.se_b2, p + ".3.linear2.bias", C);
    }
    L.conv(&h->ecapa_out, e + ".conv", 1536, 3 * C, 1);
    // ---- PerceiverResampler (perceiver_encoder.py)
    const std::string pp = "speaker_encoder.perceiver_sampler";
    const int inner = sp.perceiver_heads * sp.perceiver_dim_head;
    h->ff = D * 4 * 2 / 3;  // FeedForward: int(dim * mult * 2 / 3)
    h->ffp = (int)round_up(h->ff, 32);
    L.conv(&h->proj_context, pp + ".proj_context", D, 1536, 1);
    L.vec(&h->latents, pp + ".latents", (int64_t)sp.token_num * D);
    h->perceiver.resize(sp.perceiver_depth);
    for (int i = 0; i < sp.perceiver_depth; ++i) {
        PerceiverLayerW& lw = h->perceiver[i];
        const std::string q = pp + ".layers." + std::to_string(i);
        L.conv(&lw.to_q, q + ".0.to_q", inner, D, 1, false);
        L.conv(&lw.to_kv, q + ".0.to_kv", 2 * inner, D, 1, false);
        L.conv(&lw.to_out, q + ".0.to_out", D, inner, 1, false);
        L.conv(&lw.ff1, q + ".1.0", 2 * h->ff, D, 1);
        std::vector<float> w2, wp((size_t)D * h->ffp, 0.f);
        if (L.weight(q + ".1.2", D, h->ff, &w2))
            for (int n = 0; n < D; ++n)
                for (int k = 0; k < h->ff; ++k) wp[(size_t)n * h->ffp + k] = w2[(size_t)n * h->ff + k];
        lw.ff2.N = D; lw.ff2.C_in = h->ffp; lw.ff2.ksize = 1;
        L.raw(&lw.ff2.w, wp);
        L.vec(&lw.ff2.b, q + ".1.2.bias", D);
    }
    L.vec(&h->norm_gamma, pp + ".norm.gamma", D);
    L.conv(&h->fsq_in, "speaker_encoder.quantizer.project_in", sp.n_levels, D, 1);
    return QA_OK;
}

// rl (per-clip calls; rl.n null: the rectangular call): clip b holds rl.n[b] of the N feature frames; rows of `feat` behind them are
// never read, and tokens[b, n] = -1 for n >= rl.n[b]
int semantic_graph(qa_bicodec_enc* h, Ctx& c, const float* feat, int B, int N, ClipLens rl, long long* tokens) {
    const qa_bicodec_enc_spec& sp = h->spec;
    const int C = sp.vocos_dim, I = sp.vocos_inter, Ld = sp.latent_dim, D = sp.codebook_dim;
    const int64_t rows = (int64_t)B * N;
    float* x = c.arena.alloc<float>(rows * C);
    float* t1 = c.arena.alloc<float>(rows * C);
    float* u = c.arena.alloc<float>(rows * std::max(I, Ld));
    QA_TRY(vocos(c, h->backbone, x, t1, u, B, N, C, nullptr, 0, rl, feat));
    c.tap("enc.backbone", x, rows * C);
    for (int i = 0; i < 2; ++i) QA_TRY(vocos(c, h->down[i], x, t1, u, B, N, C, nullptr, 0, rl));
    c.tap("enc.down", x, rows * C);
    float* z = u;  // the ConvNeXt scratch is dead: z [rows, latent]
    QA_TRY(linear_op(c, x, rows, h->project, z));
    c.tap("enc.out", z, rows * Ld);
    float* ze = c.arena.alloc<float>(rows * D);
    QA_TRY(linear_op(c, z, rows, h->in_project, ze));
    QA_RUN(c, launch_l2norm_rows(ze, ze, rows, D, c.stream));
    // one stage, no residual kept: the codebook search of rvq.hip (dist = (|e|^2 - 2 e.c) + |c|^2, lowest index on a tie)
    QA_RUN(c, launch_rvq_search(ze, rows, h->codebook, h->e2, 1, sp.codebook_size, D, tokens, nullptr, 0, nullptr, c.stream));
    if (rl.n) QA_RUN(c, launch_tokens_fill_behind(tokens, B, N, rl.n, c.stream));
    c.tap("vq.latent", ze, rows * D);
    return QA_OK;
}

int conv_bn_relu(Ctx& c, const float* x, int64_t ldx, int B, int T, const ConvBnW& w, float* y, int64_t ldy, int pad) {
    ConvOpt o;
    o.pad_left = pad; o.pad_right = pad; o.act = ACT_RELU; o.gamma = w.s; o.shift = w.t;
    return conv_op(c, x, ldx, B, T, w.conv, y, ldy, T, o);
}

// latent_out (forward only): the ECAPA latent [B, frames, 1536] stays in the arena for the x-vector head.
// samples (per-clip calls, device [B]; null: the rectangular call): the reference clip of row b is wav[b, k % samples[b]] - the framing
// kernel is the only reader of wav, and everything behind it runs over the ref_len samples every row then has
int global_graph(qa_bicodec_enc* h, Ctx& c, const float* wav, int B, int64_t T, int64_t ref_len, const int* samples, int* tokens,
                 const float** latent_out = nullptr) {
    const qa_bicodec_enc_spec& sp = h->spec;
    const int hop = sp.hop_length, C = sp.ecapa_channels, D = sp.spk_latent_dim, nl = sp.token_num;
    const int nf = (int)(ref_len / hop) + 1;  // torch.stft(center=True) frames
    const int64_t rows = (int64_t)B * nf;
    // ---- mel spectrogram [B, nf, mel_dim]
    float* P = c.arena.alloc<float>((size_t)B * (nf + 1) * hop);
    float* ri = c.arena.alloc<float>((size_t)rows * 2 * h->nbp);
    float* mag = c.arena.alloc<float>((size_t)rows * h->kp);
    float* mel = c.arena.alloc<float>((size_t)rows * sp.mel_dim);
    QA_RUN(c, launch_mel_frames(wav, B, T, ref_len, hop, nf, P, c.stream, samples));
    QA_TRY(conv_op(c, P, hop, B, nf + 1, h->dft, ri, 2 * h->nbp, nf, ConvOpt()));
    QA_RUN(c, launch_spec_mag(ri, h->nbp, h->nb, mag, h->kp, rows, c.stream));
    QA_TRY(linear_op(c, mag, rows, h->fbank, mel));
    c.tap("mel", mel, rows * sp.mel_dim);
    // ---- ECAPA-TDNN latent [B, nf, 1536]
    float* out1 = c.arena.alloc<float>((size_t)rows * C);
    float* cat = c.arena.alloc<float>((size_t)rows * 3 * C);
    float* y1 = c.arena.alloc<float>((size_t)rows * C);
    float* y2 = c.arena.alloc<float>((size_t)rows * C);
    float* gate = c.arena.alloc<float>((size_t)B * C);
    QA_TRY(conv_bn_relu(c, mel, sp.mel_dim, B, nf, h->layer1, out1, C, 2));
    c.tap("ecapa.layer1", out1, rows * C);
    const float* xin = out1;
    int64_t ldin = C;
    for (int bi = 0; bi < 3; ++bi) {
        const SeRes2W& b = h->blocks[bi];
        QA_TRY(conv_bn_relu(c, xin, ldin, B, nf, b.c0, y1, C, 0));
        QA_RUN(c, launch_res2_chain(y1, y2, b.res2_w, b.res2_bst, B, nf, C, b.dilation, c.stream));
        QA_TRY(conv_bn_relu(c, y2, C, B, nf, b.c2, y1, C, 0));
        QA_RUN(c, launch_se_residual(xin, ldin, y1, b.se_w1, b.se_b1, b.se_w2, b.se_b2, gate, cat + (size_t)bi * C, 3 * C, B, nf, C, 128,
                                     c.stream));
        xin = cat + (size_t)bi * C;
        ldin = 3 * C;
    }
    c.tap("ecapa.layers234", cat, rows * 3 * C);
    float* latent = c.arena.alloc<float>((size_t)rows * 1536);
    {
        ConvOpt o;
        o.act = ACT_RELU;
        QA_TRY(conv_op(c, cat, 3 * C, B, nf, h->ecapa_out, latent, 1536, nf, o));
    }
    c.tap("ecapa.latent", latent, rows * 1536);
    if (latent_out) *latent_out = latent;
    // ---- PerceiverResampler [B, token_num, D]
    const int inner = sp.perceiver_heads * sp.perceiver_dim_head, nk = nl + nf;
    const int64_t lrows = (int64_t)B * nl;
    float* xc = c.arena.alloc<float>((size_t)rows * D);
    float* ctx = c.arena.alloc<float>((size_t)B * nk * D);
    float* lat = c.arena.alloc<float>((size_t)lrows * D);
    float* q = c.arena.alloc<float>((size_t)lrows * inner);
    float* kv = c.arena.alloc<float>((size_t)B * nk * 2 * inner);
    float* att = c.arena.alloc<float>((size_t)lrows * inner);
    float* hh = c.arena.alloc<float>((size_t)lrows * 2 * h->ff);
    float* gg = c.arena.alloc<float>((size_t)lrows * h->ffp);
    float* pout = c.arena.alloc<float>((size_t)lrows * D);
    QA_TRY(linear_op(c, latent, rows, h->proj_context, xc));
    QA_RUN(c, launch_perceiver_ctx(h->latents, 0, xc, ctx, B, nl, nf, D, c.stream));      // cat(latents, x)
    QA_RUN(c, launch_perceiver_ctx(h->latents, 0, nullptr, lat, B, nl, 0, D, c.stream));  // latents, broadcast over the batch
    for (size_t li = 0; li < h->perceiver.size(); ++li) {
        const PerceiverLayerW& lw = h->perceiver[li];
        if (li > 0) QA_RUN(c, launch_perceiver_ctx(lat, (int64_t)nl * D, nullptr, ctx, B, nl, nf, D, c.stream));
        QA_TRY(linear_op(c, lat, lrows, lw.to_q, q));
        QA_TRY(linear_op(c, ctx, (int64_t)B * nk, lw.to_kv, kv));
        AttnArgs at;  // the latents over the packed keys / values [B nk, 2 inner] of cat(latents, x)
        at.q = q; at.ldq = inner; at.out = att; at.ldo = inner;
        at.k = kv; at.v = kv + inner; at.ldkv = 2 * inner; at.kv_batch_stride = (int64_t)nk * 2 * inner;
        at.B = B; at.n_q = nl; at.n_keys = nk; at.H = sp.perceiver_heads; at.hd = sp.perceiver_dim_head;
        at.scale = 1.f / std::sqrt((float)sp.perceiver_dim_head);
        QA_TRY(attention_op(c, at));
        QA_TRY(linear_op(c, att, lrows, lw.to_out, lat, epi(ACT_NONE, lat)));
        QA_TRY(linear_op(c, lat, lrows, lw.ff1, hh));
        QA_RUN(c, launch_geglu(hh, h->ff, gg, h->ffp, lrows, c.stream));
        QA_TRY(linear_op(c, gg, lrows, lw.ff2, lat, epi(ACT_NONE, lat)));
    }
    QA_RUN(c, launch_l2norm_scale(lat, h->norm_gamma, pout, lrows, D, std::sqrt((float)D), c.stream));
    c.tap("perceiver.out", pout, lrows * D);
    // ---- ResidualFSQ indices
    float* bounded = c.capture ? c.arena.alloc<float>((size_t)lrows * sp.n_levels) : nullptr;
    QA_RUN(c, launch_fsq(pout, h->fsq_in.w, h->fsq_in.b, sp.levels, sp.n_levels, D, lrows, tokens, bounded, c.stream));
    if (bounded) c.tap("fsq.bounded", bounded, lrows * sp.n_levels);
    return QA_OK;
}

int check_global_shape(const qa_bicodec_enc* h, int64_t B, int64_t T, int64_t ref_len) {
    QA_REQUIRE(B > 0 && T > 0, "qa_bicodec_get_global_tokens: wav is [%lld, %lld]", (long long)B, (long long)T);
    QA_REQUIRE(ref_len > h->spec.n_fft / 2, "qa_bicodec_get_global_tokens: a reference clip of %lld samples is too short for the centred "
               "STFT's reflect padding (n_fft / 2 = %d)", (long long)ref_len, h->spec.n_fft / 2);
    QA_REQUIRE(B * (ref_len / h->spec.hop_length + 2) * 3 * h->spec.ecapa_channels < (1LL << 31) && B * T < (1LL << 40),
               "qa_bicodec_get_global_tokens: batch too large (split it)");
    return QA_OK;
}

// ---------------------------------------------------------------- BiCodec.forward (bicodec.py:113-149)

void vocos_keys(std::vector<std::pair<std::string, int64_t>>* k, const std::string& p, int C, int I, int n_layers) {
    k->push_back({p + ".embed.weight", (int64_t)C * C * 7});
    k->push_back({p + ".embed.bias", C});
    k->push_back({p + ".norm.weight", C});
    k->push_back({p + ".norm.bias", C});
    for (int i = 0; i < n_layers; ++i) {
        const std::string q = p + ".convnext." + std::to_string(i);
        k->push_back({q + ".dwconv.weight", (int64_t)C * 7});
        k->push_back({q + ".dwconv.bias", C});
        k->push_back({q + ".norm.weight", C});
        k->push_back({q + ".norm.bias", C});
        k->push_back({q + ".pwconv1.weight", (int64_t)I * C});
        k->push_back({q + ".pwconv1.bias", I});
        k->push_back({q + ".pwconv2.weight", (int64_t)C * I});
        k->push_back({q + ".pwconv2.bias", C});
        k->push_back({q + ".gamma", C});
    }
    k->push_back({p + ".final_layer_norm.weight", C});
    k->push_back({p + ".final_layer_norm.bias", C});
}

// The forward-only weights: the x-vector head speaker_encoder.speaker_encoder.{pool.linear1, pool.linear2, bn, linear}.* (into the
// tokenizer handle, which owns the ECAPA latent) and postnet.* (into the detokenizer handle, which owns the prenet output).  Every key is
// checked in module order before anything is folded, so the error names the first missing or mis-shaped one.
int build_forward(const qa_bicodec* dec, const qa_bicodec_enc* enc, const qa_bicodec_forward_spec& sp, const HostTable& tab,
                  std::unique_ptr<qa_bicodec::Postnet>* post_out, std::unique_ptr<qa_bicodec_enc::XvecHead>* xvec_out) {
    const qa_bicodec_spec& ds = dec->spec;
    const qa_bicodec_enc_spec& es = enc->spec;
    const int Ld = ds.latent_dim, C = sp.postnet_vocos_dim, I = sp.postnet_vocos_inter, O = sp.postnet_out_channels, X = sp.xvector_dim;
    QA_REQUIRE(dec->device == enc->device, "bicodec forward: the detokenizer (device %d) and the tokenizer (device %d) must share a device",
               dec->device, enc->device);
    QA_REQUIRE(sp.postnet_input_channels == Ld, "bicodec forward: postnet.input_channels %d != the prenet output width %d",
               sp.postnet_input_channels, Ld);
    QA_REQUIRE(C > 0 && C % 32 == 0 && I > 0 && I % 32 == 0 && O > 0 && O % 32 == 0 && sp.postnet_vocos_layers >= 1,
               "bicodec forward: postnet vocos_dim %d, vocos_intermediate_dim %d, out_channels %d must be positive multiples of 32 and "
               "vocos_num_layers %d >= 1", C, I, O, sp.postnet_vocos_layers);
    QA_REQUIRE(X > 0 && X % 32 == 0, "bicodec forward: speaker_encoder.out_dim %d must be a positive multiple of 32", X);
    QA_REQUIRE(es.ecapa_channels * 3 == 1536, "bicodec forward: the pooling head reads the 1536-wide ECAPA latent (channels %d)",
               es.ecapa_channels);
    bool same = es.latent_dim == Ld && es.codebook_size == ds.codebook_size && es.token_num == ds.token_num && es.n_levels == ds.n_levels;
    for (int i = 0; same && i < ds.n_levels; ++i) same = es.levels[i] == ds.levels[i];
    QA_REQUIRE(same, "bicodec forward: the tokenizer (latent %d, codebook %d, %d global tokens of %d levels) and the detokenizer (latent %d, "
               "codebook %d, %d global tokens of %d levels) disagree", es.latent_dim, es.codebook_size, es.token_num, es.n_levels, Ld,
               ds.codebook_size, ds.token_num, ds.n_levels);
    const std::string e = "speaker_encoder.speaker_encoder";
    std::vector<std::pair<std::string, int64_t>> keys = {
        {e + ".pool.linear1.weight", (int64_t)128 * 4608}, {e + ".pool.linear1.bias", 128},
        {e + ".pool.linear2.weight", (int64_t)1536 * 128}, {e + ".pool.linear2.bias", 1536},
        {e + ".bn.weight", 3072}, {e + ".bn.bias", 3072}, {e + ".bn.running_mean", 3072}, {e + ".bn.running_var", 3072},
        {e + ".linear.weight", (int64_t)X * 3072}, {e + ".linear.bias", X},
        {"postnet.linear_pre.weight", (int64_t)C * Ld}, {"postnet.linear_pre.bias", C}};
    for (int i = 0; i < 2; ++i) vocos_keys(&keys, "postnet.downsample." + std::to_string(i) + ".1", C, I, 2);
    vocos_keys(&keys, "postnet.vocos_backbone", C, I, sp.postnet_vocos_layers);
    keys.push_back({"postnet.linear.weight", (int64_t)O * C});
    keys.push_back({"postnet.linear.bias", O});
    for (const auto& k : keys)
        if (!tab.get(k.first, k.second)) return QA_ERR_MISSING;  // HostTable::get has set the error message
    std::unique_ptr<qa_bicodec_enc::XvecHead> xv(new qa_bicodec_enc::XvecHead());
    {
        Loader L(tab, xv->store);
        std::vector<float> w1;  // [128][4608]: columns 0 .. 1535 the frames, 1536 .. 4607 the context (pooling_layers.py:133)
        if (L.weight(e + ".pool.linear1", 128, 4608, &w1)) {
            std::vector<float> wx((size_t)128 * 1536), wc((size_t)128 * 3072);
            for (int n = 0; n < 128; ++n) {
                std::memcpy(&wx[(size_t)n * 1536], &w1[(size_t)n * 4608], sizeof(float) * 1536);
                std::memcpy(&wc[(size_t)n * 3072], &w1[(size_t)n * 4608 + 1536], sizeof(float) * 3072);
            }
            xv->lin1x.N = 128; xv->lin1x.C_in = 1536; xv->lin1x.ksize = 1;
            xv->lin1c.N = 128; xv->lin1c.C_in = 3072; xv->lin1c.ksize = 1;
            L.raw(&xv->lin1x.w, wx);
            L.raw(&xv->lin1c.w, wc);
            L.vec(&xv->lin1c.b, e + ".pool.linear1.bias", 128);
        }
        L.conv(&xv->lin2, e + ".pool.linear2", 1536, 128, 1);
        std::vector<float> s, t;
        batchnorm(L, e + ".bn", 3072, &s, &t);
        L.raw(&xv->bn_s, s);
        L.raw(&xv->bn_t, t);
        L.conv(&xv->linear, e + ".linear", X, 3072, 1);
        QA_TRY(L.upload());
    }
    std::unique_ptr<qa_bicodec::Postnet> pn(new qa_bicodec::Postnet());
    pn->spec = sp;
    {
        Loader L(tab, pn->store);
        L.conv(&pn->linear_pre, "postnet.linear_pre", C, Ld, 1);
        for (int i = 0; i < 2; ++i) build_vocos(L, &pn->down[i], "postnet.downsample." + std::to_string(i) + ".1", C, I, 2, false, 3.0f);
        build_vocos(L, &pn->backbone, "postnet.vocos_backbone", C, I, sp.postnet_vocos_layers, false, 1.0f);
        L.conv(&pn->linear_out, "postnet.linear", O, C, 1);
        QA_TRY(L.upload());
    }
    *post_out = std::move(pn);
    *xvec_out = std::move(xv);
    return QA_OK;
}

// the tokenizer half of forward: semantic tokens and their statistics, global tokens of the whole rows (ref_len = T) as int64, and the
// x-vector from the ECAPA latent global_graph leaves in the arena (it is not recomputed)
int forward_enc_graph(qa_bicodec_enc* h, Ctx& c, const float* feat, int B, int N, const float* wav, int64_t T, long long* sem,
                      long long* glob, float* xvec, float* perplexity, float* active) {
    const qa_bicodec_enc_spec& sp = h->spec;
    const qa_bicodec_enc::XvecHead& xv = *h->xvec;
    QA_TRY(semantic_graph(h, c, feat, B, N, ClipLens(), sem));
    QA_RUN(c, launch_code_usage(sem, (long long)B * N, sp.codebook_size, perplexity, active, c.stream));
    int* g32 = c.arena.alloc<int>((size_t)B * sp.token_num);
    const float* latent = nullptr;
    QA_TRY(global_graph(h, c, wav, B, T, T, nullptr, g32, &latent));
    QA_RUN(c, launch_widen_i32(g32, glob, (long long)B * sp.token_num, c.stream));
    // ---- x-vector (ecapa_tdnn.py:204-206): ASTP with the global context of ECAPA_TDNN_GLOB_c512 (pooling_layers.py:129-144), BN, Linear.
    // linear1(cat(x, mean, std)) = W_x x + (W_c [mean; std] + b): the context half is one row per item, folded into that item's bias
    const int nf = (int)(T / sp.hop_length) + 1;
    const int64_t rows = (int64_t)B * nf;
    float* ctx = c.arena.alloc<float>((size_t)B * 3072);
    float* cb = c.arena.alloc<float>((size_t)B * 128);
    float* a1 = c.arena.alloc<float>((size_t)rows * 128);
    float* logit = c.arena.alloc<float>((size_t)rows * 1536);
    float* pool = c.arena.alloc<float>((size_t)B * 3072);
    float* bn = c.arena.alloc<float>((size_t)B * 3072);
    QA_RUN(c, launch_frame_stats(latent, B, nf, 1536, ctx, c.stream));
    QA_TRY(linear_per_item(c, ctx, B, xv.lin1c, cb));
    for (int b = 0; b < B; ++b) {  // tanh(W_x x + cb[b]) over the item's frames
        ConvW w = xv.lin1x;
        w.b = cb + (size_t)b * 128;
        QA_TRY(conv_op(c, latent + (size_t)b * nf * 1536, 1536, 1, nf, w, a1 + (size_t)b * nf * 128, 128, nf, epi(ACT_TANH)));
    }
    QA_TRY(linear_op(c, a1, rows, xv.lin2, logit));
    QA_RUN(c, launch_astp_pool(logit, latent, B, nf, 1536, xv.bn_s, xv.bn_t, pool, bn, c.stream));
    c.tap("ecapa.pool", pool, (int64_t)B * 3072);
    QA_TRY(linear_per_item(c, bn, B, xv.linear, xvec));
    c.tap("x_vector", xvec, (int64_t)B * xv.linear.N);
    return QA_OK;
}

}  // namespace

extern "C" {

int qa_bicodec_create(qa_bicodec** out, const qa_bicodec_spec* spec, const qa_tensor* tensors, int64_t n_tensors, int device) {
    if (!out || !spec || !tensors) {
        set_error("qa_bicodec_create: null argument");
        return QA_ERR_INVALID;
    }
    *out = nullptr;
    QA_HIP(hipSetDevice(device));
    std::unique_ptr<qa_bicodec> h(new qa_bicodec());
    h->spec = *spec;
    h->device = device;
    QA_TRY(build(h.get(), HostTable(tensors, n_tensors)));
    *out = h.release();
    return QA_OK;
}

void qa_bicodec_destroy(qa_bicodec* h) { destroy_handle(h); }

int64_t qa_bicodec_hop(const qa_bicodec* h) { return h ? h->hop : QA_ERR_INVALID; }

// qa_bicodec_detokenize (lengths == nullptr) and qa_bicodec_detokenize_ragged.  Every check runs before the first launch; a length vector
// whose entries all equal T leaves the call without a device array: the rectangular call as it is
static int detokenize_call(qa_bicodec* h, const char* fn, const int64_t* semantic_tokens, const int64_t* global_tokens, int64_t B, int64_t T,
                           const int64_t* lengths, float* wav_out, void* stream) {
    QA_REQUIRE(B > 0 && T > 0, "%s: tokens are [%lld, %lld]", fn, (long long)B, (long long)T);
    QA_REQUIRE(B * T * (int64_t)h->hop * 32 < (1LL << 31), "%s: batch too large (split it)", fn);
    const int* lens = nullptr;
    if (lengths) {
        std::vector<int> len;
        bool full = true;
        QA_TRY(check_clip_lengths(fn, B, lengths, 1, T, "tokens", "T", &len, &full));
        if (!full) {
            QA_HIP(hipSetDevice(h->device));
            QA_TRY(h->lens.upload({&len}, static_cast<hipStream_t>(stream), &lens));
        }
    }
    return run_planned(*h, stream, [&] {
        return detokenize_graph(h, h->ctx, (const long long*)semantic_tokens, (const long long*)global_tokens, (int)B, (int)T,
                                ClipLens{lens, lens ? 1 : 0}, wav_out);
    });
}

int qa_bicodec_detokenize(qa_bicodec* h, const int64_t* semantic_tokens, const int64_t* global_tokens, int64_t B, int64_t T, float* wav_out,
                          void* stream) {
    if (!h || !semantic_tokens || !global_tokens || !wav_out) {
        set_error("qa_bicodec_detokenize: null argument");
        return QA_ERR_INVALID;
    }
    return detokenize_call(h, "qa_bicodec_detokenize", semantic_tokens, global_tokens, B, T, nullptr, wav_out, stream);
}

int qa_bicodec_detokenize_ragged(qa_bicodec* h, const int64_t* semantic_tokens, const int64_t* global_tokens, int64_t B, int64_t T,
                                 const int64_t* lengths, float* wav_out, void* stream) {
    if (!h || !semantic_tokens || !global_tokens || !lengths || !wav_out) {
        set_error("qa_bicodec_detokenize_ragged: null argument");
        return QA_ERR_INVALID;
    }
    return detokenize_call(h, "qa_bicodec_detokenize_ragged", semantic_tokens, global_tokens, B, T, lengths, wav_out, stream);
}

int qa_bicodec_enc_create(qa_bicodec_enc** out, const qa_bicodec_enc_spec* spec, const qa_tensor* tensors, int64_t n_tensors, int device) {
    if (!out || !spec || !tensors) {
        set_error("qa_bicodec_enc_create: null argument");
        return QA_ERR_INVALID;
    }
    *out = nullptr;
    QA_HIP(hipSetDevice(device));
    std::unique_ptr<qa_bicodec_enc> h(new qa_bicodec_enc());
    h->spec = *spec;
    h->device = device;
    QA_TRY(build_encoder(h.get(), HostTable(tensors, n_tensors)));
    *out = h.release();
    return QA_OK;
}

void qa_bicodec_enc_destroy(qa_bicodec_enc* h) { destroy_handle(h); }

// The tokenizer's entry points, rectangular (lengths == nullptr) and per-clip.  *_checks: every check of a call,
// lengths included (frames: 1 .. N feature frames; samples: 1 .. T samples) - all of them run before the first launch, and for
// qa_bicodec_tokenize_ragged both halves are checked before either runs.  A vector whose entries all equal the full extent leaves its
// half without a device array: the rectangular call as it is.
struct EncLens {
    std::vector<int> len;
    bool ragged = false;
    const int* dev = nullptr;  // the device copy of a ragged half (upload_lens)
};
static int semantic_checks(qa_bicodec_enc* h, const char* fn, int64_t B, int64_t N, const int64_t* frame_lengths, EncLens* out) {
    QA_REQUIRE(B > 0 && N > 0, "%s: feat is [%lld, %lld, C]", fn, (long long)B, (long long)N);
    QA_REQUIRE(B * N * (int64_t)std::max(h->spec.vocos_inter, h->spec.input_channels) < (1LL << 31), "%s: batch too large (split it)", fn);
    if (frame_lengths) {
        bool full = true;
        QA_TRY(check_clip_lengths(fn, B, frame_lengths, 1, N, "feature frames", "N", &out->len, &full));
        out->ragged = !full;
    }
    return QA_OK;
}
static int global_checks(qa_bicodec_enc* h, const char* fn, int64_t B, int64_t T, int64_t* ref_len, const int64_t* lengths, EncLens* out) {
    if (lengths) {
        QA_REQUIRE(B > 0 && T > 0, "%s: wav is [%lld, %lld]", fn, (long long)B, (long long)T);
        bool full = true;
        QA_TRY(check_clip_lengths(fn, B, lengths, 1, T, "samples", "T", &out->len, &full));
        out->ragged = !full;
        // without a reference length every clip would be its own row with its own frame count: not one rectangular mel
        QA_REQUIRE(full || *ref_len > 0, "%s: clips of different lengths need ref_len > 0 (the reference clip every row is tiled or truncated to)",
                   fn);
    }
    if (*ref_len <= 0) *ref_len = T;
    return check_global_shape(h, B, T, *ref_len);
}
// The lengths of one call on their way to the kernels: every ragged half in ONE upload (a rectangular half carries none, dev stays null)
static int upload_lens(qa_bicodec_enc* h, void* stream, EncLens* a, EncLens* b = nullptr) {
    std::vector<EncLens*> ragged;
    for (EncLens* l : {a, b})
        if (l && l->ragged) ragged.push_back(l);
    if (ragged.empty()) return QA_OK;
    std::vector<const std::vector<int>*> src;
    for (EncLens* l : ragged) src.push_back(&l->len);
    const int* dev[2] = {nullptr, nullptr};
    QA_HIP(hipSetDevice(h->device));
    QA_TRY(h->lens.upload(src, static_cast<hipStream_t>(stream), dev));
    for (size_t i = 0; i < ragged.size(); ++i) ragged[i]->dev = dev[i];
    return QA_OK;
}
static int semantic_run(qa_bicodec_enc* h, const float* feat, int64_t B, int64_t N, const EncLens& fl, int64_t* semantic_out, void* stream) {
    return run_planned(*h, stream, [&] {
        return semantic_graph(h, h->ctx, feat, (int)B, (int)N, ClipLens{fl.dev, fl.dev ? 1 : 0}, (long long*)semantic_out);
    });
}
static int global_run(qa_bicodec_enc* h, const float* wav, int64_t B, int64_t T, int64_t ref_len, const EncLens& sl, int32_t* global_out,
                      void* stream) {
    return run_planned(*h, stream, [&] { return global_graph(h, h->ctx, wav, (int)B, T, ref_len, sl.dev, (int*)global_out); });
}

int qa_bicodec_get_semantic_tokens(qa_bicodec_enc* h, const float* feat, int64_t B, int64_t N, int64_t* semantic_out, void* stream) {
    if (!h || !feat || !semantic_out) {
        set_error("qa_bicodec_get_semantic_tokens: null argument");
        return QA_ERR_INVALID;
    }
    EncLens fl;
    QA_TRY(semantic_checks(h, "qa_bicodec_get_semantic_tokens", B, N, nullptr, &fl));
    return semantic_run(h, feat, B, N, fl, semantic_out, stream);
}

int qa_bicodec_get_semantic_tokens_ragged(qa_bicodec_enc* h, const float* feat, int64_t B, int64_t N, const int64_t* frame_lengths,
                                          int64_t* semantic_out, void* stream) {
    if (!h || !feat || !frame_lengths || !semantic_out) {
        set_error("qa_bicodec_get_semantic_tokens_ragged: null argument");
        return QA_ERR_INVALID;
    }
    EncLens fl;
    QA_TRY(semantic_checks(h, "qa_bicodec_get_semantic_tokens_ragged", B, N, frame_lengths, &fl));
    QA_TRY(upload_lens(h, stream, &fl));
    return semantic_run(h, feat, B, N, fl, semantic_out, stream);
}

int qa_bicodec_get_global_tokens(qa_bicodec_enc* h, const float* wav, int64_t B, int64_t T, int64_t ref_len, int32_t* global_out, void* stream) {
    if (!h || !wav || !global_out) {
        set_error("qa_bicodec_get_global_tokens: null argument");
        return QA_ERR_INVALID;
    }
    EncLens sl;
    QA_TRY(global_checks(h, "qa_bicodec_get_global_tokens", B, T, &ref_len, nullptr, &sl));
    return global_run(h, wav, B, T, ref_len, sl, global_out, stream);
}

int qa_bicodec_get_global_tokens_ragged(qa_bicodec_enc* h, const float* wav, int64_t B, int64_t T, const int64_t* lengths, int64_t ref_len,
                                        int32_t* global_out, void* stream) {
    if (!h || !wav || !lengths || !global_out) {
        set_error("qa_bicodec_get_global_tokens_ragged: null argument");
        return QA_ERR_INVALID;
    }
    EncLens sl;
    QA_TRY(global_checks(h, "qa_bicodec_get_global_tokens_ragged", B, T, &ref_len, lengths, &sl));
    QA_TRY(upload_lens(h, stream, &sl));
    return global_run(h, wav, B, T, ref_len, sl, global_out, stream);
}

int qa_bicodec_tokenize(qa_bicodec_enc* h, const float* feat, int64_t B, int64_t N, const float* ref_wav, int64_t T_ref, int64_t ref_len,
                        int64_t* semantic_out, int32_t* global_out, void* stream) {
    if (!h || !feat || !ref_wav || !semantic_out || !global_out) {
        set_error("qa_bicodec_tokenize: null argument");
        return QA_ERR_INVALID;
    }
    QA_TRY(qa_bicodec_get_semantic_tokens(h, feat, B, N, semantic_out, stream));
    return qa_bicodec_get_global_tokens(h, ref_wav, B, T_ref, ref_len, global_out, stream);
}

int qa_bicodec_tokenize_ragged(qa_bicodec_enc* h, const float* feat, int64_t B, int64_t N, const int64_t* frame_lengths, const float* ref_wav,
                               int64_t T_ref, const int64_t* lengths, int64_t ref_len, int64_t* semantic_out, int32_t* global_out,
                               void* stream) {
    if (!h || !feat || !frame_lengths || !ref_wav || !lengths || !semantic_out || !global_out) {
        set_error("qa_bicodec_tokenize_ragged: null argument");
        return QA_ERR_INVALID;
    }
    EncLens fl, sl;
    QA_TRY(semantic_checks(h, "qa_bicodec_tokenize_ragged", B, N, frame_lengths, &fl));
    QA_TRY(global_checks(h, "qa_bicodec_tokenize_ragged", B, T_ref, &ref_len, lengths, &sl));
    QA_TRY(upload_lens(h, stream, &fl, &sl));
    QA_TRY(semantic_run(h, feat, B, N, fl, semantic_out, stream));
    return global_run(h, ref_wav, B, T_ref, ref_len, sl, global_out, stream);
}

int qa_bicodec_enc_enable_taps(qa_bicodec_enc* h, int on) { return taps_enable(h ? &h->ctx : nullptr, "qa_bicodec_enc_enable_taps", on); }

int64_t qa_bicodec_enc_tap(qa_bicodec_enc* h, const char* name, float* dst, int64_t cap, void* stream) {
    return tap_read(h ? &h->ctx : nullptr, "qa_bicodec_enc_tap", name, dst, cap, stream);
}

int qa_wav_normalize(const float* wav, int64_t B, int64_t T, float* out, float eps, void* stream) {
    if (!wav || !out) {
        set_error("qa_wav_normalize: null argument");
        return QA_ERR_INVALID;
    }
    QA_REQUIRE(B > 0 && B < (1LL << 31) && T > 0, "qa_wav_normalize: wav is [%lld, %lld]", (long long)B, (long long)T);
    QA_REQUIRE(eps >= 0.f, "qa_wav_normalize: eps %g < 0", (double)eps);
    return launch_wav_normalize(wav, out, (int)B, (long long)T, eps, static_cast<hipStream_t>(stream));
}

int qa_wav_normalize_ragged(const float* wav, int64_t B, int64_t T, const int64_t* lengths, float* out, float eps, void* stream) {
    if (!wav || !lengths || !out) {
        set_error("qa_wav_normalize_ragged: null argument");
        return QA_ERR_INVALID;
    }
    QA_REQUIRE(B > 0 && B < (1LL << 31) && T > 0, "qa_wav_normalize_ragged: wav is [%lld, %lld]", (long long)B, (long long)T);
    QA_REQUIRE(eps >= 0.f, "qa_wav_normalize_ragged: eps %g < 0", (double)eps);
    std::vector<int> len;
    bool full = true;
    QA_TRY(check_clip_lengths("qa_wav_normalize_ragged", B, lengths, 1, T, "samples", "T", &len, &full));
    static_assert(sizeof(long long) == sizeof(int64_t), "the launcher reads the caller's int64 lengths as they are");
    return launch_wav_normalize(wav, out, (int)B, (long long)T, eps, static_cast<hipStream_t>(stream),
                                full ? nullptr : reinterpret_cast<const long long*>(lengths));
}

int qa_bicodec_enable_taps(qa_bicodec* h, int on) { return taps_enable(h ? &h->ctx : nullptr, "qa_bicodec_enable_taps", on); }

int64_t qa_bicodec_tap(qa_bicodec* h, const char* name, float* dst, int64_t cap, void* stream) {
    return tap_read(h ? &h->ctx : nullptr, "qa_bicodec_tap", name, dst, cap, stream);
}

int qa_code_usage(const int64_t* indices, int64_t n, int32_t codebook_size, float* perplexity, float* cluster_size, void* stream) {
    if (!indices || !perplexity || !cluster_size) {
        set_error("qa_code_usage: null argument");
        return QA_ERR_INVALID;
    }
    return launch_code_usage((const long long*)indices, n, codebook_size, perplexity, cluster_size, static_cast<hipStream_t>(stream));
}

int qa_bicodec_load_forward(qa_bicodec* dec, qa_bicodec_enc* enc, const qa_bicodec_forward_spec* spec, const qa_tensor* tensors,
                            int64_t n_tensors) {
    if (!dec || !enc || !spec || !tensors) {
        set_error("qa_bicodec_load_forward: null argument");
        return QA_ERR_INVALID;
    }
    QA_HIP(hipSetDevice(dec->device));
    std::unique_ptr<qa_bicodec::Postnet> post;
    std::unique_ptr<qa_bicodec_enc::XvecHead> xvec;
    QA_TRY(build_forward(dec, enc, *spec, HostTable(tensors, n_tensors), &post, &xvec));
    if (dec->post || enc->xvec) QA_HIP(hipDeviceSynchronize());  // the old weights may still be read by an earlier forward
    dec->post = std::move(post);
    enc->xvec = std::move(xvec);
    return QA_OK;
}

int qa_bicodec_has_forward(const qa_bicodec* dec, const qa_bicodec_enc* enc) {
    if (!dec || !enc) {
        set_error("qa_bicodec_has_forward: null handle");
        return QA_ERR_INVALID;
    }
    return dec->post && enc->xvec ? 1 : 0;
}

int qa_bicodec_forward(qa_bicodec* dec, qa_bicodec_enc* enc, const float* feat, int64_t B, int64_t N, const float* ref_wav, int64_t T_ref,
                       int64_t* semantic_out, int64_t* global_out, float* recons, float* pred_feat, float* x_vector, float* d_vector,
                       float* perplexity, float* cluster_size, void* stream) {
    if (!dec || !enc || !feat || !ref_wav || !semantic_out || !global_out || !recons || !pred_feat || !x_vector || !d_vector || !perplexity ||
        !cluster_size) {
        set_error("qa_bicodec_forward: null argument");
        return QA_ERR_INVALID;
    }
    QA_REQUIRE(dec->post && enc->xvec, "qa_bicodec_forward: no forward head is attached (qa_bicodec_load_forward: the checkpoint's "
               "postnet.* and speaker_encoder.speaker_encoder.{pool, bn, linear}.* weights)");
    QA_REQUIRE(B > 0 && N > 0, "qa_bicodec_forward: feat is [%lld, %lld, C]", (long long)B, (long long)N);
    const qa_bicodec_forward_spec& ps = dec->post->spec;
    const int64_t wide = std::max({(int64_t)enc->spec.vocos_inter, (int64_t)enc->spec.input_channels, (int64_t)ps.postnet_vocos_inter,
                                   (int64_t)ps.postnet_out_channels, (int64_t)dec->hop * 32});
    QA_REQUIRE(B * N * wide < (1LL << 31) && B * N < (1LL << 24), "qa_bicodec_forward: batch too large (split it)");
    QA_TRY(check_global_shape(enc, B, T_ref, T_ref));
    QA_TRY(run_planned(*enc, stream, [&] {
        return forward_enc_graph(enc, enc->ctx, feat, (int)B, (int)N, ref_wav, T_ref, (long long*)semantic_out, (long long*)global_out,
                                 x_vector, perplexity, cluster_size);
    }));
    return run_planned(*dec, stream, [&] {
        return detokenize_graph(dec, dec->ctx, (const long long*)semantic_out, (const long long*)global_out, (int)B, (int)N, ClipLens(), recons,
                                pred_feat, d_vector);
    });
}

}  // extern "C"
