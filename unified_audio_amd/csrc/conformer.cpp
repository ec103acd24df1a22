// conformer.cpp - the condition encoder of the UniSE LM and the log-mel front that feeds it.
//
// CustomLlamaModel's condition path (QuarkAudio-UniSE/model/llm/llm.py:52-54,130-132,304-306): cond_input_layer (Linear cond_dim -> dim),
// cond_encoder (ConformerEncoder, model/llm/conformer.py:384-484, eval mode) and cond_output_layer (Linear dim -> hidden).  One layer:
//   x = 0.5 FF1(x) + x;  x = Attn(LN(x)) + x;  x = Conv(x) + x;  x = 0.5 FF2(x) + x;  x = LN(x)
// The factor 0.5 is folded into each FeedForward's second Linear at load (exact in binary floating point), BatchNorm1d's running
// statistics into a per-channel scale / shift.  Model.stft_logmel (model/model.py:53-79) runs as a framed-signal DFT GEMM like the
// BiCodec mel front.
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <tuple>

#include "host_util.h"
#include "row_lengths.h"

using namespace qa;

namespace {
constexpr int CF_MAX_POS = 4096;  // frames per call: the RoPE table's length (the LM takes at most 4096 positions)
constexpr int CF_MAX_K = 31;

struct FeedForwardW {
    const float *lnw = nullptr, *lnb = nullptr;
    ConvW l1, l2h;  // l2h: weight and bias times 0.5
};
struct ConformerLayerW {
    FeedForwardW ff1, ff2;
    const float *anw = nullptr, *anb = nullptr, *cnw = nullptr, *cnb = nullptr, *fnw = nullptr, *fnb = nullptr;
    ConvW qkv, out, pw1, pw2;
    const float *dw = nullptr, *dwb = nullptr, *bns = nullptr, *bnt = nullptr;  // depthwise taps [31][C] (centred), bias, BatchNorm scale / shift
};
}  // namespace

struct qa_cond_encoder : Handle {
    qa_cond_encoder_spec spec{};
    ConvW in_layer, out_layer;
    std::vector<ConformerLayerW> layers;
    const float* rope = nullptr;
    int* host_counts = nullptr;  // pinned: valid keys per batch item of a masked call
    int host_cap = 0;
    DeviceInts lens;  // the _ragged entry points: the items' frame counts
    ~qa_cond_encoder() {
        if (host_counts) (void)hipHostFree(host_counts);
    }
};

namespace {

// Linear [N, C] (+ bias) scaled by `gain`, recording the key names it read
struct Keys {
    std::set<std::string> seen;
};
void lin(Loader& L, Keys& K, ConvW* dst, const std::string& p, int N, int C, float gain = 1.f) {
    K.seen.insert(p + ".weight");
    K.seen.insert(p + ".bias");
    std::vector<float> w((size_t)N * C, 0.f), b((size_t)N, 0.f);
    if (const float* wp = L.need(p + ".weight", (int64_t)N * C))
        for (size_t i = 0; i < w.size(); ++i) w[i] = wp[i] * gain;
    if (const float* bp = L.need(p + ".bias", N))
        for (int i = 0; i < N; ++i) b[i] = bp[i] * gain;
    dst->N = N; dst->C_in = C; dst->ksize = 1;
    L.raw(&dst->w, w);
    L.raw(&dst->b, b);
}
void norm(Loader& L, Keys& K, const float** w, const float** b, const std::string& p, int d) {
    K.seen.insert(p + ".weight");
    K.seen.insert(p + ".bias");
    L.norm(w, b, p, d);
}
void feed_forward(Loader& L, Keys& K, FeedForwardW* f, const std::string& p, int d, int inner) {
    norm(L, K, &f->lnw, &f->lnb, p + ".sequential.0", d);
    lin(L, K, &f->l1, p + ".sequential.1", inner, d);
    lin(L, K, &f->l2h, p + ".sequential.4", d, inner, 0.5f);
}

int build_encoder(qa_cond_encoder* h, const qa_tensor* tensors, int64_t n_tensors) {
    const qa_cond_encoder_spec& sp = h->spec;
    const int d = sp.dim, H = sp.heads, hd = sp.dim_head, inner = H * hd, k = sp.dw_kernel, ffd = d * sp.ff_mult;
    HostTable tab(tensors, n_tensors);
    Loader L(tab, h->store);
    Keys K;
    const bool wrapped = sp.cond_dim > 0;
    const std::string root = wrapped ? "cond_encoder." : "";
    if (wrapped) {
        lin(L, K, &h->in_layer, "cond_input_layer", d, sp.cond_dim);
        lin(L, K, &h->out_layer, "cond_output_layer", sp.hidden_out, d);
    }
    h->layers.resize(sp.n_layers);
    for (int l = 0; l < sp.n_layers; ++l) {
        ConformerLayerW& W = h->layers[l];
        const std::string p = root + "layers." + std::to_string(l);
        feed_forward(L, K, &W.ff1, p + ".ff1", d, ffd);
        feed_forward(L, K, &W.ff2, p + ".ff2", d, ffd);
        norm(L, K, &W.anw, &W.anb, p + ".attn_norm", d);
        norm(L, K, &W.cnw, &W.cnb, p + ".conv_module.layer_norm", d);
        norm(L, K, &W.fnw, &W.fnb, p + ".final_norm", d);
        {  // fused q / k / v projection
            std::vector<float> w((size_t)3 * inner * d, 0.f), b((size_t)3 * inner, 0.f);
            const char* nm[3] = {".attn.to_q", ".attn.to_k", ".attn.to_v"};
            for (int j = 0; j < 3; ++j) {
                K.seen.insert(p + nm[j] + ".weight");
                K.seen.insert(p + nm[j] + ".bias");
                if (const float* wp = L.need(p + nm[j] + ".weight", (int64_t)inner * d))
                    std::memcpy(&w[(size_t)j * inner * d], wp, sizeof(float) * inner * d);
                if (const float* bp = L.need(p + nm[j] + ".bias", inner)) std::memcpy(&b[(size_t)j * inner], bp, sizeof(float) * inner);
            }
            W.qkv.N = 3 * inner; W.qkv.C_in = d; W.qkv.ksize = 1;
            L.raw(&W.qkv.w, w);
            L.raw(&W.qkv.b, b);
        }
        lin(L, K, &W.out, p + ".attn.to_out.0", d, inner);
        const std::string cp = p + ".conv_module.sequential";
        lin(L, K, &W.pw1, cp + ".0", 2 * d, d);  // Conv1d(d, 2d, 1): [2d, d, 1]
        lin(L, K, &W.pw2, cp + ".5", d, d);
        {  // depthwise taps [d, 1, k] -> 31 centred taps [31][d]
            K.seen.insert(cp + ".2.weight");
            K.seen.insert(cp + ".2.bias");
            std::vector<float> w((size_t)CF_MAX_K * d, 0.f);
            const int shift = CF_MAX_K / 2 - k / 2;
            if (const float* wp = L.need(cp + ".2.weight", (int64_t)d * k))
                for (int c = 0; c < d; ++c)
                    for (int j = 0; j < k; ++j) w[(size_t)(j + shift) * d + c] = wp[(size_t)c * k + j];
            L.raw(&W.dw, w);
            L.vec(&W.dwb, cp + ".2.bias", d);
        }
        {  // BatchNorm1d, eval: y = (x - mean) / sqrt(var + eps) * w + b = x s + t
            for (const char* nm : {".3.weight", ".3.bias", ".3.running_mean", ".3.running_var"}) K.seen.insert(cp + nm);
            const float* g = L.need(cp + ".3.weight", d);
            const float* bb = L.need(cp + ".3.bias", d);
            const float* mu = L.need(cp + ".3.running_mean", d);
            const float* var = L.need(cp + ".3.running_var", d);
            std::vector<float> s((size_t)d, 0.f), t((size_t)d, 0.f);
            if (g && bb && mu && var)
                for (int c = 0; c < d; ++c) {
                    const double sc = (double)g[c] / std::sqrt((double)var[c] + 1e-5);
                    s[c] = (float)sc;
                    t[c] = (float)((double)bb[c] - (double)mu[c] * sc);
                }
            L.raw(&W.bns, s);
            L.raw(&W.bnt, t);
        }
    }
    // a key under the module's prefixes that the model does not have is an error (buffers that carry no parameter excepted)
    for (int64_t i = 0; i < n_tensors; ++i) {
        if (!tensors[i].name) continue;
        const std::string nm(tensors[i].name);
        const bool ours = wrapped ? (nm.rfind("cond_input_layer.", 0) == 0 || nm.rfind("cond_encoder.", 0) == 0 || nm.rfind("cond_output_layer.", 0) == 0)
                                  : nm.rfind("layers.", 0) == 0;
        if (!ours || K.seen.count(nm)) continue;
        const bool buffer = nm.size() >= 19 && nm.compare(nm.size() - 19, 19, "num_batches_tracked") == 0;
        if (buffer || nm == root + "rotary_embedding.inv_freq") continue;
        set_error("condition encoder: unexpected tensor '%s' (qk_norm and joint attention are not supported)", nm.c_str());
        return QA_ERR_INVALID;
    }
    // RotaryEmbedding(dim_head).forward_from_seq_len: inv_freq = 10000^(-2i / dim_head), angle = t * inv_freq in fp32
    const int half = hd / 2;
    std::vector<float> cs((size_t)CF_MAX_POS * half * 2);
    for (int i = 0; i < half; ++i) {
        const float inv = 1.0f / std::pow(10000.0f, (float)(2 * i) / (float)hd);
        for (int t = 0; t < CF_MAX_POS; ++t) {
            const float fr = (float)t * inv;
            cs[((size_t)t * half + i) * 2] = (float)std::cos((double)fr);
            cs[((size_t)t * half + i) * 2 + 1] = (float)std::sin((double)fr);
        }
    }
    L.raw(&h->rope, cs);
    return L.upload();
}

struct CfTemps {
    float *hn, *u, *v;
};

int feed_forward_op(Ctx& c, const FeedForwardW& f, float* x, const CfTemps& t, int64_t rows, int d) {
    QA_TRY(layernorm_op(c, x, f.lnw, f.lnb, t.hn, rows, d, 1e-5f));
    QA_TRY(linear_op(c, t.hn, rows, f.l1, t.u, epi(ACT_SILU)));
    return linear_op(c, t.u, rows, f.l2h, x, epi(ACT_NONE, x));
}

// the ConformerEncoder in place on x [B, T, dim].  mask: the reference's key-padding mask (bytes [B, T], device) or null.  lens (device int
// [B], null in every call without lengths; never together with mask): item b holds lens[b] of the T frames and comes
// out as it would alone at that length - the keys behind are invisible (the byte image of the lengths takes the mask's place in the
// attention and in masked_add), the convolution module's zero padding starts at lens[b], and the rows behind are zeros on entry (so that
// whatever the caller left there, NaN included, never reaches a product with an attention weight of 0) and zeros on return.  The per-frame
// stages stay rectangular: a GEMM or LayerNorm row depends on its own input row alone.
int encoder_graph(qa_cond_encoder* h, Ctx& c, float* x, const unsigned char* mask, const int* lens, int B, int T) {
    const qa_cond_encoder_spec& sp = h->spec;
    const int d = sp.dim, H = sp.heads, hd = sp.dim_head, inner = H * hd;
    const int64_t rows = (int64_t)B * T;
    const size_t mark = c.arena.mark();
    CfTemps t;
    t.hn = c.arena.alloc<float>(rows * d);
    t.u = c.arena.alloc<float>(rows * std::max(std::max(d * sp.ff_mult, 2 * d), 3 * inner));
    t.v = c.arena.alloc<float>(rows * std::max(inner, d));
    AttnArgs at = attn_packed_qkv(t.u, t.v, B, T, H, hd);
    if (lens) {
        unsigned char* image = c.arena.alloc<unsigned char>((size_t)rows);
        QA_RUN(c, launch_len_mask(image, B, T, ClipLens{lens, 1}, c.stream));
        QA_RUN(c, launch_lm_rows_zero_pad(x, 0, 1, B, T, d, lens, c.stream));
        mask = image;
    }
    at.kvalid = mask;
    for (int l = 0; l < sp.n_layers; ++l) {
        const ConformerLayerW& W = h->layers[l];
        const std::string lp = "conformer." + std::to_string(l);
        QA_TRY(feed_forward_op(c, W.ff1, x, t, rows, d));
        c.tap(lp + ".ff1", x, rows * d);
        QA_TRY(layernorm_op(c, x, W.anw, W.anb, t.hn, rows, d, 1e-5f));
        QA_TRY(linear_op(c, t.hn, rows, W.qkv, t.u));
        QA_TRY(rope_op(c, t.u, h->rope, B, T, H, hd, 3 * inner, 0, sp.rope_interleaved, sp.pe_attn_head < 0 ? 0 : sp.pe_attn_head));
        QA_TRY(attention_op(c, at));
        QA_TRY(linear_op(c, t.v, rows, W.out, t.hn));
        QA_RUN(c, launch_masked_add(x, t.hn, mask, rows, d, c.stream));
        c.tap(lp + ".attn", t.hn, rows * d);
        QA_TRY(layernorm_op(c, x, W.cnw, W.cnb, t.hn, rows, d, 1e-5f));
        QA_TRY(linear_op(c, t.hn, rows, W.pw1, t.u));
        QA_RUN(c, launch_glu_dwconv_bn_silu(t.u, W.dw, W.dwb, W.bns, W.bnt, t.v, B, T, d, c.stream, lens));
        QA_TRY(linear_op(c, t.v, rows, W.pw2, x, epi(ACT_NONE, x)));
        c.tap(lp + ".conv", x, rows * d);
        QA_TRY(feed_forward_op(c, W.ff2, x, t, rows, d));
        QA_TRY(layernorm_op(c, x, W.fnw, W.fnb, x, rows, d, 1e-5f));
        c.tap(lp + ".out", x, rows * d);
    }
    if (lens) QA_RUN(c, launch_lm_rows_zero_pad(x, 0, 1, B, T, d, lens, c.stream));  // the last LayerNorm made non-zero rows out of zeros
    c.arena.release(mark);
    return QA_OK;
}

// a batch item without a valid key has no attention output (the reference yields NaN): refused.  One small copy and one wait, masked calls only.
int check_mask(qa_cond_encoder* h, const unsigned char* mask, int B, int T, hipStream_t s) {
    QA_REQUIRE(!stream_capturing(s), "condition encoder: a masked call waits for its mask check on the host and cannot run under a "
               "stream capture (check the mask beforehand and pass the valid items unmasked, or call outside the capture)");
    if (B > h->host_cap) {
        if (h->host_counts) QA_HIP(hipHostFree(h->host_counts));
        h->host_counts = nullptr;
        h->host_cap = 0;
        QA_HIP(hipHostMalloc(reinterpret_cast<void**>(&h->host_counts), sizeof(int) * (size_t)B));
        h->host_cap = B;
    }
    // the counters borrow the front of the planned workspace: the wait below ends before run_planned may reuse or reallocate it
    QA_TRY(h->ws.ensure(sizeof(int) * (size_t)B));
    int* counts = reinterpret_cast<int*>(h->ws.ptr);
    QA_TRY(launch_mask_count(mask, B, T, counts, s));
    QA_HIP(hipMemcpyAsync(h->host_counts, counts, sizeof(int) * (size_t)B, hipMemcpyDeviceToHost, s));
    QA_HIP(hipStreamSynchronize(s));
    for (int b = 0; b < B; ++b)
        QA_REQUIRE(h->host_counts[b] > 0, "condition encoder: batch item %d has no valid position in its mask (the reference yields NaN there)", b);
    return QA_OK;
}

int forward_checks(qa_cond_encoder* h, const char* fn, const void* x, const void* out, int64_t B, int64_t T, bool wrapped) {
    if (!h || !x || !out) {
        set_error("%s: null argument", fn);
        return QA_ERR_INVALID;
    }
    QA_REQUIRE((h->spec.cond_dim > 0) == wrapped, wrapped ? "%s: this handle is a bare ConformerEncoder, use qa_conformer_forward"
                                                          : "%s: this handle is a condition encoder, use qa_cond_encoder_forward", fn);
    const int64_t wide = std::max<int64_t>(std::max(h->spec.dim * h->spec.ff_mult, 3 * h->spec.heads * h->spec.dim_head), h->spec.hidden_out);
    QA_REQUIRE(B > 0 && B < 65536 && T > 0 && T <= CF_MAX_POS && B * T * wide < (1LL << 31), "%s: input is [%lld, %lld, .] (T <= %d)", fn,
               (long long)B, (long long)T, CF_MAX_POS);
    return QA_OK;
}

// The length vector of a _ragged call (HOST int64 [B], 1 .. T frames each; null: none) -> *dev, the device copy the graph reads, or null
// when the call is the rectangular one (no vector, or every entry equal to T).  Everything is checked before the first launch, on the host
// alone: where a masked call reads its counters back and waits, a call with lengths does not.
int upload_lengths(qa_cond_encoder* h, const char* fn, const int64_t* lengths, int64_t B, int64_t T, hipStream_t s, const int** dev) {
    *dev = nullptr;
    if (!lengths) return QA_OK;
    QA_TRY(refuse_capture(fn, s, LENGTHS_ARE_HOST_DATA));
    std::vector<int> v;
    bool full = true;
    const int64_t bad = check_row_lengths(lengths, B, 1, T, &v, &full);
    QA_REQUIRE(bad < 0, "%s: lengths[%lld] = %lld is outside 1 .. T = %lld frames", fn, (long long)bad, (long long)lengths[bad], (long long)T);
    return full ? QA_OK : h->lens.upload({&v}, s, dev);
}

// qa_conformer_forward(_ragged): at most one of mask and lengths
int conformer_call(qa_cond_encoder* h, const char* fn, const float* x, const uint8_t* mask, const int64_t* lengths, int64_t B, int64_t T,
                   float* out, void* stream) {
    QA_TRY(forward_checks(h, fn, x, out, B, T, false));
    hipStream_t s = static_cast<hipStream_t>(stream);
    QA_HIP(hipSetDevice(h->device));
    const int* lens = nullptr;
    QA_TRY(upload_lengths(h, fn, lengths, B, T, s, &lens));
    if (mask) QA_TRY(check_mask(h, mask, (int)B, (int)T, s));
    const int64_t n = B * T * h->spec.dim;
    return run_planned(*h, stream, [&]() -> int {
        // real pass only, more than a launch: the copy of the input the encoder then updates in place
        if (!h->ctx.dry && out != x) QA_HIP(hipMemcpyAsync(out, x, sizeof(float) * n, hipMemcpyDeviceToDevice, s));
        return encoder_graph(h, h->ctx, out, mask, lens, (int)B, (int)T);
    });
}

int cond_encoder_call(qa_cond_encoder* h, const char* fn, const float* mel, const uint8_t* mask, const int64_t* lengths, int64_t B, int64_t T,
                      float* out, void* stream) {
    QA_TRY(forward_checks(h, fn, mel, out, B, T, true));
    hipStream_t s = static_cast<hipStream_t>(stream);
    QA_HIP(hipSetDevice(h->device));
    const int* lens = nullptr;
    QA_TRY(upload_lengths(h, fn, lengths, B, T, s, &lens));
    if (mask) QA_TRY(check_mask(h, mask, (int)B, (int)T, s));
    const int64_t rows = B * T;
    return run_planned(*h, stream, [&]() -> int {
        Ctx& c = h->ctx;
        float* x = c.arena.alloc<float>(rows * h->spec.dim);
        QA_TRY(linear_op(c, mel, rows, h->in_layer, x));
        QA_TRY(encoder_graph(h, c, x, mask, lens, (int)B, (int)T));
        QA_TRY(linear_op(c, x, rows, h->out_layer, out));
        // the biased Linear made non-zero rows out of the zeros behind an item's frames
        if (lens) QA_RUN(c, launch_lm_rows_zero_pad(out, 0, 1, (int)B, (int)T, h->spec.hidden_out, lens, c.stream));
        return QA_OK;
    });
}

// ---------------------------------------------------------------- log-mel front

struct LogMel {
    WeightStore store;
    Workspace ws;
    Ctx ctx;
    ConvW dft, fbank;
    int nb = 0, nbp = 0, kp = 0, hop = 0, win = 0, n_mels = 0;
    DeviceInts lens{2};  // qa_logmel_ragged: the rows' samples and frames
    std::mutex mu;
};
typedef std::tuple<int, int, int, int, int, int, float, float> LogMelKey;
std::mutex g_logmel_mu;
std::map<LogMelKey, LogMel*> g_logmel;  // per (device, parameters); lives as long as the process

int build_logmel(LogMel* m, int n_fft, int win, int hop, int n_mels, int sr, double fmin, double fmax) {
    m->hop = hop; m->win = win; m->n_mels = n_mels;
    m->nb = n_fft / 2 + 1;
    m->nbp = (int)round_up(m->nb, 4);
    m->kp = (int)round_up(m->nb, 32);
    HostTable tab(nullptr, 0);
    Loader L(tab, m->store);
    {
        const int off = (n_fft - win) / 2;
        std::vector<float> w((size_t)2 * m->nbp * win, 0.f);
        const double two_pi = 6.283185307179586476925;
        for (int jj = 0; jj < win; ++jj) {
            const double wj = 0.5 - 0.5 * std::cos(two_pi * jj / win);  // periodic Hann (torch.hann_window)
            for (int k = 0; k < m->nb; ++k) {
                const long long ph = ((long long)k * (off + jj)) % n_fft;  // exact phase reduction
                const double a = two_pi * (double)ph / n_fft;
                w[(size_t)k * win + jj] = (float)(wj * std::cos(a));
                w[(size_t)(m->nbp + k) * win + jj] = (float)(-wj * std::sin(a));
            }
        }
        // library layout [N][ksize][C_in] with tap j, channel c <-> window sample j * hop + c
        m->dft.N = 2 * m->nbp; m->dft.C_in = hop; m->dft.ksize = 2;
        L.raw(&m->dft.w, w);
    }
    {  // torchaudio.functional.melscale_fbanks(mel_scale="htk", norm=None)
        auto hz2mel = [](double f) { return 2595.0 * std::log10(1.0 + f / 700.0); };
        std::vector<double> fpts(n_mels + 2);
        const double m0 = hz2mel(fmin), m1 = hz2mel(fmax);
        for (int i = 0; i < n_mels + 2; ++i) fpts[i] = 700.0 * (std::pow(10.0, (m0 + (m1 - m0) * i / (n_mels + 1)) / 2595.0) - 1.0);
        std::vector<float> fb((size_t)n_mels * m->kp, 0.f);
        for (int k = 0; k < m->nb; ++k) {
            const double f = (double)(sr / 2) * k / (m->nb - 1);
            for (int i = 0; i < n_mels; ++i) {
                const double down = (f - fpts[i]) / (fpts[i + 1] - fpts[i]), up = (fpts[i + 2] - f) / (fpts[i + 2] - fpts[i + 1]);
                fb[(size_t)i * m->kp + k] = (float)std::max(0.0, std::min(down, up));
            }
        }
        m->fbank.N = n_mels; m->fbank.C_in = m->kp; m->fbank.ksize = 1;
        L.raw(&m->fbank.w, fb);
    }
    return L.upload();
}

}  // namespace

extern "C" {

int qa_cond_encoder_create(qa_cond_encoder** out, const qa_cond_encoder_spec* spec, const qa_tensor* tensors, int64_t n_tensors, int device) {
    if (!out || !spec || !tensors) {
        set_error("qa_cond_encoder_create: null argument");
        return QA_ERR_INVALID;
    }
    *out = nullptr;
    const qa_cond_encoder_spec& sp = *spec;
    QA_REQUIRE(sp.qk_norm == 0, "qa_cond_encoder_create: qk_norm = \"rms_norm\" is not supported (the shipped configuration has qk_norm: null)");
    QA_REQUIRE(sp.dw_kernel >= 1 && (sp.dw_kernel - 1) % 2 == 0,
               "qa_cond_encoder_create: depthwise_kernel_size must be odd to achieve 'SAME' padding (got %d)", sp.dw_kernel);
    QA_REQUIRE(sp.dw_kernel <= CF_MAX_K, "qa_cond_encoder_create: depthwise kernel size %d above %d", sp.dw_kernel, CF_MAX_K);
    QA_REQUIRE(sp.dim > 0 && sp.dim % 32 == 0 && sp.n_layers > 0 && sp.heads > 0 && sp.ff_mult > 0 && sp.dim <= 2048,
               "qa_cond_encoder_create: dim %d must be a positive multiple of 32 (<= 2048), layers / heads / ff_mult positive", sp.dim);
    QA_REQUIRE(sp.dim_head == 32 || sp.dim_head == 64 || sp.dim_head == 96 || sp.dim_head == 128,
               "qa_cond_encoder_create: dim_head %d unsupported (32/64/96/128)", sp.dim_head);
    QA_REQUIRE(sp.pe_attn_head == -1 || (sp.pe_attn_head >= 1 && sp.pe_attn_head <= sp.heads),
               "qa_cond_encoder_create: pe_attn_head %d outside 1 .. %d (-1 = all heads)", sp.pe_attn_head, sp.heads);
    QA_REQUIRE(sp.rope_interleaved == 0 || sp.rope_interleaved == 1, "qa_cond_encoder_create: rope_interleaved must be 0 or 1");
    QA_REQUIRE((sp.cond_dim == 0 && sp.hidden_out == 0) || (sp.cond_dim > 0 && sp.cond_dim % 16 == 0 && sp.hidden_out > 0 && sp.hidden_out % 4 == 0),
               "qa_cond_encoder_create: cond_dim %d must be a multiple of 16 and hidden_out %d a multiple of 4 (both 0: the bare ConformerEncoder)",
               sp.cond_dim, sp.hidden_out);
    QA_HIP(hipSetDevice(device));
    std::unique_ptr<qa_cond_encoder> h(new qa_cond_encoder());
    h->spec = sp;
    h->device = device;
    QA_TRY(build_encoder(h.get(), tensors, n_tensors));
    *out = h.release();
    return QA_OK;
}

void qa_cond_encoder_destroy(qa_cond_encoder* h) { destroy_handle(h); }

int qa_conformer_forward(qa_cond_encoder* h, const float* x, const uint8_t* mask, int64_t B, int64_t T, float* out, void* stream) {
    return conformer_call(h, "qa_conformer_forward", x, mask, nullptr, B, T, out, stream);
}

int qa_conformer_forward_ragged(qa_cond_encoder* h, const float* x, const int64_t* lengths, int64_t B, int64_t T, float* out, void* stream) {
    return conformer_call(h, "qa_conformer_forward_ragged", x, nullptr, lengths, B, T, out, stream);
}

int qa_cond_encoder_forward(qa_cond_encoder* h, const float* mel, const uint8_t* mask, int64_t B, int64_t T, float* out, void* stream) {
    return cond_encoder_call(h, "qa_cond_encoder_forward", mel, mask, nullptr, B, T, out, stream);
}

int qa_cond_encoder_forward_ragged(qa_cond_encoder* h, const float* mel, const int64_t* lengths, int64_t B, int64_t T, float* out,
                                   void* stream) {
    return cond_encoder_call(h, "qa_cond_encoder_forward_ragged", mel, nullptr, lengths, B, T, out, stream);
}

int qa_cond_encoder_enable_taps(qa_cond_encoder* h, int on) { return taps_enable(h ? &h->ctx : nullptr, "qa_cond_encoder_enable_taps", on); }

int64_t qa_cond_encoder_tap(qa_cond_encoder* h, const char* name, float* dst, int64_t cap, void* stream) {
    return tap_read(h ? &h->ctx : nullptr, "qa_cond_encoder_tap", name, dst, cap, stream);
}

int64_t qa_logmel_frames(int64_t n, int32_t hop_length) { return (n <= 0 || hop_length <= 0) ? (int64_t)QA_ERR_INVALID : (n + hop_length - 1) / hop_length; }

// qa_logmel (lengths == nullptr) and qa_logmel_ragged.  Everything is checked before the first launch; a call whose rows all hold n samples
// is the rectangular call as it is: nothing uploaded, the same launches.
static int logmel_call(const char* fn, const float* wav, const int64_t* lengths, int64_t B, int64_t n, int32_t n_fft, int32_t win_length,
                       int32_t hop_length, int32_t n_mels, int32_t sample_rate, float f_min, float f_max, float* out, void* stream) {
    if (!wav || !out) {
        set_error("%s: null argument", fn);
        return QA_ERR_INVALID;
    }
    QA_REQUIRE(hop_length >= 16 && hop_length % 16 == 0 && win_length == 2 * hop_length && n_fft >= win_length && (n_fft - win_length) % 2 == 0,
               "%s: the framed-signal DFT needs win_length = 2 * hop_length, hop a multiple of 16, n_fft >= win_length (got n_fft %d, "
               "win %d, hop %d)", fn, n_fft, win_length, hop_length);
    QA_REQUIRE(n_mels > 0 && n_mels % 4 == 0 && sample_rate > 0 && f_min >= 0.f && f_max > f_min && f_max <= sample_rate / 2,
               "%s: n_mels %d (a multiple of 4), band %g - %g Hz at %d Hz", fn, n_mels, f_min, f_max, sample_rate);
    const int64_t nf = (n + hop_length - 1) / hop_length;
    QA_REQUIRE(B > 0 && B < 65536 && n > 0 && B * (nf + 1) * (int64_t)std::max(hop_length, n_fft + 8) < (1LL << 31), "%s: wav is [%lld, %lld]", fn,
               (long long)B, (long long)n);
    std::vector<int> samples, frames;
    bool full = true;
    if (lengths) {
        QA_TRY(refuse_capture(fn, static_cast<hipStream_t>(stream), LENGTHS_ARE_HOST_DATA));
        const int64_t bad = check_row_lengths(lengths, B, 1, n, &samples, &full);
        QA_REQUIRE(bad < 0, "%s: lengths[%lld] = %lld is outside 1 .. n = %lld samples", fn, (long long)bad, (long long)lengths[bad], (long long)n);
        for (int v : samples) frames.push_back((v + hop_length - 1) / hop_length);
    }
    int device = 0;
    QA_HIP(hipGetDevice(&device));
    LogMel* m = nullptr;
    {
        std::lock_guard<std::mutex> lock(g_logmel_mu);
        const LogMelKey key(device, n_fft, win_length, hop_length, n_mels, sample_rate, f_min, f_max);
        auto it = g_logmel.find(key);
        if (it == g_logmel.end()) {
            std::unique_ptr<LogMel> fresh(new LogMel());
            QA_TRY(build_logmel(fresh.get(), n_fft, win_length, hop_length, n_mels, sample_rate, f_min, f_max));
            it = g_logmel.emplace(key, fresh.release()).first;
        }
        m = it->second;
    }
    std::lock_guard<std::mutex> lock(m->mu);
    Ctx& c = m->ctx;
    const int64_t rows = B * nf;
    const int* lens[2] = {nullptr, nullptr};  // device: the rows' samples, the rows' frames
    if (!full) QA_TRY(m->lens.upload({&samples, &frames}, static_cast<hipStream_t>(stream), lens));
    auto graph = [&]() -> int {
        float* P = c.arena.alloc<float>((size_t)B * (nf + 1) * m->hop);
        float* ri = c.arena.alloc<float>((size_t)rows * 2 * m->nbp);
        float* mag = c.arena.alloc<float>((size_t)rows * m->kp);
        QA_RUN(c, launch_logmel_frames(wav, (int)B, n, (m->win - m->hop) / 2, (nf + 1) * m->hop, P, c.stream, lens[0]));
        QA_TRY(conv_op(c, P, m->hop, (int)B, (int)nf + 1, m->dft, ri, 2 * m->nbp, (int)nf, ConvOpt()));
        QA_RUN(c, launch_spec_mag(ri, m->nbp, m->nb, mag, m->kp, rows, c.stream));
        QA_TRY(linear_op(c, mag, rows, m->fbank, out));
        QA_RUN(c, launch_log_eps(out, rows * m->n_mels, 1e-10f, c.stream, lens[1], (int)nf, m->n_mels));  // and the zeros behind a row's frames
        return QA_OK;
    };
    QA_TRY(plan(device, static_cast<hipStream_t>(stream), c, m->ws, graph));
    return graph();
}

int qa_logmel(const float* wav, int64_t B, int64_t n, int32_t n_fft, int32_t win_length, int32_t hop_length, int32_t n_mels, int32_t sample_rate,
              float f_min, float f_max, float* out, void* stream) {
    return logmel_call("qa_logmel", wav, nullptr, B, n, n_fft, win_length, hop_length, n_mels, sample_rate, f_min, f_max, out, stream);
}

int qa_logmel_ragged(const float* wav, const int64_t* lengths, int64_t B, int64_t n, int32_t n_fft, int32_t win_length, int32_t hop_length,
                     int32_t n_mels, int32_t sample_rate, float f_min, float f_max, float* out, void* stream) {
    return logmel_call("qa_logmel_ragged", wav, lengths, B, n, n_fft, win_length, hop_length, n_mels, sample_rate, f_min, f_max, out, stream);
}

}  // extern "C"
