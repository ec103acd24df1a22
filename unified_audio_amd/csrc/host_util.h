// host_util.h - host-side plumbing shared by the model graphs: weight-table lookup, the folded-weight store and its loader,
// the per-call bump arena, the workspace and the planning / execution context, the convolution launcher, the planning-pass gate of
// every other launch (QA_RUN and the shared ops), test taps and the resources every model handle owns.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "kernels.h"
#include "split_planes.h"

namespace qa {

// name -> host tensor view of the caller's state_dict
class HostTable {
   public:
    HostTable(const qa_tensor* t, int64_t n) {
        for (int64_t i = 0; i < n; ++i)
            if (t[i].name && t[i].data) map_[t[i].name] = &t[i];
    }
    // nullptr + error message when absent or mis-sized
    const float* get(const std::string& name, int64_t numel) const {
        auto it = map_.find(name);
        if (it == map_.end()) {
            set_error("weight table: missing tensor '%s'", name.c_str());
            return nullptr;
        }
        if (it->second->numel != numel) {
            set_error("weight table: tensor '%s' has %lld elements, expected %lld", name.c_str(),
                      (long long)it->second->numel, (long long)numel);
            return nullptr;
        }
        return it->second->data;
    }
    bool has(const std::string& name) const { return map_.count(name) != 0; }

   private:
    std::unordered_map<std::string, const qa_tensor*> map_;
};

// Folded weights are appended to one host blob (64-float aligned) and uploaded with a single copy.  upload() also builds the
// pre-split image of the whole blob (split_planes.h: 6 bytes per weight beside the 4 of the fp32 blob, padding, biases and raw()
// vectors included, so that the planes of any stored weight follow from its address) and attaches it for conv_gemm's split-6
// launches - unless `planes` is off (a handle whose conv_gemm launches all keep the fp32 chain) or QA_GEMM_PRESPLIT is 0 at load time.
// The fp32 blob stays: the fp32 chain and every kernel that is not conv_gemm read it.
class WeightStore {
   public:
    WeightStore() = default;
    WeightStore(const WeightStore&) = delete;
    WeightStore& operator=(const WeightStore&) = delete;
    ~WeightStore() {
        if (planes_attached_) weight_planes_detach(dev_);
        if (planes_) (void)hipFree(planes_);
        if (dev_) (void)hipFree(dev_);
    }
    bool planes = true;
    size_t add(const std::vector<float>& v) { return add(v.data(), v.size()); }
    size_t add(const float* p, size_t n) {
        const size_t off = blob_.size();
        blob_.insert(blob_.end(), p, p + n);
        blob_.resize(round_up((int64_t)blob_.size(), 64), 0.f);
        return off;
    }
    int upload() {
        const size_t n = blob_.size();
        QA_HIP(hipMalloc(&dev_, n * sizeof(float)));
        QA_HIP(hipMemcpy(dev_, blob_.data(), n * sizeof(float), hipMemcpyHostToDevice));
        bytes_ = n * sizeof(float);
        std::vector<float>().swap(blob_);
        if (planes && n > 0 && knob(K_GEMM_PRESPLIT) != 0) {
            if (hipMalloc(&planes_, n / 8 * PLANE_GROUP_BYTES) != hipSuccess) {
                // no room for the image: the model still loads and every launch splits in the loop - same kernels, same bits
                (void)hipGetLastError();
                planes_ = nullptr;
                return QA_OK;
            }
            QA_TRY(launch_weight_planes(dev_, (long long)n, planes_, nullptr));
            QA_HIP(hipStreamSynchronize(nullptr));  // the handle's calls run on the caller's streams
            QA_TRY(weight_planes_attach(dev_, (long long)n, planes_));
            planes_attached_ = true;
        }
        return QA_OK;
    }
    const float* ptr(size_t off) const { return dev_ + off; }
    size_t bytes() const { return bytes_; }

   private:
    std::vector<float> blob_;
    float* dev_ = nullptr;
    void* planes_ = nullptr;
    bool planes_attached_ = false;
    size_t bytes_ = 0;
};

// Bump allocator over one device buffer.  In planning mode (base == nullptr) it only tracks the peak.
class Arena {
   public:
    void begin(char* base, size_t cap) {
        base_ = base;
        cap_ = cap;
        off_ = 0;
        peak_ = 0;
        floor_ = 0;
    }
    template <typename T>
    T* alloc(size_t n) {
        const size_t bytes = (size_t)round_up((int64_t)(n * sizeof(T)), 256);
        const size_t at = off_;
        off_ += bytes;
        if (off_ > peak_) peak_ = off_;
        return base_ ? reinterpret_cast<T*>(base_ + at) : reinterpret_cast<T*>(uintptr_t(4096) + at);
    }
    size_t mark() const { return off_; }
    void release(size_t m) { off_ = m > floor_ ? m : floor_; }
    // everything allocated so far survives later release() calls (test taps snapshot buffers inside a mark / release region)
    void pin() { floor_ = off_; }
    size_t peak() const { return peak_; }
    bool planning() const { return base_ == nullptr; }

   private:
    char* base_ = nullptr;
    size_t cap_ = 0, off_ = 0, peak_ = 0, floor_ = 0;
};

// A device buffer that only grows: ensure() frees the old buffer (hipFree waits for the work still reading it) and allocates the
// request plus 1/8 headroom.
struct Workspace {
    char* ptr = nullptr;
    size_t cap = 0;
    Workspace() = default;
    Workspace(const Workspace&) = delete;
    Workspace& operator=(const Workspace&) = delete;
    ~Workspace() {
        if (ptr) (void)hipFree(ptr);
    }
    int ensure(size_t bytes) {
        if (bytes <= cap) return QA_OK;
        if (ptr) QA_HIP(hipFree(ptr));
        ptr = nullptr;
        cap = 0;
        const size_t grown = bytes + bytes / 8;
        QA_HIP(hipMalloc(reinterpret_cast<void**>(&ptr), grown));
        cap = grown;
        return QA_OK;
    }
};

// The host integers of a call with per-row lengths on their way to the kernels: a handle-owned device array of
// `slots` vectors of up to `cap` ints each, written on the call's stream by launch_row_ints.  It only grows, by whole multiples of
// ROW_INTS_CHUNK rows; hipFree waits for the work that still reads the old array.
struct DeviceInts {
    int* dev = nullptr;
    int cap = 0;
    const int slots;
    explicit DeviceInts(int slots = 1) : slots(slots) {}
    DeviceInts(const DeviceInts&) = delete;
    DeviceInts& operator=(const DeviceInts&) = delete;
    ~DeviceInts() {
        if (dev) (void)hipFree(dev);
    }
    // ALL the vectors of one call, each of the same B host ints: out[i] = the device copy of *src[i], i < src.size() <= slots.  The
    // array grows at most once and before anything is written, so no vector of the call can land in an array that the same call frees.
    int upload(const std::vector<const std::vector<int>*>& src, hipStream_t stream, const int** out) {
        const size_t k = src.size(), B = k ? src[0]->size() : 0;
        bool same = k >= 1 && k <= (size_t)slots && B >= 1 && B < ((size_t)1 << 30);
        for (size_t i = 1; same && i < k; ++i) same = src[i]->size() == B;
        QA_REQUIRE(same, "DeviceInts: %zu vectors of %zu ints into %d slots", k, B, slots);
        if (B > (size_t)cap) {
            if (dev) QA_HIP(hipFree(dev));
            dev = nullptr;
            cap = 0;
            const int grown = (int)round_up((int64_t)B, ROW_INTS_CHUNK);
            QA_HIP(hipMalloc(reinterpret_cast<void**>(&dev), sizeof(int) * (size_t)grown * slots));
            cap = grown;
        }
        for (size_t i = 0; i < k; ++i) {
            QA_TRY(launch_row_ints(dev + i * cap, src[i]->data(), (long long)B, stream));
            out[i] = dev + i * cap;
        }
        return QA_OK;
    }
};

// One float buffer of a handle's own that lives across calls, outside the arena: the streaming and cache states.  release() first waits for
// the device - the steps that still read the buffer - and the caller has set the device, on every path that ends in it (the destructor too).
struct DeviceFloats {
    float* ptr = nullptr;
    DeviceFloats() = default;
    DeviceFloats(const DeviceFloats&) = delete;
    DeviceFloats& operator=(const DeviceFloats&) = delete;
    ~DeviceFloats() { release(); }
    // n floats in place of what it held, not cleared
    int allocate(size_t n) {
        release();
        QA_HIP(hipMalloc(reinterpret_cast<void**>(&ptr), sizeof(float) * n));
        return QA_OK;
    }
    void release() {
        if (!ptr) return;
        (void)hipDeviceSynchronize();
        (void)hipFree(ptr);
        ptr = nullptr;
    }
};

struct Tap {
    const float* ptr;
    int64_t numel;
};

struct Ctx {
    Arena arena;
    hipStream_t stream = nullptr;
    bool dry = false;      // planning pass: allocate, do not launch
    bool gemm_fp32 = false;  // conv_op launches keep conv_gemm's fp32 chain (ConvParams::math_fp32)
    bool att_fp32 = false;   // attention_op launches keep the fp32 form of attention_kernel (SPLIT = false) (set wherever gemm_fp32 is)
    bool capture = false;  // test hook: snapshot named intermediates (buffers are reused / updated in place later)
    std::unordered_map<std::string, Tap> taps;
    void tap(const std::string& name, const float* p, int64_t n) {
        if (!capture) return;
        float* copy = arena.alloc<float>((size_t)n);
        arena.pin();  // the snapshot must outlive the mark / release region it was taken in
        if (dry) return;
        (void)hipMemcpyAsync(copy, p, sizeof(float) * (size_t)n, hipMemcpyDeviceToDevice, stream);
        taps[name] = Tap{copy, n};
    }
};

// A folded convolution / linear layer in library layout [N][ksize][C_in].
struct ConvW {
    const float* w = nullptr;
    const float* b = nullptr;
    int N = 0, C_in = 0, ksize = 1;
    int algo_n = 0, algo_cin = 0;  // un-padded sizes (0 = same as N / C_in)
};

inline int pad32(int c) { return (int)round_up(c, 32); }

// ---------------------------------------------------------------- weight loading

// How a layer's weight is stored in the state_dict: a plain `.weight`, torch.nn.utils.weight_norm's `.weight_g` / `.weight_v`, or
// whichever of the two the table holds.
enum { WN_NONE = 0, WN_FOLD = 1, WN_DETECT = 2 };

// Folds tensors of a HostTable into a WeightStore.  Every fold records where its data lands; upload() copies the store to the device
// and points the recorded destinations at it.  A missing or mis-sized tensor fails the load (QA_ERR_MISSING), and qa_last_error()
// names it.
class Loader {
   public:
    Loader(const HostTable& tab, WeightStore& store, int wn = WN_NONE) : tab(tab), wn(wn), store_(store) {}

    const HostTable& tab;
    int wn;  // the weight-norm mode of weight() and conv()

    const float* need(const std::string& name, int64_t numel) {
        const float* p = tab.get(name, numel);
        if (!p) ok_ = false;
        return p;
    }
    void vec(const float** dst, const std::string& name, int64_t n) {
        const float* p = need(name, n);
        if (p) pend_.push_back({dst, store_.add(p, (size_t)n)});
    }
    void raw(const float** dst, const std::vector<float>& v) { pend_.push_back({dst, store_.add(v)}); }
    // nn.Linear [N][C_in] as it is stored (never weight-normed: `wn` does not apply); bias_key empty: no bias
    void linear(ConvW* dst, const std::string& weight_key, const std::string& bias_key, int N, int C_in) {
        dst->N = N;
        dst->C_in = C_in;
        dst->ksize = 1;
        vec(&dst->w, weight_key, (int64_t)N * C_in);
        if (!bias_key.empty()) vec(&dst->b, bias_key, N);
    }
    // the `.weight` / `.bias` pair of a normalisation over d channels
    void norm(const float** w, const float** b, const std::string& prefix, int d) {
        vec(w, prefix + ".weight", d);
        vec(b, prefix + ".bias", d);
    }
    // the [d0][rest] weight of prefix p; weight norm over dim 0 is folded as torch._weight_norm does it: w = v * (g / ||v||_2), the
    // sum of squares in double, the scale in fp32
    bool weight(const std::string& p, int64_t d0, int64_t rest, std::vector<float>* out) {
        out->assign((size_t)(d0 * rest), 0.f);
        const int mode = wn == WN_DETECT ? (tab.has(p + ".weight") ? WN_NONE : WN_FOLD) : wn;
        if (mode == WN_NONE) {
            const float* w = need(p + ".weight", d0 * rest);
            if (!w) return false;
            std::memcpy(out->data(), w, sizeof(float) * (size_t)(d0 * rest));
            return true;
        }
        const float* v = need(p + ".weight_v", d0 * rest);
        const float* g = need(p + ".weight_g", d0);
        if (!v || !g) return false;
        for (int64_t i = 0; i < d0; ++i) {
            double ss = 0.0;
            for (int64_t j = 0; j < rest; ++j) ss += (double)v[i * rest + j] * v[i * rest + j];
            const float scale = g[i] / (float)std::sqrt(ss);
            for (int64_t j = 0; j < rest; ++j) (*out)[(size_t)(i * rest + j)] = v[i * rest + j] * scale;
        }
        return true;
    }
    // Conv1d / Linear weight [N][C_in][k] -> library layout [Np][k][Cp] scaled by `gain`, bias -> [Np]; Np / Cp > 0 zero-pad the
    // output / input channels (the un-padded sizes stay in algo_n / algo_cin)
    void conv(ConvW* dst, const std::string& p, int N, int C_in, int k, bool bias = true, float gain = 1.f, int Np = 0, int Cp = 0) {
        if (Np <= 0) Np = N;
        if (Cp <= 0) Cp = C_in;
        std::vector<float> w, r((size_t)Np * k * Cp, 0.f);
        if (weight(p, N, (int64_t)C_in * k, &w))
            for (int n = 0; n < N; ++n)
                for (int c = 0; c < C_in; ++c)
                    for (int j = 0; j < k; ++j) r[((size_t)n * k + j) * Cp + c] = w[((size_t)n * C_in + c) * k + j] * gain;
        dst->N = Np;
        dst->C_in = Cp;
        dst->ksize = k;
        dst->algo_n = N;
        dst->algo_cin = C_in;
        raw(&dst->w, r);
        if (bias) {
            std::vector<float> b(Np, 0.f);
            if (const float* bp = need(p + ".bias", N)) std::memcpy(b.data(), bp, sizeof(float) * N);
            raw(&dst->b, b);
        }
    }
    int upload() {
        if (!ok_) return QA_ERR_MISSING;
        QA_TRY(store_.upload());
        for (auto& pv : pend_) *pv.first = store_.ptr(pv.second);
        return QA_OK;
    }

   private:
    WeightStore& store_;
    bool ok_ = true;
    std::vector<std::pair<const float**, size_t>> pend_;
};

// ---------------------------------------------------------------- convolution launcher

// Everything of a conv_gemm launch that is not the operands' shapes.
struct ConvOpt {
    int stride = 1, pad_left = 0, pad_right = 0, pad_mode = PAD_ZERO;
    int dilation = 1;  // tap j reads frame t * stride - pad_left + j * dilation (zero padding only)
    int in_rep = 1;    // x read as x.repeat_interleave(in_rep) along frames
    int prologue = ACT_NONE, act = ACT_NONE, post_act = ACT_NONE;
    const float *gamma = nullptr, *res = nullptr, *gate = nullptr;
    int64_t ldr = 0;               // residual row stride (0: N)
    const float* shift = nullptr;  // per-channel constant added after gamma (the residual operand with row stride 0): BN after a ReLU
    // Snake (ConvParams::alpha) and the second, activated output y2
    const float *alpha = nullptr, *alpha2 = nullptr;
    float* y2 = nullptr;
    int64_t ldy2 = 0;
    // fused interleaved-pair RoPE on the first rope_n output channels (ConvParams::rope)
    const float* rope = nullptr;
    int rope_n = 0, rope_hd = 0, rope_T = 0, rope_pos0 = 0;
    ClipLens rl;  // per-clip lengths of a ragged call (ConvParams::lens / len_mul): clip b holds rl.n[b] * rl.mul input frames
};

// geometry only
inline ConvOpt conv_geom(int stride, int pad_left, int pad_right, int pad_mode = PAD_ZERO) {
    ConvOpt o;
    o.stride = stride;
    o.pad_left = pad_left;
    o.pad_right = pad_right;
    o.pad_mode = pad_mode;
    return o;
}
// the epilogue of a linear: activation, residual (row stride N), gamma, gate
inline ConvOpt epi(int act, const float* res = nullptr, const float* gamma = nullptr, const float* gate = nullptr) {
    ConvOpt o;
    o.act = act;
    o.res = res;
    o.gamma = gamma;
    o.gate = gate;
    return o;
}

// The time axis of a [B, T, C] activation in a model graph and what rides along with it: whether the model's convolutions are causal and,
// in a ragged call, the clips' lengths at this stage's rate (clip b holds rl.n[b] * rl.mul of the T frames; rl.n null: all T).
struct TimeAxis {
    int B = 0, T = 0;
    bool causal = false;
    ClipLens rl;
    int64_t rows() const { return (int64_t)B * T; }
    // the same clips at another stage of the graph: T_new frames, `rate` frames per unit of rl.n
    TimeAxis at(int T_new, int rate) const { return TimeAxis{B, T_new, causal, ClipLens{rl.n, rl.n ? rate : 0}}; }
};

// y [B, T_out, w.N] (row stride ldy) = conv(x [B, T_in, w.C_in] (row stride ldx), w) on the implicit GEMM; nothing in a dry pass
inline int conv_op(Ctx& c, const float* x, int64_t ldx, int B, int T_in, const ConvW& w, float* y, int64_t ldy, int T_out,
                   const ConvOpt& o) {
    if (c.dry) return QA_OK;
    qa_conv_args a{};
    a.x = x; a.w = w.w; a.bias = w.b; a.gamma = o.gamma; a.residual = o.res; a.gate = o.gate; a.y = y;
    a.B = B; a.T_in = T_in; a.C_in = w.C_in; a.T_out = T_out; a.N = w.N;
    a.ldx = ldx; a.ldy = ldy; a.ldr = o.ldr;
    a.ksize = w.ksize; a.stride = o.stride; a.pad_left = o.pad_left; a.pad_right = o.pad_right; a.pad_mode = o.pad_mode;
    a.prologue = o.prologue; a.act = o.act; a.post_act = o.post_act;
    a.in_rep = o.in_rep;
    ConvParams p;
    if (o.dilation > 1) {
        // conv_params_from_args checks the window span for a dense kernel: hand it the dense-equivalent paddings, then set the dilation
        a.pad_left = o.pad_left + (w.ksize - 1) * (o.dilation - 1);
        QA_TRY(conv_params_from_args(a, &p));
        p.pad_left = o.pad_left;
        const int max_pad = std::max(o.pad_left, o.pad_right);
        p.Lp = (p.T_in <= max_pad) ? max_pad + 1 : p.T_in;
        p.dilation = o.dilation;
    } else {
        QA_TRY(conv_params_from_args(a, &p));
    }
    p.algo_n = w.algo_n;
    p.algo_k = w.algo_cin ? w.algo_cin * w.ksize : 0;
    p.rope = o.rope; p.rope_n = o.rope_n; p.rope_hd = o.rope_hd; p.rope_T = o.rope_T; p.rope_pos0 = o.rope_pos0;
    p.alpha = o.alpha; p.y2 = o.y2; p.alpha2 = o.alpha2; p.ldy2 = o.ldy2;
    p.math_fp32 = c.gemm_fp32 ? 1 : 0;
    p.lens = o.rl.n; p.len_mul = o.rl.mul; p.max_pad = std::max(o.pad_left, o.pad_right);
    if (o.shift) {
        p.res = o.shift;
        p.ldr = 0;
    }
    return launch_conv_gemm(p, c.stream);
}

// plain linear over `rows` rows
inline int linear_op(Ctx& c, const float* x, int64_t rows, const ConvW& w, float* y, const ConvOpt& o = ConvOpt()) {
    return conv_op(c, x, w.C_in, 1, (int)rows, w, y, w.N, (int)rows, o);
}

// The gate of every other launch of a model graph: QA_RUN(c, launch_...(..., c.stream)) launches in the real pass and does nothing
// (its arguments are not even evaluated) in the planning pass, whose arena addresses are made up.  Taps and allocations still happen
// in both passes - they size the arena - only the launch is skipped.  A graph function touches the device through conv_op /
// linear_op, the ops below and QA_RUN alone, or inside a commented real-pass block.
#define QA_RUN(c, call) do { if (!(c).dry) QA_TRY(call); } while (0)

// The launchers that more than one model file issues, on c.stream and gated like conv_op (arguments as in kernels.h).
inline int layernorm_op(Ctx& c, const float* x, const float* w, const float* b, float* y, int64_t rows, int C, float eps) {
    return c.dry ? QA_OK : launch_layernorm(x, w, b, y, rows, C, eps, c.stream);
}
inline int rmsnorm_op(Ctx& c, const float* x, const float* w, float* y, int64_t rows, int C, float eps) {
    return c.dry ? QA_OK : launch_rmsnorm(x, w, y, rows, C, eps, c.stream);
}
inline int dwconv_op(Ctx& c, const float* x, const float* w_kc, const float* bias, const float* lnw, const float* lnb, float* y, int B,
                     int T, int C, int ksize, float eps, int pad_left = -1, ClipLens rl = ClipLens()) {
    return c.dry ? QA_OK : launch_dwconv(x, w_kc, bias, lnw, lnb, y, B, T, C, ksize, eps, c.stream, pad_left, rl);
}
inline int to_channel_last_op(Ctx& c, const float* x, long long sb, long long sc, long long st, float* y, int B, int C, int T) {
    return c.dry ? QA_OK : launch_to_channel_last(x, sb, sc, st, y, B, C, T, c.stream);
}
inline int rope_op(Ctx& c, float* qkv, const float* cos_sin, int B, int N, int H, int hd, long long ld, int pos0, int interleaved = 0,
                   int rot_heads = 0) {
    return c.dry ? QA_OK : launch_rope(qkv, cos_sin, B, N, H, hd, ld, pos0, c.stream, interleaved, rot_heads);
}
inline int attention_op(Ctx& c, AttnArgs a) {
    if (c.dry) return QA_OK;
    a.math_fp32 = c.att_fp32 || a.row_nq != nullptr;  // the chunk form with per-item counts exists in the fp32 form alone (section 34)
    return launch_attention(a, c.stream);
}

// ---------------------------------------------------------------- planning a call

// the real pass: launches on, the taps of the previous call dropped, the arena on the workspace
inline void arm(Ctx& c, Workspace& ws) {
    c.dry = false;
    c.taps.clear();
    c.arena.begin(ws.ptr, ws.cap);
}

struct NoPreGrow {
    int operator()(size_t) const { return QA_OK; }
};

// Set the device, run `graph` as the planning pass (allocations only), grow `ws` to the arena's peak and arm the real pass on it; the
// caller then runs `graph` again.  `pre_grow(bytes)` runs first whenever the workspace has to grow.
template <typename G, typename P = NoPreGrow>
int plan(int device, hipStream_t stream, Ctx& c, Workspace& ws, G&& graph, P&& pre_grow = P()) {
    QA_HIP(hipSetDevice(device));
    c.stream = stream;
    c.dry = true;
    c.arena.begin(nullptr, 0);
    QA_TRY(graph());
    if (c.arena.peak() > ws.cap) QA_TRY(pre_grow(c.arena.peak()));
    QA_TRY(ws.ensure(c.arena.peak()));
    arm(c, ws);
    return QA_OK;
}

// whether `s` is being captured into a hipGraph by its owner (a failed query clears the sticky error and counts as "no")
inline bool stream_capturing(hipStream_t s) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cs) == hipSuccess) return cs == hipStreamCaptureStatusActive;
    (void)hipGetLastError();
    return false;
}

// A call that reads host state cannot be recorded into a caller's graph: a replay would run with what the capture read.  Refused, with the
// reason.  CACHE_IS_HOST_STATE: length and batch of a cache (the session calls); LENGTHS_ARE_HOST_DATA: the length vectors of a call with
// per-row lengths.
constexpr const char* CACHE_IS_HOST_STATE = "the cache length is host state, a replayed graph would repeat the captured positions";
constexpr const char* LENGTHS_ARE_HOST_DATA =
    "the rows' lengths are host data read during the call, a replayed graph would repeat the captured lengths";
inline int refuse_capture(const char* fn, hipStream_t s, const char* why) {
    QA_REQUIRE(!stream_capturing(s), "%s: refused under a stream capture - %s", fn, why);
    return QA_OK;
}

// ---------------------------------------------------------------- test taps (the qa_*_tap / qa_*_enable_taps entry points)

inline int taps_enable(Ctx* c, const char* fn, int on) {
    if (!c) {
        set_error("%s: null handle", fn);
        return QA_ERR_INVALID;
    }
    c->capture = on != 0;
    return QA_OK;
}

inline int64_t tap_read(const Ctx* c, const char* fn, const char* name, float* dst, int64_t cap, void* stream) {
    if (!c || !name) {
        set_error("%s: null argument", fn);
        return QA_ERR_INVALID;
    }
    auto it = c->taps.find(name);
    if (it == c->taps.end()) {
        set_error("%s: no intermediate named '%s' in the last call", fn, name);
        return QA_ERR_MISSING;
    }
    if (dst) {
        if (cap < it->second.numel) {
            set_error("%s: '%s' has %lld elements, capacity %lld", fn, name, (long long)it->second.numel, (long long)cap);
            return QA_ERR_INVALID;
        }
        QA_HIP(hipMemcpyAsync(dst, it->second.ptr, sizeof(float) * it->second.numel, hipMemcpyDeviceToDevice,
                              static_cast<hipStream_t>(stream)));
    }
    return it->second.numel;
}

// ---------------------------------------------------------------- model handles

// What every qa_* handle owns.  A handle frees its own further resources in its destructor, so a failed create and qa_*_destroy
// release everything the same way (derived members go before these).
struct Handle {
    int device = 0;
    WeightStore store;
    Workspace ws;
    Ctx ctx;
};

// plan a call on the handle's context and workspace, then run its real pass
template <typename G>
int run_planned(Handle& h, void* stream, G&& graph) {
    QA_TRY(plan(h.device, static_cast<hipStream_t>(stream), h.ctx, h.ws, graph));
    return graph();
}

// The real pass of a planned call whose graph may launch the persistent LSTM recurrence (lstm.hip): every launch_lstm of a model graph.  Such
// a call waits for its stream before returning and, should one of that kernel's grid barriers have timed out (it needs every workgroup
// resident at once: the device was shared with another such kernel), runs the graph again on the per-step kernels - the call that hit the
// failure returns valid results, and the device stops choosing the persistent kernel by itself.  A graph whose recurrences are all
// launch_lstm_carry (the stream steps) or that has none uses only per-step kernels and needs no ticket: run_planned.
template <typename F>
int run_graph_checked(Handle* h, F&& graph) {
    Ctx& c = h->ctx;
    void* ticket = nullptr;
    QA_TRY(lstm_call_begin(h->device, &ticket));
    {
        const int st = graph();
        if (st != QA_OK) {  // error path only: the aggregator side stream may still run out of the workspace
            (void)hipDeviceSynchronize();
            bool ignored = false;
            (void)lstm_call_end(ticket, c.stream, &ignored);
            return st;
        }
    }
    bool failed = false;
    QA_TRY(lstm_call_end(ticket, c.stream, &failed));  // host-synchronous only for a call that launched an in-launch recurrence
    if (!failed) return QA_OK;
    std::fprintf(stderr, "libquarkaudio_hip: the grid barrier of the persistent LSTM recurrence timed out on device %d (shared device?); "
                         "re-running the call on the per-step kernels\n", h->device);
    lstm_force_per_step(true);
    arm(c, h->ws);
    const int st = graph();
    lstm_force_per_step(false);
    return st;
}

// qa_*_destroy: wait for the handle's work on its device, then free it
template <typename H>
void destroy_handle(H* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    (void)hipDeviceSynchronize();
    delete h;
}

// One output phase of a ConvTranspose1d(k, stride s, padding pad) as a stride-1 convolution.  Weight w [C_in][C_out][k] (nullptr: the
// filter stays zero).  y[q s + phi] = sum_m x[q + c0 - m] W[:, :, j0 + m s] with j0 = (phi + pad) mod s, c0 = (phi + pad) div s: a
// stride-1 convolution with taps jj = 0 .. n-1 <-> m = n-1-jj, pad_left = n - 1 - c0 (n = number of taps of the phase), right padding
// c0.  `filter` receives the library layout [C_out][n][C_in]; phase phi of the output is written to rows q s + phi.
struct PolyphaseFilter {
    std::vector<float> filter;
    int ntaps = 0, pad_left = 0;
};
inline int polyphase_filter(const float* w, int cin, int cout, int k, int s, int pad, int phi, PolyphaseFilter* out) {
    const int j0 = (phi + pad) % s, c0 = (phi + pad) / s, n = (k - j0 + s - 1) / s;
    QA_REQUIRE(n >= 1 && n - 1 - c0 >= 0, "ConvTranspose1d phase %d of k=%d s=%d has no causal tap layout", phi, k, s);
    out->filter.assign((size_t)cout * n * cin, 0.f);
    if (w)
        for (int o = 0; o < cout; ++o)
            for (int jj = 0; jj < n; ++jj) {
                const int j = j0 + (n - 1 - jj) * s;
                for (int c = 0; c < cin; ++c) out->filter[((size_t)o * n + jj) * cin + c] = w[((size_t)c * cout + o) * k + j];
            }
    out->ntaps = n;
    out->pad_left = n - 1 - c0;
    return QA_OK;
}

}  // namespace qa
