// stream_conv.hip - the carried left context of a causal SConv1d in a stream.
//
// A causal SConv1d pads (ctx, 0) with ctx = k_eff - stride (encoder_modules/conv.py:203-206).  In a stream every such convolution runs as a
// VALID convolution over a window [B, ctx + n, C] = the last ctx input rows of the previous step | the n rows of this step, and keeps the
// window's last ctx rows for the next one.  On the first step the head is the reflection of the chunk itself (position -1 - j reads frame
// 1 + j), what pad1d gives an input longer than its padding.  One launch per stateful convolution builds the window and the next state.
//
// Pure copies, HBM-bound and at the launch floor for the shapes of a stream step (a few hundred rows): one thread per float4 of the
// window (one float where C % 4 != 0: the waveform, C = 1), consecutive threads on consecutive addresses of every buffer they touch.
#include "kernels.h"

namespace qa {

// I: the index type of an element of the window (int unless B (ctx + n) C can pass 2^31); V: float4 or float.
// Element (b, t, c) of the window:
//     t <  ctx : first ? chunk[b, ctx - t, c] : state_in[b, t, c]
//     t >= ctx : chunk[b, t - ctx, c]
// and the rows t >= n are the next state, row t - n.  For n < ctx those rows start inside the head, i.e. the next state takes rows of the
// current one: state_in and state_out are therefore DIFFERENT buffers (the host alternates two per convolution), no thread reads a row
// that a thread of the same launch writes, and the result does not depend on the order in which the threads run.
//
// ROWS (a step with per-row lengths): item b holds n_b = min(n_rows[b] * mul, n) live chunk rows and is a first step
// iff first_rows[b] != 0 (and n_b > ctx, what the reflection reads).  Its body is the chunk for t - ctx < n_b and 0.0f behind it - the
// caller's rows behind a length are never read, so whatever they hold stays out of the ladder - and its next state is the window rows
// n_b .. n_b + ctx - 1, all of them head or live chunk rows.  n_b = 0: the state moves to the other buffer unchanged.  `first` is not
// read.  Without ROWS the kernel is the rectangular one, instruction for instruction.
template <typename I, typename V, bool ROWS>
__global__ __launch_bounds__(256) void stream_window_kernel(const V* __restrict__ state_in, const V* __restrict__ chunk, V* __restrict__ win,
                                                            V* __restrict__ state_out, I total, int ctx, int n, int Cv, int first,
                                                            const int* __restrict__ n_rows, int mul, const int* __restrict__ first_rows) {
    const I gid = (I)blockIdx.x * (I)blockDim.x + (I)threadIdx.x;
    if (gid >= total) return;
    const int c = (int)(gid % Cv);
    const I row = gid / Cv;
    const int W = ctx + n;
    const int t = (int)(row % W);
    const I b = row / W;
    V v;
    if (ROWS) {
        const int nb = min(max(n_rows[b], 0) * mul, n);
        const bool fb = first_rows[b] != 0 && nb > ctx;
        if (t >= ctx) v = (t - ctx < nb) ? chunk[(b * n + (t - ctx)) * Cv + c] : V{};
        else if (fb) v = chunk[(b * n + (ctx - t)) * Cv + c];
        else v = state_in[(b * ctx + t) * Cv + c];
        win[gid] = v;
        if (t >= nb && t < nb + ctx) state_out[(b * ctx + (t - nb)) * Cv + c] = v;
        return;
    }
    if (t >= ctx) v = chunk[(b * n + (t - ctx)) * Cv + c];
    else if (first) v = chunk[(b * n + (ctx - t)) * Cv + c];
    else v = state_in[(b * ctx + t) * Cv + c];
    win[gid] = v;
    if (t >= n) state_out[(b * ctx + (t - n)) * Cv + c] = v;
}

template <typename I, typename V>
static void stream_window_launch(const float* state_in, const float* chunk, float* win, float* state_out, long long total, int ctx, int n,
                                 int Cv, int first, hipStream_t s, const int* n_rows, int mul, const int* first_rows) {
    const dim3 grid((unsigned)ceil_div(total, 256));
    if (n_rows)
        hipLaunchKernelGGL((stream_window_kernel<I, V, true>), grid, dim3(256), 0, s, reinterpret_cast<const V*>(state_in),
                           reinterpret_cast<const V*>(chunk), reinterpret_cast<V*>(win), reinterpret_cast<V*>(state_out), (I)total, ctx, n, Cv,
                           first, n_rows, mul, first_rows);
    else
        hipLaunchKernelGGL((stream_window_kernel<I, V, false>), grid, dim3(256), 0, s, reinterpret_cast<const V*>(state_in),
                           reinterpret_cast<const V*>(chunk), reinterpret_cast<V*>(win), reinterpret_cast<V*>(state_out), (I)total, ctx, n, Cv,
                           first, n_rows, mul, first_rows);
}

int launch_stream_window(const float* state_in, const float* chunk, float* win, float* state_out, int B, int ctx, int n, int C, int first,
                         hipStream_t s, ClipLens rows, const int* first_rows) {
    QA_REQUIRE(chunk && win && state_out && B > 0 && ctx > 0 && n > 0 && C > 0, "stream_window: B=%d ctx=%d n=%d C=%d", B, ctx, n, C);
    const int* n_rows = rows.n;
    const int mul = rows.mul;
    QA_REQUIRE((n_rows == nullptr) == (first_rows == nullptr) && (!n_rows || mul >= 1),
               "stream_window: the rows' counts and first flags come together, with a multiplier >= 1");
    if (n_rows) {
        first = 0;
        QA_REQUIRE(state_in && state_in != state_out, "stream_window: a step with per-row lengths needs the state of the previous one in a "
                   "buffer other than state_out (an idle row's state moves from one to the other)");
    }
    QA_REQUIRE(first || state_in, "stream_window: a later step needs the state of the previous one");
    QA_REQUIRE(first || state_in != state_out, "stream_window: state_in and state_out must be different buffers (for n < ctx the next state "
               "takes rows of the current one)");
    // the reflection of a first chunk reads its frames 1 .. ctx; a shorter one falls under pad1d's short-input rule, another function
    QA_REQUIRE(!first || n > ctx, "stream_window: a first chunk of %d rows cannot fill a reflected context of %d", n, ctx);
    const long long elems = (long long)B * (ctx + n) * C;
    QA_REQUIRE(elems / 256 < (1LL << 31), "stream_window: window of %lld elements is too large", elems);
    auto aligned = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    const bool vec = C % 4 == 0 && aligned(state_in) && aligned(chunk) && aligned(win) && aligned(state_out);
    const int Cv = vec ? C / 4 : C;
    const long long total = vec ? elems / 4 : elems;
    // 64-bit row arithmetic only where an element index - the last block's padding threads included - can pass 2^31
    const bool wide = elems + 256 >= (1LL << 31);
    if (vec) {
        if (wide) stream_window_launch<long long, float4>(state_in, chunk, win, state_out, total, ctx, n, Cv, first, s, n_rows, mul, first_rows);
        else stream_window_launch<int, float4>(state_in, chunk, win, state_out, total, ctx, n, Cv, first, s, n_rows, mul, first_rows);
    } else {
        if (wide) stream_window_launch<long long, float>(state_in, chunk, win, state_out, total, ctx, n, Cv, first, s, n_rows, mul, first_rows);
        else stream_window_launch<int, float>(state_in, chunk, win, state_out, total, ctx, n, Cv, first, s, n_rows, mul, first_rows);
    }
    QA_LAUNCH_CHECK();
    return QA_OK;
}

}  // namespace qa

extern "C" int qa_debug_stream_window(const float* state_in, const float* chunk, float* win, float* state_out, int B, int ctx, int n, int C,
                                      int first, void* stream) {
    return qa::launch_stream_window(state_in, chunk, win, state_out, B, ctx, n, C, first, static_cast<hipStream_t>(stream));
}

extern "C" int qa_debug_stream_window_rows(const float* state_in, const float* chunk, float* win, float* state_out, int B, int ctx, int n,
                                           int C, const int* n_rows_dev, const int* first_dev, void* stream) {
    QA_REQUIRE(n_rows_dev && first_dev, "qa_debug_stream_window_rows: null row arrays (qa_debug_stream_window is the rectangular call)");
    return qa::launch_stream_window(state_in, chunk, win, state_out, B, ctx, n, C, 0, static_cast<hipStream_t>(stream),
                                    qa::ClipLens{n_rows_dev, 1}, first_dev);
}
