"""The codec Transformer (encoder_modules/transformer.py:396-489) restated on the CPU in three forms - offline, the reference's cache mode
and a streaming state - with the arithmetic in the dtype of the input: float64 is the truth of tests/test_transformer_stream_gpu.py, float32
its yardstick.  tests/test_transformer_stream_cpu.py pins the float32 offline form against oracle.hcodec_ref.transformer
and the reference's own module, the cache mode against the module driven with a DynamicCache, and the streaming form against the offline one.

One thing stays in float32 whatever the dtype: the RoPE angle.  The reference forces it (transformer.py:38-39, "Force float32"), so
position * inv_freq rounded to float32 IS the angle, and cos / sin of that angle are then taken in the working dtype.
"""
import importlib.util
import os

import torch
import torch.nn.functional as F

from oracle import ref_shim


def random_state_dict(seed, hidden, inter, layers, prefix=""):
    """Seeded weights that keep activations O(1): matrices N(0, 1 / fan_in), LSTM matrices and biases U(-1 / sqrt(d), 1 / sqrt(d)) like
    nn.LSTM's own init, norm weights around 1 (the reference's default init is a hundred times smaller: every output would be ~x)."""
    g = torch.Generator().manual_seed(seed)
    p = prefix + "." if prefix else ""
    sd = {}

    def mat(n, k, gain=1.0):
        return torch.randn(n, k, generator=g) * (gain / k ** 0.5)

    def uni(*shape):
        return (torch.rand(*shape, generator=g) * 2 - 1) / hidden ** 0.5

    for l in range(layers):
        lp = f"{p}layers.{l}"
        sd[lp + ".input_layernorm.weight"] = 1 + 0.1 * torch.randn(hidden, generator=g)
        sd[lp + ".post_attention_layernorm.weight"] = 1 + 0.1 * torch.randn(hidden, generator=g)
        sd[lp + ".self_attn.rnn.weight_ih_l0"] = uni(4 * hidden, hidden) * 2
        sd[lp + ".self_attn.rnn.weight_hh_l0"] = uni(4 * hidden, hidden) * 2
        sd[lp + ".self_attn.rnn.bias_ih_l0"] = uni(4 * hidden)
        sd[lp + ".self_attn.rnn.bias_hh_l0"] = uni(4 * hidden)
        for n in ("q_proj", "k_proj", "v_proj"):
            sd[f"{lp}.self_attn.{n}.weight"] = mat(hidden, hidden, 2.0)
            sd[f"{lp}.self_attn.{n}.bias"] = 0.1 * torch.randn(hidden, generator=g)
        sd[lp + ".self_attn.o_proj.weight"] = mat(hidden, hidden)
        sd[lp + ".mlp.w1.weight"] = mat(inter, hidden)
        sd[lp + ".mlp.w3.weight"] = mat(inter, hidden)
        sd[lp + ".mlp.w2.weight"] = mat(hidden, inter)
    return sd


def cast(sd, dtype):
    return {k: v.to(dtype) for k, v in sd.items()}


def rms_norm(x, w, eps=1e-6):
    return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * w


def lstm(x, w_ih, w_hh, b_ih, b_hh, state=None):
    """nn.LSTM(d, d, 1, batch_first=True) in x's dtype, gate order i, f, g, o; state = (h, c) [B, d] each or None (zeros).  Returns
    (h of every step [B, T, d], (h, c) behind the last step)."""
    B, T, d = x.shape
    h, c = state if state is not None else (x.new_zeros(B, d), x.new_zeros(B, d))
    xw = x @ w_ih.t() + (b_ih + b_hh)
    out = []
    for t in range(T):
        i, f, g, o = (xw[:, t] + h @ w_hh.t()).split(d, dim=1)
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
        h = torch.sigmoid(o) * torch.tanh(c)
        out.append(h)
    return torch.stack(out, 1), (h, c)


def rope_cos_sin(pos0, n, hd, dtype):
    inv_freq = 1.0 / (10000.0 ** (torch.arange(0, hd, 2, dtype=torch.int64).float() / hd))
    ang = torch.arange(pos0, pos0 + n).float()[:, None] * inv_freq[None, :]  # float32, like the reference
    emb = torch.cat((ang, ang), -1).to(dtype)
    return emb.cos(), emb.sin()


def _rotate_half(x):
    h = x.shape[-1] // 2
    return torch.cat((-x[..., h:], x[..., :h]), -1)


class LayerState:
    """What one layer keeps between chunks: the roped keys and the values so far [B, H, len, hd], and (streaming only) the LSTM's (h, c)."""

    def __init__(self):
        self.k = self.v = self.hc = None


def new_state(layers):
    return [LayerState() for _ in range(layers)]


def state_length(state):
    return 0 if state[0].k is None else state[0].k.shape[2]


def chunk(sd, x, layers, heads, causal, left_context=0, state=None, carry=False, prefix=""):
    """One call on x [B, n, d] at positions len .. len + n - 1 (len = frames in `state`; state None: 0 and nothing kept).  Keys = state |
    chunk.  causal: the query at p sees key j iff j <= p and (left_context == 0 or p - j < left_context); else every key.  carry: the LSTM
    continues from the state's (h, c) and leaves them there (streaming); else it starts from zero, as the reference's does on every call."""
    sd = cast(sd, x.dtype)
    p0 = prefix + "." if prefix else ""
    B, n, d = x.shape
    hd = d // heads
    pos0 = state_length(state) if state is not None else 0
    cos, sin = rope_cos_sin(pos0, n, hd, x.dtype)
    for l in range(layers):
        lp = f"{p0}layers.{l}"
        ap = lp + ".self_attn"
        st = state[l] if state is not None else LayerState()
        h = rms_norm(x, sd[lp + ".input_layernorm.weight"])
        h, hc = lstm(h, sd[ap + ".rnn.weight_ih_l0"], sd[ap + ".rnn.weight_hh_l0"], sd[ap + ".rnn.bias_ih_l0"], sd[ap + ".rnn.bias_hh_l0"],
                     st.hc if carry else None)
        if carry:
            st.hc = hc
        q, k, v = (F.linear(h, sd[f"{ap}.{m}.weight"], sd[f"{ap}.{m}.bias"]).view(B, n, heads, hd).transpose(1, 2)
                   for m in ("q_proj", "k_proj", "v_proj"))
        q = q * cos + _rotate_half(q) * sin
        k = k * cos + _rotate_half(k) * sin
        st.k = k if st.k is None else torch.cat((st.k, k), 2)
        st.v = v if st.v is None else torch.cat((st.v, v), 2)
        w = torch.matmul(q, st.k.transpose(2, 3)) * hd ** -0.5
        if causal:
            p = torch.arange(pos0, pos0 + n)[:, None]
            j = torch.arange(pos0 + n)[None, :]
            seen = j <= p
            if left_context > 0:
                seen = seen & (p - j < left_context)
            w = w.masked_fill(~seen, float("-inf"))
        o = torch.matmul(F.softmax(w, -1), st.v).transpose(1, 2).reshape(B, n, d)
        x = x + F.linear(o, sd[ap + ".o_proj.weight"])
        h = rms_norm(x, sd[lp + ".post_attention_layernorm.weight"])
        x = x + F.linear(F.silu(F.linear(h, sd[lp + ".mlp.w1.weight"])) * F.linear(h, sd[lp + ".mlp.w3.weight"]), sd[lp + ".mlp.w2.weight"])
    return x


def forward(sd, x, layers, heads, causal=False, left_context=0, prefix=""):
    """Transformer.forward(x): the offline form."""
    return chunk(sd, x, layers, heads, causal, left_context, prefix=prefix)


def forward_cached(sd, x, state, layers, heads, causal=False, left_context=0, prefix=""):
    """Transformer.forward(x, past_key_values, use_cache=True): LSTM from zero, keys = cache | chunk.  The reference's causal mask is (T, T)
    for the chunk alone, so with a non-empty cache it raises; so does this."""
    if causal and state_length(state) > 0:
        raise RuntimeError("causal Transformer: the (T, T) mask cannot be combined with cached keys (transformer.py:469-475)")
    return chunk(sd, x, layers, heads, causal, left_context, state=state, prefix=prefix)


def stream(sd, x, chunks, layers, heads, left_context=0, prefix="", state=None):
    """x [B, sum(chunks), d] through one streaming state, chunk by chunk; the outputs concatenated."""
    state = new_state(layers) if state is None else state
    out, t = [], 0
    for n in chunks:
        out.append(chunk(sd, x[:, t:t + n], layers, heads, True, left_context, state=state, carry=True, prefix=prefix))
        t += n
    assert t == x.shape[1]
    return torch.cat(out, 1)


def rel_err(y, y64):
    """e = max|y - y64| / max|y64|."""
    return float((y.double() - y64).abs().max() / y64.abs().max())


# ------------------------------------------------------------------------------------------------ the reference's own module and the golden
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "transformer_cache_small.npz")
GOLDEN_SHAPE = dict(hidden=128, inter=256, heads=2, layers=2, B=2, T=24)
GOLDEN_CHUNKS = (5, 7, 1, 11)


def golden_inputs(seed):
    s = GOLDEN_SHAPE
    sd = random_state_dict(seed, s["hidden"], s["inter"], s["layers"])
    x = torch.randn(s["B"], s["T"], s["hidden"], generator=torch.Generator().manual_seed(seed + 1))
    return sd, x


def load_reference_transformer(hidden, inter, heads, layers, causal=False, use_sliding_window=False, left_context=0):
    """The reference's own Transformer class, from its file alone (the `vq` package around it pulls in the whole codec)."""
    path = os.path.join(ref_shim.REFERENCE_ROOT, "QuarkAudio-HCodec", "HCodec-1.0", "vq", "encoder_modules", "transformer.py")
    spec = importlib.util.spec_from_file_location("_qa_ref_codec_transformer", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    m = mod.Transformer(hidden, inter, heads, layers, causal=causal, use_sliding_window=use_sliding_window, left_context=left_context)
    return m.eval(), mod.DynamicCache


def reference_golden(seed):
    """The arrays of tests/golden/transformer_cache_small.npz, from the reference module itself."""
    s = GOLDEN_SHAPE
    sd, x = golden_inputs(seed)
    out = {"seed": torch.tensor(seed), "x": x}
    with torch.no_grad():
        for name, causal in (("offline_noncausal", False), ("offline_causal", True)):
            m, _ = load_reference_transformer(s["hidden"], s["inter"], s["heads"], s["layers"], causal=causal)
            m.load_state_dict(sd)
            out[name] = m(x)
        m, cache_cls = load_reference_transformer(s["hidden"], s["inter"], s["heads"], s["layers"])
        m.load_state_dict(sd)
        cache, ys, t = cache_cls(), [], 0
        for n in GOLDEN_CHUNKS:
            y, cache = m(x[:, t:t + n], past_key_values=cache, use_cache=True)
            ys.append(y)
            t += n
        out["cached_noncausal"] = torch.cat(ys, 1)
    return {k: v.numpy() for k, v in out.items()}
