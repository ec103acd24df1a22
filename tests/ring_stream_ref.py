"""The ring K / V cache under a sliding window restated on the CPU, and the cases its CPU and GPU tests share.

Three things live here:
  - the geometry of unified_audio_amd/csrc/ring_geometry.h in Python (capacity, row of a position, p(s), visibility);
  - ring_stream(): tests/transformer_stream_ref.py's streaming chunk with its growing key list replaced by a literal ring - rows that are
    never cleared (NaN to begin with), appended at p mod cap, read back through p(s) and the visibility rule in PHYSICAL row order, loads
    of unwritten rows redirected to the row of the last position - the way the kernels of stream_attn.hip do it;
  - the windowed H-Codec case: the SEANet encoder whose Transformer was built with use_sliding_window=True, left_context=W.  This is not
    the shipped full-causal model (vq/codec.py never sets the window); it is the definition a windowed stream is held to.
"""
import torch
import torch.nn.functional as F

from oracle import hcodec_ref as R
from tests import hcodec_stream_ref as S
from tests import transformer_stream_ref as TR
from tests.util import MINI

ROW_ALIGN = 32
MAX_POSITIONS = 1 << 24
TABLE_POSITIONS = 8192  # the static RoPE table of the library


# ------------------------------------------------------------------------------------------------ geometry
def capacity(left_context, max_chunk):
    """Rows of the ring: left_context - 1 + max_chunk is what a chunk's own appends need; one more because attention_kernel's ring mode
    counts the row under the write cursor as unwritten; whole 32-key tiles."""
    need = left_context + max_chunk
    return (need + ROW_ALIGN - 1) // ROW_ALIGN * ROW_ALIGN


def min_rows(context, n):
    return context - 1 + n


def row_of(p, cap):
    return p % cap


def pos_of_row(s, e, cap):
    """p(s) with e = pos0 + nq the item's own end; negative: never written for this sequence."""
    return e - 1 - ((e - 1 - s) % cap)


def visible(p, P, context):
    return 0 <= p <= P and P - p < context


# ------------------------------------------------------------------------------------------------ the block over a literal ring
class RingState:
    def __init__(self, layers):
        self.k = [None] * layers
        self.v = [None] * layers
        self.hc = [None] * layers
        self.pos = 0


def ring_chunk(sd, x, layers, heads, left_context, cap, state, prefix=""):
    """One streaming step of x [B, n, d] at positions state.pos .. + n - 1 over rings of `cap` rows [B, H, cap, hd]."""
    sd = TR.cast(sd, x.dtype)
    p0 = prefix + "." if prefix else ""
    B, n, d = x.shape
    hd = d // heads
    pos0, e = state.pos, state.pos + n
    assert cap >= min_rows(left_context, n), "the chunk's own appends would overwrite a key its first query sees"
    cos, sin = TR.rope_cos_sin(pos0, n, hd, x.dtype)
    rows = torch.tensor([row_of(p, cap) for p in range(pos0, e)])
    pos = torch.tensor([pos_of_row(s, e, cap) for s in range(cap)])
    P = torch.arange(pos0, e)[:, None]
    seen = (pos[None, :] >= 0) & (pos[None, :] <= P) & (P - pos[None, :] < left_context)  # [n, cap]
    load = torch.where(pos >= 0, torch.arange(cap), torch.full((cap,), row_of(e - 1, cap)))  # unwritten rows: the last position's row
    for l in range(layers):
        lp = f"{p0}layers.{l}"
        ap = lp + ".self_attn"
        if state.k[l] is None:
            state.k[l] = x.new_full((B, heads, cap, hd), float("nan"))
            state.v[l] = x.new_full((B, heads, cap, hd), float("nan"))
        h = TR.rms_norm(x, sd[lp + ".input_layernorm.weight"])
        h, state.hc[l] = TR.lstm(h, sd[ap + ".rnn.weight_ih_l0"], sd[ap + ".rnn.weight_hh_l0"], sd[ap + ".rnn.bias_ih_l0"],
                                 sd[ap + ".rnn.bias_hh_l0"], state.hc[l])
        q, k, v = (F.linear(h, sd[f"{ap}.{m}.weight"], sd[f"{ap}.{m}.bias"]).view(B, n, heads, hd).transpose(1, 2)
                   for m in ("q_proj", "k_proj", "v_proj"))
        q = q * cos + TR._rotate_half(q) * sin
        k = k * cos + TR._rotate_half(k) * sin
        state.k[l][:, :, rows] = k  # appended first ...
        state.v[l][:, :, rows] = v
        kk, vv = state.k[l][:, :, load], state.v[l][:, :, load]  # ... then every query attends over the physical rows
        w = (torch.matmul(q, kk.transpose(2, 3)) * hd ** -0.5).masked_fill(~seen, float("-inf"))
        o = torch.matmul(F.softmax(w, -1), vv).transpose(1, 2).reshape(B, n, d)
        x = x + F.linear(o, sd[ap + ".o_proj.weight"])
        h = TR.rms_norm(x, sd[lp + ".post_attention_layernorm.weight"])
        x = x + F.linear(F.silu(F.linear(h, sd[lp + ".mlp.w1.weight"])) * F.linear(h, sd[lp + ".mlp.w3.weight"]), sd[lp + ".mlp.w2.weight"])
    state.pos = e
    return x


def ring_stream(sd, x, chunks, layers, heads, left_context, cap, prefix=""):
    state, out, t = RingState(layers), [], 0
    for n in chunks:
        out.append(ring_chunk(sd, x[:, t:t + n], layers, heads, left_context, cap, state, prefix))
        t += n
    assert t == x.shape[1]
    return torch.cat(out, 1)


# ------------------------------------------------------------------------------------------------ one step of attention, for the kernel tests
def attn_step_ref(qkv, kc, vc, heads, cap, context, pos0, nq, ring, dtype=torch.float64):
    """qa_debug_stream_attn for ONE item in `dtype` (float64: the truth, float32: the yardstick): qkv [n, 3 d] (its first nq rows live),
    caches kc / vc [cap, d] (NaN where never written).  Returns (out [n, d] with zeros behind nq, the caches after the append).  The RoPE
    angle is fp32, as everywhere."""
    n, d3 = qkv.shape
    d = d3 // 3
    hd = d // heads
    qkv, kc, vc = qkv.to(dtype), kc.to(dtype).clone(), vc.to(dtype).clone()
    out = torch.zeros(n, d, dtype=dtype)
    if nq == 0:
        return out, kc, vc
    e = pos0 + nq
    cos, sin = TR.rope_cos_sin(pos0, nq, hd, dtype)
    q, k, v = (qkv[:nq, i * d:(i + 1) * d].view(nq, heads, hd).transpose(0, 1) for i in range(3))
    q = q * cos + TR._rotate_half(q) * sin
    k = k * cos + TR._rotate_half(k) * sin
    rows = torch.tensor([row_of(p, cap) if ring else p for p in range(pos0, e)])
    kc[rows] = k.transpose(0, 1).reshape(nq, d)
    vc[rows] = v.transpose(0, 1).reshape(nq, d)
    pos = torch.tensor([pos_of_row(s, e, cap) for s in range(cap)]) if ring else torch.where(torch.arange(cap) < e, torch.arange(cap), -1)
    P = torch.arange(pos0, e)[:, None]
    seen = (pos[None, :] >= 0) & (pos[None, :] <= P)
    if context > 0:
        seen = seen & (P - pos[None, :] < context)
    keep = pos >= 0
    kk = kc[keep].view(-1, heads, hd).transpose(0, 1)
    vv = vc[keep].view(-1, heads, hd).transpose(0, 1)
    w = (torch.matmul(q, kk.transpose(1, 2)) * hd ** -0.5).masked_fill(~seen[:, keep], float("-inf"))
    out[:nq] = torch.matmul(F.softmax(w, -1), vv).transpose(0, 1).reshape(nq, d)
    return out, kc, vc


# ------------------------------------------------------------------------------------------------ the windowed H-Codec case
CAUSAL_MINI = dict(MINI, causal=True)
# weights seed 11, waveform seed 61, B = 3, 72 code frames: no RVQ decision of the windowed oracle is a near-tie for W = 12 and W = 7
# (asserted by tests/test_stream_ring_cpu.py; waveform seeds 31 and 62 fail that audit), so a correct windowed stream gives EQUAL codes
CODEC_CASE = dict(seed=11, wav_seed=61, B=3, frames=72)
CODEC_WINDOWS = (12, 7)  # Transformer frames, two per code frame
CODEC_MAX_CHUNK = 5      # code frames
CODEC_CHUNKINGS = {"2-1-5": (2, 1, 5) * 9, "2+1x70": (2,) + (1,) * 70, "2+5x14": (2,) + (5,) * 14}


def codec_inputs():
    return S.case_inputs(CODEC_CASE, CAUSAL_MINI)


def transformer_prefix(ospec):
    return f"encoder.model.{3 * len(ospec.ratios) + 2}"


def windowed_oracle(sd, wav, ospec, W):
    """The windowed offline form in fp32, the oracle's own Transformer in the middle: emb [B, D, N] and its acoustic codes [B, nq, N]."""
    tp = transformer_prefix(ospec)
    N = wav.shape[-1] // ospec.enc_hop
    emb = S.stream(sd, wav, ospec, (N,), block=lambda x: R.transformer(sd, tp, x, ospec.enc_layers, ospec.enc_heads, None, True, W))
    ac, _ = R.rvq_search(emb.transpose(1, 2), R.rvq_codebooks(sd, "quantizer", ospec.num_quantizers))
    return emb, ac.transpose(1, 2).contiguous()


def windowed_stream(sd, wav, ospec, W, chunks, dtype):
    """The windowed STREAM restatement: the SEANet stream of hcodec_stream_ref with TR's streaming chunk under left_context = W."""
    tp = transformer_prefix(ospec)
    sd_t = TR.cast({k: v for k, v in sd.items() if k.startswith(tp + ".")}, dtype)
    state = TR.new_state(ospec.enc_layers)
    block = lambda x: TR.chunk(sd_t, x, ospec.enc_layers, ospec.enc_heads, True, W, state=state, carry=True, prefix=tp)  # noqa: E731
    return S.stream(sd, wav, ospec, chunks, dtype=dtype, block=block)


def windowed_offline(sd, wav, ospec, W, dtype):
    """The windowed offline form in `dtype` with TR.forward in the middle (the oracle's LSTM is fp32 only)."""
    tp = transformer_prefix(ospec)
    sd_t = TR.cast({k: v for k, v in sd.items() if k.startswith(tp + ".")}, dtype)
    N = wav.shape[-1] // ospec.enc_hop
    return S.stream(sd, wav, ospec, (N,), dtype=dtype, block=lambda x: TR.forward(sd_t, x, ospec.enc_layers, ospec.enc_heads, True, W, prefix=tp))
