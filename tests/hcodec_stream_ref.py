"""The causal H-Codec 1.0 acoustic encoder (SEANetEncoder, seanet.py:121-187) restated on the CPU as a STREAM, with the arithmetic in the
dtype of the input: every causal SConv1d keeps the last ctx = k_eff - stride frames of its own input between chunks, the Transformer block
is tests/transformer_stream_ref.py's streaming form (DESIGN.md sections 42, 43).  float64 is the truth of the chunking property, float32
the form that tests/test_hcodec_stream_cpu.py pins to oracle.hcodec_ref.seanet_encoder.

The first chunk pads its left edge as the offline graph pads the chunk alone (oracle.hcodec_ref._pad1d_reflect).  While the chunk is longer
than ctx at every layer that is the reflection of its own frames 1 .. ctx - the same frames the offline call on the whole utterance reflects.
A shorter first chunk falls under pad1d's short-input rule (conv.py:79-96), and the whole utterance then reflects frames that the chunk
does not have yet: the stream is another function, which is why the library refuses such a chunk (`first_min_frames`).

Also here: the cases that the CPU and GPU tests of the stream share (seeds, shapes, chunkings), so that the near-tie condition the CPU test
asserts is the condition of the very inputs the GPU test runs.
"""
import torch
import torch.nn.functional as F

from oracle import hcodec_ref as R
from oracle import synth
from tests import transformer_stream_ref as TR

# chunkings of 24 code frames (test_hcodec_stream_cpu.py: B = 2, fp64; test_hcodec_stream_gpu.py: B = 3 against the oracle)
FRAMES = 24
CHUNKINGS = {"whole": (24,), "2+1x22": (2,) + (1,) * 22, "2-1-5-16": (2, 1, 5, 16), "3-4-3-4-3-4-3": (3, 4, 3, 4, 3, 4, 3)}
# (weights seed, waveform seed, B, code frames): seeds for which no RVQ decision of the oracle is a near-tie (asserted by the CPU test), so a
# correct stream must give EQUAL codes
GPU_MINI_CASE = dict(seed=11, wav_seed=31, B=3, frames=FRAMES)
GPU_LONG_CASE = dict(seed=11, wav_seed=41, B=1, frames=302)
GPU_REAL_CASE = dict(seed=1234, wav_seed=51, B=2, frames=8, chunks=(2, 1, 1, 4))


def conv_table(spec):
    """(k, stride, input frames per code frame) of the convolutions with a temporal footprint, in graph order: conv0, per stage the
    residual k3 and the down conv, the out conv."""
    n = len(spec.ratios)
    rate = [2] * (n + 1)
    for i in range(n - 1, -1, -1):
        rate[i] = rate[i + 1] * spec.ratios[i]
    rows = [(7, 1, rate[0])]
    for i, r in enumerate(spec.ratios):
        rows += [(3, 1, rate[i]), (2 * r, r, rate[i])]
    return rows + [(4, 2, 2)]


def contexts(spec):
    return [k - s for k, s, _ in conv_table(spec)]


def first_min_frames(spec):
    """The fewest code frames n for which every such convolution sees MORE input frames than its context (else pad1d's short-input rule)."""
    n = 1
    while any(n * rate <= k - s for k, s, rate in conv_table(spec)):
        n += 1
    return n


class State:
    """What the encoder keeps between chunks: per convolution the tail of its (activated) input, per Transformer layer TR's LayerState."""

    def __init__(self, spec):
        self.ctx = {}
        self.tr = TR.new_state(spec.enc_layers)
        self.frames = 0


def _sconv(state, sd, p, x, stride=1):
    """One causal SConv1d (weight-normed) on the chunk x [B, C, L]: a valid convolution over carried context | chunk."""
    w, b = R._fold_weight_norm(sd, p + ".conv.conv"), sd[p + ".conv.conv.bias"]
    ctx = w.shape[-1] - stride
    if ctx == 0:
        return F.conv1d(x, w, b, stride=stride)
    head = state.ctx.get(p)
    if head is None:  # first chunk: what the offline graph pads this chunk with
        head = R._pad1d_reflect(x, ctx, 0)[..., :ctx]
    win = torch.cat((head, x), -1)
    state.ctx[p] = win[..., -ctx:]
    return F.conv1d(win, w, b, stride=stride)


def step(sd, wav, spec, state, block=None, taps=None):
    """The next chunk wav [B, 1, n * enc_hop] -> emb [B, dimension, n].  sd must already be in wav's dtype (TR.cast).  block: the
    Transformer on x [B, T, d] (default: TR's streaming chunk over state.tr)."""
    p = "encoder.model"
    nr = len(spec.ratios)
    x = _sconv(state, sd, f"{p}.0", wav)
    if taps is not None:
        taps["enc.conv0"] = x
    for i, r in enumerate(spec.ratios):
        rp = f"{p}.{1 + 3 * i}"
        h = _sconv(state, sd, rp + ".block.1", F.elu(x))
        h = _sconv(state, sd, rp + ".block.3", F.elu(h))
        x = _sconv(state, sd, rp + ".shortcut", x) + h
        x = _sconv(state, sd, f"{p}.{3 + 3 * i}", F.elu(x), stride=r)
        if taps is not None:
            taps[f"enc.stage{i}"] = x
    tp = f"{p}.{3 * nr + 2}"
    if block is None:
        tsd = {k: v for k, v in sd.items() if k.startswith(tp + ".")}
        x = TR.chunk(tsd, x.transpose(1, 2), spec.enc_layers, spec.enc_heads, True, state=state.tr, carry=True, prefix=tp).transpose(1, 2)
    else:
        x = block(x.transpose(1, 2)).transpose(1, 2)
    if taps is not None:
        taps["enc.transformer"] = x
    state.frames += wav.shape[-1] // spec.enc_hop
    return _sconv(state, sd, f"{p}.{3 * nr + 5}", F.elu(x), stride=2)


def stream(sd, wav, spec, chunks, dtype=None, block=None, taps=None):
    """wav [B, 1, sum(chunks) * enc_hop] through one streaming state, chunk by chunk (code frames); the outputs concatenated.  One chunk
    of the whole length is the offline causal forward."""
    dtype = dtype or wav.dtype
    sd, wav = TR.cast(sd, dtype), wav.to(dtype)
    state, out, t = State(spec), [], 0
    for n in chunks:
        out.append(step(sd, wav[..., t * spec.enc_hop:(t + n) * spec.enc_hop], spec, state, block, taps))
        t += n
    assert t * spec.enc_hop == wav.shape[-1]
    return torch.cat(out, -1)


def case_inputs(case, spec_kwargs):
    """(oracle spec, state_dict, wav [B, 1, frames * hop]) of one of the shared cases."""
    ospec = R.HCodecSpec(**spec_kwargs)
    sd = synth.hcodec10_state_dict(case["seed"], ospec)
    wav = synth.synth_wav(case["wav_seed"], case["B"], case["frames"] * ospec.enc_hop).unsqueeze(1)
    return ospec, sd, wav


def oracle_emb_and_codes(sd, wav, ospec):
    """The oracle's offline causal acoustic half: emb [B, D, N] (fp32) and acoustic codes [B, nq, N]."""
    emb = R.seanet_encoder(sd, wav, ospec)
    ac, _ = R.rvq_search(emb.transpose(1, 2), R.rvq_codebooks(sd, "quantizer", ospec.num_quantizers))
    return emb, ac.transpose(1, 2).contiguous()
