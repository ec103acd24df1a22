"""QA_AGG_LAST_ROWS: the last layer of each H-Codec 1.5 aggregator stack on the query rows only (csrc/hcodec.cpp mimi_readout_layer)
against the full last layer followed by agg_gather (knob 0).  Every op past the key / value projection is row-wise, conv_gemm's bits
do not depend on M or the tile and attention's not on the number of queries, so the two must agree BIT FOR BIT on the aggregated
embeddings (taps enc.emb_agg, enc.sem_agg) and on both code tensors.

The model is tests/util.MINI as an H-Codec 1.5 (weights from unified_audio_amd.synth): 2 heads, ff 128, 2 aggregator layers, B = 3.
Its width is 128, the smallest the library builds: the aggregators run at the SEANet encoder's width, whose LSTM needs a multiple
of 128.  Groups come from SSL features that are piecewise constant with a different number of pieces per clip; every case asserts
the group pattern it is about, read from the codes' injected lengths."""
import dataclasses

import numpy as np
import pytest
import torch

from tests.util import MINI
from unified_audio_amd import synth

pytestmark = pytest.mark.gpu

B = 3


def _codec(device, agg_layers=2):
    import unified_audio_amd as qa

    spec = dataclasses.replace(qa.HCodecSpec(**MINI), adaptive=True, agg_layers=agg_layers, bt_layers=1, agg_heads=2, bt_heads=2, agg_ff=128,
                               bt_ff=128, max_tokens_per_group=32)  # 32 > N25: a clip can be one group
    codec = qa.Codec(None, None, None, spec=spec, device=device).load_state_dict(synth.hcodec10_state_dict(7, spec))
    codec.enable_taps()
    return codec, spec


def _pieces(seed, counts, frames, dim):
    """[B, dim, frames]: clip b is counts[b] constant pieces of (almost) equal length, each an independent normal vector"""
    rng = np.random.default_rng(seed)
    out = np.zeros((len(counts), dim, frames), np.float32)
    for b, k in enumerate(counts):
        edges = np.linspace(0, frames, k + 1).round().astype(int)
        for i in range(k):
            out[b, :, edges[i]:edges[i + 1]] = rng.standard_normal((dim, 1))
    return torch.from_numpy(out)


def _both(codec, spec, knob, n25, feat, threshold):
    """encode with the knob at 1 and at 0: nseg [B] and G of the call; asserts the bit identity"""
    wav = synth.synth_wav(8, B, n25 * spec.enc_hop).to(codec.device).unsqueeze(1)
    feat = feat.to(codec.device)
    runs = []
    for v in (1, 0):
        knob("QA_AGG_LAST_ROWS", v)
        codes = codec.encode(wav, feat, threshold=threshold)
        torch.cuda.synchronize()
        runs.append((codes["acoustic_codes"].clone(), codes["semantic_codes"].clone(), codec.tap("enc.emb_agg").clone(),
                     codec.tap("enc.sem_agg").clone()))
    for name, u, v in zip(("acoustic_codes", "semantic_codes", "enc.emb_agg", "enc.sem_agg"), *runs):
        assert u.shape == v.shape and torch.equal(u, v), f"{name}: QA_AGG_LAST_ROWS = 1 differs from 0 in {int((u != v).sum())} of {u.numel()} values"
    sc = runs[0][1]
    G = sc.shape[-1]
    assert runs[0][2].numel() == B * G * spec.code_dim and bool(torch.isfinite(runs[0][2]).all())
    length = torch.div(sc[:, 0], spec.codebook_size, rounding_mode="floor") + 1  # injected group lengths; 0 = padded group
    nseg = (length > 0).sum(dim=1).cpu().tolist()
    assert int(length.clamp(min=0).sum()) == B * n25 and max(nseg) == G
    return nseg, G


@pytest.mark.parametrize("n25, agg_layers, want", [(16, 2, [2, 5, 1]), (20, 2, [2, 4, 2]), (16, 1, [2, 5, 1])],
                         ids=["ragged-3x5", "ragged-3x4", "depth-1"])
def test_ragged_groups(qa_lib, gpu_device, knob, n25, agg_layers, want):
    """Ragged group counts, so padded groups exist; at 16 frames one clip is a single group and B G = 15 is no multiple of 4 (tile edge
    and scalar epilogue tail), at 20 frames B G = 12 is; in a stack of depth 1 the last layer is also the first."""
    codec, spec = _codec(gpu_device, agg_layers)
    nseg, G = _both(codec, spec, knob, n25, _pieces(9, (1, n25 // 4, 2), 2 * n25, spec.sem_in), 0.70)
    print("nseg", nseg, "G", G)
    assert nseg == want and min(nseg) < G and (n25 != 16 or (min(nseg) == 1 and (B * G) % 4 != 0)), nseg


def test_every_frame_its_own_group(qa_lib, gpu_device, knob):
    codec, spec = _codec(gpu_device)
    nseg, G = _both(codec, spec, knob, 12, synth.synth_feat(10, B, 24, spec.sem_in), 1.0)
    assert nseg == [12] * B and G == 12, nseg


def test_one_group_per_clip(qa_lib, gpu_device, knob):
    codec, spec = _codec(gpu_device)
    nseg, G = _both(codec, spec, knob, 16, _pieces(9, (1, 1, 1), 32, spec.sem_in), 0.5)
    assert nseg == [1] * B and G == 1, nseg
