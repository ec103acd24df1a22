"""Codec.forward on the HIP path (1.0, 1.5, 2.0): recon is decode(encode()) bit for bit, pred_feat (the semantic decoder) agrees with
the fp64 restatement applied to the path's own codes, and both match the reference's own forward (tests/golden/hcodec_forward_*)."""
import os

import numpy as np
import pytest
import torch

from oracle import hcodec_ref as R
from oracle import synth
from tests import hcodec_forward_ref as F
from tests.util import MINI, audit_codes_bnq, rel_err

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = {"10": ("hcodec_forward_10_b2", "1.0", 9501, 2, 640 * 6),
         "15": ("hcodec_forward_15_b2", "1.5", 9601, 2, 640 * 6),
         "20": ("hcodec_forward_20_b2", "2.0", 9701, 2, 3840 * 4)}


def _gen():
    import importlib.util

    path = os.path.join(os.path.dirname(GOLDEN), "..", "tools", "gen_golden_hcodec_forward.py")
    spec = importlib.util.spec_from_file_location("gen_golden_hcodec_forward", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _product_spec(ospec):
    import unified_audio_amd as qa

    if hasattr(ospec, "enc_transformer_layers"):  # oracle H-Codec 2.0 spec
        return qa.HCodecSpec(version=20, enc_dim=ospec.enc_dim, enc_inter=ospec.enc_inter, enc_convnext_layers=ospec.enc_convnext_layers,
                             enc_layers=ospec.enc_transformer_layers, frame_stride=ospec.stride, tr_inter_cap=ospec.tr_inter_cap,
                             dimension=ospec.dimension, code_dim=ospec.dimension, sem_in=ospec.sem_in, sem_ch=ospec.sem_ch,
                             sem_strides=ospec.sem_strides, codebook_size=ospec.codebook_size, num_quantizers=ospec.num_quantizers,
                             dec_dim=ospec.dec_dim, dec_inter=ospec.dec_inter, dec_heads=ospec.dec_dim // 64,
                             dec_layers=ospec.dec_transformer_layers, convnext_layers=ospec.dec_convnext_layers, n_fft=ospec.n_fft,
                             hop=ospec.hop, gn_groups=ospec.gn_groups, causal=ospec.causal)
    return qa.HCodecSpec(**{f: getattr(ospec, f) for f in ospec.__dataclass_fields__})


def _codec(sd, ospec, device):
    import unified_audio_amd as qa

    return qa.Codec(None, None, None, spec=_product_spec(ospec), device=device).load_state_dict(sd)


def _max_rel(a, ref):
    a, ref = a.double().cpu(), ref.double().cpu()
    return float((a - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


def _pred_bound(sd, sc, ospec, sds, adaptive):
    """fp64 restatement on the given semantic codes, and the fp32 restatement's own distance from it"""
    K = ospec.codebook_size if adaptive else 0
    p64 = F.pred_feat(sd, sc.cpu(), ospec.num_quantizers, sds, torch.float64, codebook_size=K)
    p32 = F.pred_feat(sd, sc.cpu(), ospec.num_quantizers, sds, torch.float32, codebook_size=K)
    return p64, 4 * max(_max_rel(p32, p64), 1e-6)


def _encode_decode(codec, x, feat):
    enc = codec.encode(x, feat)
    if codec.spec.adaptive:
        return enc["acoustic_codes"], enc["semantic_codes"], codec.decode(enc["acoustic_codes"], enc["semantic_codes"])
    return enc[0], enc[1], codec.decode(*enc)


@pytest.mark.parametrize("version", ["10", "15", "20"])
def test_forward_matches_encode_decode_fp64_and_reference_golden(qa_lib, gpu_device, version):
    gen = _gen()
    name, v, seed, batch, samples = CASES[version]
    ospec = gen.spec_for(v)
    sds = gen.sd_spec_for(ospec)
    sd, wav, feat = gen.inputs(v, seed, batch, samples, ospec)
    codec = _codec(sd, ospec, gpu_device)
    assert codec.has_semantic_decoder
    x = (wav if version == "20" else wav.unsqueeze(1)).to(gpu_device)
    f = feat.to(gpu_device)
    out = codec(x, f)
    ac, sc, wav_ed = _encode_decode(codec, x, f)
    torch.cuda.synchronize()
    adaptive = version == "15"
    recon, pred, loss = (out["recon"], out["pred_feat"], out["commit_loss"]) if adaptive else out
    # recon: the same kernels on the same device-resident codes
    assert recon.dtype == torch.float32 and recon.device == x.device and torch.equal(recon, wav_ed)
    assert loss.dim() == 0 and loss.device == x.device and float(loss) == 0.0
    if adaptive:
        K = ospec.codebook_size
        assert torch.equal(out["token_lengths"], torch.div(sc[:, 0], K, rounding_mode="floor") + 1)
        assert out["token_lengths"].dtype == torch.int64 and int(out["token_lengths"].sum(1).min()) == samples // 640
    # pred_feat against the fp64 restatement on the HIP path's OWN semantic codes (near-tie code flips cannot make this flaky)
    p64, bound = _pred_bound(sd, sc, ospec, sds, adaptive)
    assert pred.shape == p64.shape
    err = _max_rel(pred, p64)
    print(f"{name}: pred_feat max-rel error {err:.2e} (bound {bound:.2e})")
    assert err <= bound, (err, bound)
    # the reference's own forward (golden)
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    g_ac, g_sc = torch.from_numpy(g["acoustic_codes"].astype(np.int64)), torch.from_numpy(g["semantic_codes"].astype(np.int64))
    g_recon, g_pred = torch.from_numpy(g["recon"]), torch.from_numpy(g["pred_feat"])
    assert ac.shape == g_ac.shape and recon.shape == g_recon.shape and pred.shape == g_pred.shape
    taps = {}
    with torch.no_grad():
        if adaptive:
            from oracle import hcodec15_ref as R15

            R15.encode(sd, wav.unsqueeze(1), feat, ospec, taps)
            assert torch.equal(torch.from_numpy(g["token_lengths"].astype(np.int64)), out["token_lengths"].cpu())
            e_a, e_s, K = taps["enc.emb_agg"], taps["enc.sem_agg"], ospec.codebook_size
            audit_codes_bnq(e_a, R.rvq_codebooks(sd, "quantizer", ospec.num_quantizers), ac.cpu() % K, g_ac % K)
            audit_codes_bnq(e_s, R.rvq_codebooks(sd, "semantic_quantizer", ospec.num_quantizers), sc.cpu() % K, g_sc % K)
        else:
            if version == "20":
                from oracle import hcodec20_ref as R20

                R20.encode(sd, wav, feat, ospec, taps)
            else:
                R.encode(sd, wav.unsqueeze(1), feat, ospec, taps)
            audit_codes_bnq(taps["enc.emb"], R.rvq_codebooks(sd, "quantizer", ospec.num_quantizers), ac, g_ac)
            audit_codes_bnq(taps["enc.sem"], R.rvq_codebooks(sd, "semantic_quantizer", ospec.num_quantizers), sc, g_sc)
    if torch.equal(ac.cpu(), g_ac) and torch.equal(sc.cpu(), g_sc):
        assert rel_err(recon, g_recon) < 1e-4
        g64, _ = _pred_bound(sd, g_sc, ospec, sds, adaptive)
        assert _max_rel(pred, g_pred) <= bound + _max_rel(g_pred, g64)  # both within their bound of the same fp64 values
    else:  # a near-tie flip: the decoder from the reference's codes
        assert rel_err(codec.decode(g_ac.to(gpu_device), g_sc.to(gpu_device)), g_recon) < 1e-4


def _mini(seed, device, **kw):
    from unified_audio_amd.hcodec import SemanticDecoderSpec
    from unified_audio_amd.synth import hcodec_semantic_decoder_state_dict

    ospec = R.HCodecSpec(**{**MINI, **kw})
    sds = SemanticDecoderSpec.from_codec_spec(ospec)
    sd = synth.hcodec10_state_dict(seed, ospec)
    sd.update(hcodec_semantic_decoder_state_dict(seed + 100, sds))
    return ospec, sds, sd, _codec(sd, ospec, device)


@pytest.mark.parametrize("causal,frames", [(False, 1), (True, 1), (True, 7)])
def test_forward_causal_and_one_frame(qa_lib, gpu_device, causal, frames):
    """N25 = 1 is the smallest ConvTranspose1d input (one frame -> two); the causal codec spec (the semantic decoder has no flag)."""
    ospec, sds, sd, codec = _mini(9801, gpu_device, causal=causal)
    T = ospec.enc_hop * frames
    wav = synth.synth_wav(9802, 3, T)
    feat = synth.synth_feat(9803, 3, T // (ospec.enc_hop // 2), ospec.sem_in)
    x, f = wav.unsqueeze(1).to(gpu_device), feat.to(gpu_device)
    recon, pred, loss = codec(x, f)
    ac, sc, wav_ed = _encode_decode(codec, x, f)
    torch.cuda.synchronize()
    assert torch.equal(recon, wav_ed) and recon.shape == (3, T)
    assert pred.shape == (3, ospec.sem_in, 2 * frames)
    p64, bound = _pred_bound(sd, sc, ospec, sds, False)
    assert _max_rel(pred, p64) <= bound


def test_forward_is_deterministic_and_stream_invariant(qa_lib, gpu_device, knob):
    """Two calls give the same bits, and so does the one-stream schedule (qa_set_serial) and a handle that re-uses its arena for
    encode in between."""
    ospec, sds, sd, codec = _mini(9811, gpu_device)
    T = ospec.enc_hop * 40
    x = synth.synth_wav(9812, 5, T).unsqueeze(1).to(gpu_device)
    f = synth.synth_feat(9813, 5, T // (ospec.enc_hop // 2), ospec.sem_in).to(gpu_device)
    a = [t.clone() for t in codec(x, f)]
    codec.encode(x, f)
    b = [t.clone() for t in codec(x, f)]
    knob("QA_SERIAL", 1)
    c = [t.clone() for t in codec(x, f)]
    torch.cuda.synchronize()
    for u, v, w in zip(a, b, c):
        assert torch.equal(u, v) and torch.equal(u, w)


def test_forward15_deterministic_and_serial(qa_lib, gpu_device, knob):
    gen = _gen()
    ospec = gen.spec_for("1.5")
    sd, wav, feat = gen.inputs("1.5", 9821, 3, 640 * 11, ospec)
    codec = _codec(sd, ospec, gpu_device)
    x, f = wav.unsqueeze(1).to(gpu_device), feat.to(gpu_device)
    a = {k: v.clone() for k, v in codec(x, f).items()}
    b = {k: v.clone() for k, v in codec(x, f).items()}
    knob("QA_SERIAL", 1)
    c = {k: v.clone() for k, v in codec(x, f).items()}
    torch.cuda.synchronize()
    for k in a:
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]), k


def test_forward_without_semantic_decoder_weights(qa_lib, gpu_device):
    """Encode / decode are unchanged with and without semantic_decoder.* loaded; forward refuses, naming the first missing or
    mis-shaped key."""
    import unified_audio_amd as qa

    ospec, sds, sd, full = _mini(9831, gpu_device)
    base = {k: v for k, v in sd.items() if not k.startswith("semantic_decoder.")}
    bare = _codec(base, ospec, gpu_device)
    assert full.has_semantic_decoder and not bare.has_semantic_decoder
    T = ospec.enc_hop * 12
    x = synth.synth_wav(9832, 2, T).unsqueeze(1).to(gpu_device)
    f = synth.synth_feat(9833, 2, T // (ospec.enc_hop // 2), ospec.sem_in).to(gpu_device)
    r1, r2 = _encode_decode(full, x, f), _encode_decode(bare, x, f)
    torch.cuda.synchronize()
    assert all(torch.equal(u, v) for u, v in zip(r1, r2))
    with pytest.raises(qa.QuarkAudioError, match="semantic_decoder.conv1.conv.weight"):
        bare(x, f)
    partial = dict(sd)
    del partial["semantic_decoder.conv_blocks.1.res_units.0.conv2.weight"]
    partial["semantic_decoder.conv_blocks.0.conv.deconv.bias"] = partial["semantic_decoder.conv_blocks.0.conv.deconv.bias"][:-1]
    with pytest.raises(qa.QuarkAudioError, match=r"semantic_decoder\.conv_blocks\.0\.conv\.deconv\.bias"):
        _codec(partial, ospec, gpu_device)(x, f)
    r3 = _encode_decode(_codec(partial, ospec, gpu_device), x, f)
    torch.cuda.synchronize()
    assert all(torch.equal(u, v) for u, v in zip(r1, r3))


def test_tokenizer_checkpoint_runs_forward(qa_lib, gpu_device, tmp_path):
    """A torch.save'd checkpoint with semantic_decoder.* loaded through HCodecTokenizer(pt_path): tok.model(x, feat) is the forward."""
    import unified_audio_amd as qa

    ospec, sds, sd, codec = _mini(9841, gpu_device)
    path = tmp_path / "codec.pt"
    torch.save(sd, path)
    tok = qa.HCodecTokenizer(str(path), device=gpu_device, spec=qa.HCodecSpec(**MINI))
    T = ospec.enc_hop * 9
    x = synth.synth_wav(9842, 2, T).unsqueeze(1).to(gpu_device)
    f = synth.synth_feat(9843, 2, T // (ospec.enc_hop // 2), ospec.sem_in).to(gpu_device)
    got, want = tok.model(x, f), codec(x, f)
    torch.cuda.synchronize()
    assert all(torch.equal(u, v) for u, v in zip(got, want))


def test_forward15_refuses_the_dynamic_threshold_draw(qa_lib, gpu_device):
    import unified_audio_amd as qa

    gen = _gen()
    ospec = gen.spec_for("1.5")
    sd, wav, feat = gen.inputs("1.5", 9851, 1, 640 * 4, ospec)
    codec = _codec(sd, ospec, gpu_device)
    codec.dynamic_threshold = True
    with pytest.raises(qa.QuarkAudioError, match="manual_threshold"):
        codec(wav.unsqueeze(1).to(gpu_device), feat.to(gpu_device))
    codec.encode(wav.unsqueeze(1).to(gpu_device), feat.to(gpu_device))  # encode is unchanged

