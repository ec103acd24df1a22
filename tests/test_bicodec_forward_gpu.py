"""BiCodec.forward (QuarkAudio-UniSE/model/bicodec/bicodec.py:113-149, eval mode) on the HIP path: the reference's dict, recons and
d_vector equal to detokenize(*tokenize(batch)), pred_feat and x_vector against the fp64 restatement (tests/bicodec_forward_ref.py) on the
path's own tokens / ECAPA latent, the code statistics, and the goldens the reference's own modules produced
(tools/gen_golden_bicodec_forward.py)."""
import importlib.util
import math
import os

import numpy as np
import pytest
import torch
import yaml

from tests import bicodec_forward_ref as F
from tests import bicodec_tokenize_ref as T
from tests.util import rel_err
from unified_audio_amd import synth

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
KEYS = ["vq_loss", "perplexity", "cluster_size", "recons", "pred_feat", "x_vector", "d_vector", "audios", "with_speaker_loss"]
PPL_TOL = 1e-6  # relative: fp32 p_k, fp64 log and sum, one rounding of exp to fp32
# ASTP statistics element by element against fp64 on the same latent: the kernel sums in fp64, so what is left is the fp32 rounding of
# the attention logits (linear2 on conv_gemm) and of the result; relative to max(|value|, 1e-3)
POOL_TOL = 2e-5


def _pool_err(a, ref):
    a, ref = a.double().cpu(), ref.double().cpu()
    return float(((a - ref).abs() / ref.abs().clamp_min(1e-3)).max())


def _gen():
    path = os.path.join(HERE, "..", "tools", "gen_golden_bicodec_forward.py")
    spec = importlib.util.spec_from_file_location("gen_golden_bicodec_forward", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _max_rel(a, ref):
    a, ref = a.double().cpu(), ref.double().cpu()
    return float((a - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


def _model(dspec, espec, fspec, sd, device):
    import unified_audio_amd as qa

    return qa.BiCodec(dspec, device=device, encoder_spec=espec, forward_spec=fspec).load_state_dict(sd)


def _case(name, device):
    gen = _gen()
    dspec, espec, fspec, sd, feat, wav = gen.case_inputs(name)
    m = _model(dspec, espec, fspec, sd, device)
    batch = {"feat": feat.to(device), "ref_wav": wav.to(device), "wav": wav.to(device)}
    return gen, dspec, espec, fspec, sd, m, batch


def _pred_bound(sd, sem, glob, dspec, fspec):
    """fp64 restatement on the given tokens, and 4 x the fp32 restatement's own distance from it"""
    p64 = F.pred_feat(sd, sem.cpu(), glob.cpu(), dspec, fspec.vocos_layers, torch.float64, fspec.use_tanh_at_final)
    p32 = F.pred_feat(sd, sem.cpu(), glob.cpu(), dspec, fspec.vocos_layers, torch.float32, fspec.use_tanh_at_final)
    return p64, 4 * max(_max_rel(p32, p64), 1e-6)


def _xvec_bound(sd, latent):
    """fp64 x-vector head on the given ECAPA latent, and 4 x the fp32 head's own distance from it"""
    with torch.no_grad():
        x64 = F.x_vector(T.cast(sd), latent.double())
        x32 = F.x_vector(T.cast(sd, torch.float32), latent.float())
    return x64, 4 * max(_max_rel(x32, x64), 1e-6)


@pytest.mark.parametrize("name", ["bicodec_forward_small", "bicodec_forward_published_1s"])
def test_forward_keys_shapes_dtypes(qa_lib, gpu_device, name):
    gen, dspec, espec, fspec, sd, m, batch = _case(name, gpu_device)
    assert m.has_forward
    out = m(batch)
    torch.cuda.synchronize()
    B, N = batch["feat"].shape[:2]
    assert list(out) == KEYS
    assert out["vq_loss"].dim() == 0 and out["vq_loss"].dtype == torch.float32 and math.isnan(float(out["vq_loss"]))
    for k in ("perplexity", "cluster_size"):
        assert out[k].dim() == 0 and out[k].dtype == torch.float32 and out[k].device == gpu_device
    want = {"recons": (B, 1, N * dspec.hop), "pred_feat": (B, fspec.out_channels, N), "x_vector": (B, fspec.xvector_dim),
            "d_vector": (B, dspec.latent_dim), "audios": (B, 1, batch["wav"].shape[1])}
    for k, shape in want.items():
        assert tuple(out[k].shape) == shape and out[k].dtype == torch.float32 and out[k].device.type == "cuda", k
    assert out["with_speaker_loss"] is False
    assert torch.equal(out["audios"], batch["wav"].unsqueeze(1))
    with pytest.raises(KeyError):
        m({"feat": batch["feat"], "ref_wav": batch["ref_wav"]})


@pytest.mark.parametrize("name", ["bicodec_forward_small", "bicodec_forward_published_1s"])
def test_forward_matches_tokenize_detokenize_fp64_and_golden(qa_lib, gpu_device, name):
    gen, dspec, espec, fspec, sd, m, batch = _case(name, gpu_device)
    m.enable_taps()
    out = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in m(batch).items()}
    x_tap, latent = m.tap("x_vector"), m.tap("ecapa.latent")
    sem, glob = m.tokenize(batch)
    wav = m.detokenize(sem, glob)
    d_tap = m.tap("d_vector")
    torch.cuda.synchronize()
    B, N = sem.shape
    # recons and d_vector: the detokenize kernels on the tokenize kernels' tokens
    assert torch.equal(out["recons"], wav)
    assert torch.equal(out["d_vector"].flatten(), d_tap)
    assert torch.equal(out["x_vector"].flatten(), x_tap)
    # pred_feat: fp64 restatement on the path's own tokens
    p64, pbound = _pred_bound(sd, sem, glob.reshape(B, -1), dspec, fspec)
    e_pred = _max_rel(out["pred_feat"], p64)
    # x_vector: fp64 head on the path's own ECAPA latent
    x64, xbound = _xvec_bound(sd, latent.reshape(B, -1, 1536).cpu())
    e_x = _max_rel(out["x_vector"], x64)
    # statistics
    ppl = F.perplexity_exact(sem.cpu(), espec.codebook_size)
    e_ppl = abs(float(out["perplexity"]) - ppl) / ppl
    print(f"{name}: pred_feat {e_pred:.2e} (bound {pbound:.2e}), x_vector {e_x:.2e} (bound {xbound:.2e}), perplexity {e_ppl:.1e}")
    assert e_pred <= pbound and e_x <= xbound and e_ppl <= PPL_TOL
    assert float(out["cluster_size"]) == len(torch.unique(sem))
    # the reference's own forward
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    g_sem, g_glob = torch.from_numpy(g["semantic_tokens"]), torch.from_numpy(g["global_tokens"])
    assert g_sem.shape == sem.shape and tuple(g["recons"].shape) == tuple(out["recons"].shape)
    if torch.equal(sem.cpu(), g_sem) and torch.equal(glob.reshape(B, -1).cpu().long(), g_glob):
        assert rel_err(out["recons"], torch.from_numpy(g["recons"])) < 1e-4
        g64, _ = _pred_bound(sd, g_sem, g_glob, dspec, fspec)
        g_pred = torch.from_numpy(g["pred_feat"])
        assert _max_rel(out["pred_feat"][:, ::gen.PRED_STRIDE], g_pred) <= pbound + _max_rel(g_pred, g64[:, ::gen.PRED_STRIDE])
        assert float(out["cluster_size"]) == float(g["cluster_size"])
        assert abs(float(out["perplexity"]) - float(g["perplexity"])) <= 2e-6 * ppl
    else:  # a near-tie token flip: detokenize of the reference's tokens
        print(f"{name}: tokens differ from the golden's")
        assert rel_err(m.detokenize(g_sem.to(gpu_device), g_glob.to(gpu_device)), torch.from_numpy(g["recons"])) < 1e-4
    # x_vector against the reference's own: both from fp32 mel / ECAPA chains, within the larger of 4 x the golden's distance to the fp64
    # chain and 1e-4
    with torch.no_grad():
        sd64 = T.cast(sd)
        lat64 = T.ecapa_latent(sd64, T.mel_spectrogram(batch["ref_wav"].cpu().double(), espec.mel_params))
        xc64 = F.x_vector(sd64, lat64)
    g_x = torch.from_numpy(g["x_vector"])
    assert _max_rel(out["x_vector"], xc64) <= max(4 * _max_rel(g_x, xc64), 1e-4)


@pytest.mark.parametrize("frames,B", [(3, 1), (37, 2), (301, 16), (1501, 2)])
def test_xvector_head_fp64(qa_lib, gpu_device, frames, B):
    """ASTP over T mel frames (T not a multiple of the 4 frame slices, up to 30 s of reference audio) for B items."""
    gen = _gen()
    dspec, espec, fspec = gen.specs(True)
    sd = synth.bicodec_state_dict(61, dspec)
    sd.update(synth.bicodec_encoder_state_dict(62, espec))
    sd.update(synth.bicodec_speaker_state_dict(63, espec))
    sd.update(synth.bicodec_forward_state_dict(64, fspec))
    m = _model(dspec, espec, fspec, sd, gpu_device).enable_taps()
    samples = (frames - 1) * espec.hop_length
    wav = synth.synth_wav(65 + frames, B, samples).to(gpu_device)
    feat = synth.synth_feat(66, B, 6, espec.input_channels).transpose(1, 2).contiguous().to(gpu_device)
    out = m({"feat": feat, "ref_wav": wav, "wav": wav})
    latent = m.tap("ecapa.latent").reshape(B, frames, 1536).cpu()
    pool = m.tap("ecapa.pool").reshape(B, 3072).cpu()
    torch.cuda.synchronize()
    x64, bound = _xvec_bound(sd, latent)
    e = _max_rel(out["x_vector"], x64)
    taps = {}
    with torch.no_grad():
        F.x_vector(T.cast(sd), latent.double(), taps)
    e_pool = _pool_err(pool, taps["ecapa.pool"])
    print(f"T={frames} B={B}: x_vector {e:.2e} (bound {bound:.2e}), pool element-wise {e_pool:.2e} (bound {POOL_TOL:.0e})")
    assert e <= bound and e_pool <= POOL_TOL
    if frames == 37:  # the bound is tight: one pool.linear2 weight scaled by 1 + 2^-10 breaks it - the weight from the tanh unit that
        # varies most over the frames (a weight from a unit that is constant over the frames cancels in the softmax)
        key = "speaker_encoder.speaker_encoder.pool.linear2.weight"
        sd64 = T.cast(sd)
        x = latent.double().transpose(1, 2)
        ctx = torch.cat((x, x.mean(-1, keepdim=True).expand_as(x), torch.sqrt(torch.var(x, -1, keepdim=True) + 1e-7).expand_as(x)), 1)
        a = torch.tanh(torch.nn.functional.conv1d(ctx, sd64["speaker_encoder.speaker_encoder.pool.linear1.weight"],
                                                  sd64["speaker_encoder.speaker_encoder.pool.linear1.bias"]))
        k = int(torch.argmax(a.std(-1).mean(0)))
        w = sd[key].clone()
        c = int(torch.argmax(w[:, k, 0].abs()))
        w[c, k, 0] *= 1 + 2 ** -10
        m2 = _model(dspec, espec, fspec, {**sd, key: w}, gpu_device).enable_taps()
        m2({"feat": feat, "ref_wav": wav, "wav": wav})
        e2 = _pool_err(m2.tap("ecapa.pool").reshape(B, 3072), taps["ecapa.pool"])
        torch.cuda.synchronize()
        print(f"perturbed pool.linear2[{c}, {k}]: pool element-wise {e2:.2e}")
        assert e2 > POOL_TOL


def test_pred_feat_bound_is_tight(qa_lib, gpu_device):
    gen, dspec, espec, fspec, sd, m, batch = _case("bicodec_forward_small", gpu_device)
    out = m(batch)
    sem, glob = m.tokenize(batch)
    torch.cuda.synchronize()
    p64, bound = _pred_bound(sd, sem, glob.reshape(sem.shape[0], -1), dspec, fspec)
    assert _max_rel(out["pred_feat"], p64) <= bound
    bad = dict(sd)
    key = "postnet.linear.weight"
    w = sd[key].clone()
    w.view(-1)[int(torch.argmax(w.abs()))] *= 1 + 2 ** -10
    bad[key] = w
    out2 = _model(dspec, espec, fspec, bad, gpu_device)(batch)
    torch.cuda.synchronize()
    e2 = _max_rel(out2["pred_feat"], p64)
    print(f"perturbed {key}: {e2:.2e} against bound {bound:.2e}")
    assert e2 > bound


def test_statistics_deterministic_and_batch_level(qa_lib, gpu_device):
    gen, dspec, espec, fspec, sd, m, batch = _case("bicodec_forward_small", gpu_device)
    a = m(batch)
    a = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in a.items()}
    b = m(batch)
    torch.cuda.synchronize()
    for k in KEYS:
        if k == "vq_loss":
            assert math.isnan(float(b[k]))
        elif torch.is_tensor(a[k]):
            assert torch.equal(a[k], b[k]), k
    sem = m.get_semantic_tokens(batch).cpu()
    assert sem.shape[0] == 2
    whole = F.perplexity_exact(sem, espec.codebook_size)
    items = [F.perplexity_exact(sem[i], espec.codebook_size) for i in range(2)]
    ppl = float(a["perplexity"])
    assert abs(ppl - whole) <= PPL_TOL * whole and all(abs(ppl - p) > 1e-3 * p for p in items)
    assert float(a["cluster_size"]) == len(torch.unique(sem))


def _code_usage(lib, idx, K):
    out = torch.empty(2, dtype=torch.float32, device=idx.device)
    from unified_audio_amd import _lib

    _lib.check(lib.qa_code_usage(idx.data_ptr(), idx.numel(), K, out[0:1].data_ptr(), out[1:2].data_ptr(),
                                 torch.cuda.current_stream(idx.device).cuda_stream))
    torch.cuda.synchronize()
    return float(out[0]), float(out[1]), out


def test_code_usage_kernel(qa_lib, gpu_device):
    K = 8192
    same = torch.full((2 * 50,), 1234, dtype=torch.int64, device=gpu_device)
    assert _code_usage(qa_lib, same, K)[:2] == (1.0, 1.0)
    once = torch.randperm(K, generator=torch.Generator().manual_seed(3)).to(gpu_device)
    ppl, active, _ = _code_usage(qa_lib, once, K)
    assert active == K and abs(ppl - K) <= PPL_TOL * K
    rng = np.random.default_rng(7)
    idx = torch.from_numpy(rng.integers(0, 300, size=64 * 301)).to(gpu_device)
    ppl, active, o1 = _code_usage(qa_lib, idx, K)
    _, _, o2 = _code_usage(qa_lib, idx, K)
    want = F.perplexity_exact(idx.cpu(), K)
    assert torch.equal(o1, o2) and active == len(torch.unique(idx)) and abs(ppl - want) <= PPL_TOL * want
    p64, a64 = F.code_stats(idx.cpu(), K)
    assert abs(ppl - float(p64)) <= PPL_TOL * float(p64) and active == float(a64)


def test_weights_without_forward_head(qa_lib, gpu_device, tmp_path):
    """tokenize / detokenize are bit-identical without postnet.* / the pool head; forward names the first missing key; a detokenize-only
    dict refuses with -3; a config.yaml postnet value forward has no path for loads and is refused by name only by forward."""
    import unified_audio_amd as qa

    gen, dspec, espec, fspec, sd, full, batch = _case("bicodec_forward_small", gpu_device)
    base = {k: v for k, v in sd.items() if not k.startswith("postnet.")}
    bare = _model(dspec, espec, fspec, base, gpu_device)
    assert full.has_forward and not bare.has_forward
    r1 = full.tokenize(batch)
    r2 = bare.tokenize(batch)
    w1, w2 = full.detokenize(*r1), bare.detokenize(*r2)
    torch.cuda.synchronize()
    assert all(torch.equal(u, v) for u, v in zip(r1, r2)) and torch.equal(w1, w2)
    with pytest.raises(qa.QuarkAudioError, match=r"postnet\.linear_pre\.weight"):
        bare(batch)
    partial = dict(sd)
    del partial["speaker_encoder.speaker_encoder.bn.running_var"]
    with pytest.raises(qa.QuarkAudioError, match=r"speaker_encoder\.speaker_encoder\.bn\.running_var"):
        _model(dspec, espec, fspec, partial, gpu_device)(batch)
    detok = {k: v for k, v in sd.items() if k.startswith(("quantizer.codebook", "quantizer.out_project", "speaker_encoder.quantizer.project_out",
                                                          "speaker_encoder.project.", "prenet.", "decoder."))}
    with pytest.raises(qa.QuarkAudioError) as ei:
        _model(dspec, espec, fspec, detok, gpu_device)(batch)
    assert ei.value.status == -3
    # config.yaml with a postnet the forward kernels cannot run (a condition): detokenize and tokenize load, forward refuses by name
    from safetensors.torch import save_file

    cfg = {"audio_tokenizer": {
        "mel_params": espec.mel_params,
        "encoder": dict(input_channels=espec.input_channels, vocos_dim=espec.vocos_dim, vocos_intermediate_dim=espec.vocos_inter,
                        vocos_num_layers=espec.vocos_layers, out_channels=espec.latent_dim, sample_ratios=[1, 1]),
        "decoder": dict(input_channel=dspec.latent_dim, channels=dspec.gen_channels, rates=list(dspec.rates), kernel_sizes=list(dspec.kernel_sizes)),
        "quantizer": dict(input_dim=dspec.latent_dim, codebook_size=dspec.codebook_size, codebook_dim=dspec.codebook_dim, commitment=0.25),
        "speaker_encoder": dict(input_dim=espec.mel_dim, out_dim=fspec.xvector_dim, latent_dim=espec.spk_latent_dim, token_num=espec.token_num,
                                fsq_levels=list(espec.fsq_levels), fsq_num_quantizers=1),
        "prenet": dict(input_channels=dspec.latent_dim, vocos_dim=dspec.vocos_dim, vocos_intermediate_dim=dspec.vocos_inter,
                       vocos_num_layers=dspec.vocos_layers, out_channels=dspec.latent_dim, condition_dim=dspec.latent_dim, sample_ratios=[1, 1]),
        "postnet": dict(input_channels=fspec.input_channels, vocos_dim=fspec.vocos_dim, vocos_intermediate_dim=fspec.vocos_inter,
                        vocos_num_layers=fspec.vocos_layers, out_channels=fspec.out_channels, condition_dim=fspec.input_channels)}}
    (tmp_path / "config.yaml").write_text(yaml.safe_dump(cfg))
    save_file({k: v.contiguous() for k, v in sd.items() if v.is_floating_point()}, str(tmp_path / "model.safetensors"))
    m = qa.BiCodec.load_from_checkpoint(str(tmp_path), device=gpu_device)
    r3 = m.tokenize(batch)
    w3 = m.detokenize(*r3)
    torch.cuda.synchronize()
    assert all(torch.equal(u, v) for u, v in zip(r1, r3)) and torch.equal(w1, w3)
    with pytest.raises(qa.QuarkAudioError, match=r"postnet\.condition_dim") as ei:
        m(batch)
    assert ei.value.status == -4
    cfg["audio_tokenizer"]["postnet"]["no_such_key"] = 1
    (tmp_path / "config.yaml").write_text(yaml.safe_dump(cfg))
    with pytest.raises(TypeError, match="no_such_key"):
        qa.BiCodec.load_from_checkpoint(str(tmp_path), device=gpu_device)
