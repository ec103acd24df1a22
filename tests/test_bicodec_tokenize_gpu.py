"""BiCodec.tokenize / get_semantic_tokens / get_global_tokens (QuarkAudio-UniSE/model/bicodec/bicodec.py:151-180), BiCodecTokenizer.tokenize
(audio_tokenizer.py:93-103) and the feature normalisation in front of XLSR-53 through the C-ABI, against the fp64 CPU restatement
(tests/bicodec_tokenize_ref.py, pinned to the reference's own modules by tests/test_bicodec_tokenize_oracle_cpu.py) and the golden tokens
those modules produced (tools/gen_golden_bicodec_tokenize.py)."""
import copy
import os
import time

import numpy as np
import pytest
import torch
import yaml

from oracle import bicodec_ref as BR
from tests import bicodec_tokenize_ref as T
from tests import ref_configs as RC
from tests.util import audit_codes, rel_err
from unified_audio_amd import synth

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
STAGE_TOL = 5e-5      # small shapes, as tests/test_bicodec_gpu.py
WIDE_TOL = 2e-4       # published widths (12 ConvNeXt layers over 1024 -> 384 -> 2048)
SMALL = dict(input_channels=64, vocos_dim=32, vocos_inter=64, vocos_layers=2, latent_dim=64, codebook_size=128, codebook_dim=8)
TAPS = ("enc.backbone", "enc.down", "enc.out", "vq.latent")


def _espec(**kw):
    import unified_audio_amd as qa

    return qa.BiCodecEncoderSpec(**kw)


def _dspec(espec):
    """A detokenizer spec whose quantizer / prenet widths agree with the encoder spec (the published model shares them)."""
    import unified_audio_amd as qa

    if espec == qa.SPEC_BICODEC_ENCODER:
        return qa.SPEC_BICODEC
    return qa.BiCodecSpec(latent_dim=espec.latent_dim, codebook_size=espec.codebook_size, codebook_dim=espec.codebook_dim, spk_latent_dim=32,
                          token_num=4, vocos_dim=espec.vocos_dim, vocos_inter=espec.vocos_inter, vocos_layers=espec.vocos_layers,
                          gen_channels=256, rates=(4, 5, 2), kernel_sizes=(8, 11, 4))


def _model(espec, sd, device):
    import unified_audio_amd as qa

    return qa.BiCodec(_dspec(espec), device=device, encoder_spec=espec).load_state_dict(sd)


def _full_sd(espec, seed):
    """detokenize weights + tokenizer weights; the encoder generator's codebook is the one both halves use."""
    sd = synth.bicodec_state_dict(seed, _dspec(espec))
    sd.update(synth.bicodec_encoder_state_dict(seed + 1, espec))
    sd.update(synth.bicodec_speaker_state_dict(seed + 2, espec))
    return sd


def _audit(latent, sd, got, want):
    cb = T.normalized_codebook(sd).float().numpy()[None]
    return audit_codes(latent.float().numpy(), cb, got.reshape(-1, 1).cpu().numpy(), want.reshape(-1, 1).cpu().numpy())


def _parity(espec, seed, B, N, device):
    sd = _full_sd(espec, seed)
    m = _model(espec, sd, device).enable_taps()
    feat = synth.synth_feat(seed + 2, B, N, espec.input_channels).transpose(1, 2).contiguous()
    taps = {}
    want = T.get_semantic_tokens(T.cast(sd), feat.double(), espec.vocos_layers, taps)
    got = m.get_semantic_tokens({"feat": feat.to(device)})
    torch.cuda.synchronize()
    assert got.dtype == torch.int64 and got.shape == (B, N) and got.device.type == "cuda"
    report = {k: rel_err(m.tap(k), taps[k].float().flatten()) for k in TAPS}
    flips = _audit(taps["vq.latent"], sd, got, want)
    return report, flips, got.cpu(), want, sd, m, feat


def test_small_stage_parity_and_tokens(qa_lib, gpu_device):
    report, flips, got, want, *_ = _parity(_espec(**SMALL), 21, 3, 37, gpu_device)
    print(report, flips)
    assert all(v < STAGE_TOL for v in report.values()), report
    assert flips <= 0.002


def test_published_widths_stage_parity_and_token_diversity(qa_lib, gpu_device):
    import unified_audio_amd as qa

    report, flips, got, want, *_ = _parity(qa.SPEC_BICODEC_ENCODER, 31, 2, 150, gpu_device)
    print(report, flips)
    assert all(v < WIDE_TOL for v in report.values()), report
    assert flips <= 0.002
    assert len(torch.unique(got)) >= 200, len(torch.unique(got))  # 300 vectors over 8192 codes: not collapsed onto a few


@pytest.mark.parametrize("name", ["bicodec_tokenize_small", "bicodec_tokenize_published"])
def test_golden_tokens_reproduced(qa_lib, gpu_device, name):
    import importlib.util

    spec_ = importlib.util.spec_from_file_location("gen_golden_bicodec_tokenize", os.path.join(HERE, "..", "tools", "gen_golden_bicodec_tokenize.py"))
    G = importlib.util.module_from_spec(spec_)
    spec_.loader.exec_module(G)
    espec, sd, feat = G.case_inputs(name)
    g = np.load(os.path.join(HERE, "golden", name + ".npz"))
    sd = {**synth.bicodec_state_dict(3, _dspec(espec)), **synth.bicodec_speaker_state_dict(4, espec), **sd}
    got = _model(espec, sd, gpu_device).get_semantic_tokens({"feat": feat.to(gpu_device)})
    assert got.shape == g["tokens"].shape
    flips = _audit(torch.from_numpy(g["latent"]), sd, got, torch.from_numpy(g["tokens"]))
    assert flips <= 0.002


def test_batch_invariance_and_repeatability(qa_lib, gpu_device):
    espec = _espec(**SMALL)
    sd = _full_sd(espec, 41)
    m = _model(espec, sd, gpu_device)
    feat = synth.synth_feat(43, 5, 29, espec.input_channels).transpose(1, 2).contiguous().to(gpu_device)
    full = m.get_semantic_tokens({"feat": feat})
    assert torch.equal(full, m.get_semantic_tokens({"feat": feat}))
    m.enable_taps()
    m.get_semantic_tokens({"feat": feat})
    lat = m.tap("vq.latent").reshape(5, 29, -1)
    for b in range(5):
        assert torch.equal(m.get_semantic_tokens({"feat": feat[b:b + 1]})[0], full[b]), b
        assert torch.equal(m.tap("vq.latent").reshape(29, -1), lat[b]), b


def test_wav_normalize_matches_fp64_and_is_row_local(qa_lib, gpu_device):
    import unified_audio_amd as qa

    wav = (synth.synth_wav(51, 3, 96000 + 77) * torch.tensor([[1.0], [0.01], [3.0]]) + 0.2).float()
    want = T.wav_normalize(wav.double())
    got = qa.wav_normalize(wav.to(gpu_device))
    assert got.dtype == torch.float32 and got.shape == wav.shape
    assert float((got.cpu().double() - want).abs().max()) < 1e-5
    assert torch.equal(qa.wav_normalize(wav[1].to(gpu_device)), got[1])
    x = wav.to(gpu_device)  # out may alias the input at the C-ABI
    from unified_audio_amd import _lib

    _lib.check(_lib.load_library().qa_wav_normalize(x.data_ptr(), 3, x.shape[1], x.data_ptr(), 1e-7, torch.cuda.current_stream().cuda_stream))
    assert torch.equal(x, got)


def test_round_trip_matches_the_oracle_round_trip(qa_lib, gpu_device):
    espec = _espec(**SMALL)
    report, flips, got, want, sd, m, feat = _parity(espec, 61, 2, 24, gpu_device)
    glob = synth.bicodec_tokens(62, 2, 24, _dspec(espec))[1]
    wav_gpu = m.detokenize(got.to(gpu_device), glob.to(gpu_device)).cpu()
    wav_ref = BR.detokenize(sd, want, glob, BR.BiCodecSpec(**{f: getattr(_dspec(espec), f) for f in _dspec(espec).__dataclass_fields__}))
    assert wav_gpu.shape == wav_ref.shape
    if torch.equal(got, want):  # an audited near-tie flip changes the waveform by design
        assert rel_err(wav_gpu, wav_ref) < 1e-4


def test_detokenize_only_checkpoint_is_unchanged_and_names_what_is_missing(qa_lib, gpu_device):
    import unified_audio_amd as qa

    espec = _espec(**SMALL)
    dspec = _dspec(espec)
    detok = synth.bicodec_state_dict(71, dspec)
    full = {**synth.bicodec_encoder_state_dict(72, espec), **synth.bicodec_speaker_state_dict(75, espec), **detok}  # same detokenizer
    a = qa.BiCodec(dspec, device=gpu_device).load_state_dict(detok)
    b = _model(espec, full, gpu_device)
    assert not a.has_tokenizer and b.has_tokenizer
    sem, glob = synth.bicodec_tokens(73, 2, 20, dspec)
    assert torch.equal(a.detokenize(sem.to(gpu_device), glob.to(gpu_device)), b.detokenize(sem.to(gpu_device), glob.to(gpu_device)))
    feat = synth.synth_feat(74, 1, 10, espec.input_channels).transpose(1, 2).contiguous().to(gpu_device)
    for fn in (a.get_semantic_tokens, a.get_global_tokens, a.tokenize):
        with pytest.raises(qa.QuarkAudioError, match="encoder.encoder.embed.weight"):
            fn({"feat": feat, "ref_wav": torch.zeros(1, 16000), "wav": torch.zeros(1, 16000)})
    with pytest.raises(qa.QuarkAudioError, match="too short"):
        b.get_global_tokens({"ref_wav": torch.zeros(1, 512)})
    with pytest.raises(qa.QuarkAudioError, match=r"feat must be \[B, N, 64\]"):
        b.get_semantic_tokens({"feat": feat[..., :32]})
    for name in ("encoder.project.weight", "speaker_encoder.speaker_encoder.layer3.se_res2block.1.bns.4.running_var"):
        broken = dict(full)
        del broken[name]
        with pytest.raises(qa.QuarkAudioError, match=name.replace(".", r"\.")):
            _model(espec, broken, gpu_device)


def test_semantic_tokenizer_from_a_checkpoint_directory(qa_lib, gpu_device, tmp_path):
    """`BiCodec.load_from_checkpoint(model_dir)` builds the semantic tokenizer from config.yaml's encoder / quantizer blocks and the
    encoder.* entries of model.safetensors; the tokens equal those of the in-memory path."""
    import dataclasses

    import unified_audio_amd as qa
    from safetensors.torch import save_file

    config = copy.deepcopy(RC.small_bicodec_config())
    config["audio_tokenizer"]["encoder"].update(input_channels=64, vocos_dim=32, vocos_intermediate_dim=64, vocos_num_layers=2, out_channels=64)
    espec = qa.BiCodecEncoderSpec.from_config(config["audio_tokenizer"])
    assert espec == dataclasses.replace(_espec(**SMALL), spk_latent_dim=32)  # the speaker encoder's width comes from the file too
    dspec = qa.BiCodecSpec.from_config(config["audio_tokenizer"])
    sd = {**synth.bicodec_encoder_state_dict(81, espec), **synth.bicodec_speaker_state_dict(84, espec), **synth.bicodec_state_dict(82, dspec)}
    d = tmp_path / "BiCodec"
    d.mkdir()
    (d / "config.yaml").write_text(yaml.safe_dump(config))
    save_file({k: v.contiguous() for k, v in sd.items()}, str(d / "model.safetensors"))
    from_file = qa.BiCodec.load_from_checkpoint(str(d), device=gpu_device)
    from_dict = qa.BiCodec(dspec, device=gpu_device, encoder_spec=espec).load_state_dict(sd)
    feat = synth.synth_feat(83, 2, 33, 64).transpose(1, 2).contiguous().to(gpu_device)
    a, b = from_file.get_semantic_tokens({"feat": feat}), from_dict.get_semantic_tokens({"feat": feat})
    assert from_file.encoder_spec == espec and torch.equal(a, b)


def test_published_shapes_16_rows_of_6_seconds(qa_lib, gpu_device):
    """The bulk workload: 16 rows x 6 s (299 XLSR-53 frames each) at the published widths, seeded weights."""
    import unified_audio_amd as qa

    espec = qa.SPEC_BICODEC_ENCODER
    m = _model(espec, _full_sd(espec, 91), gpu_device)
    feat = synth.synth_feat(92, 16, 299, 1024).transpose(1, 2).contiguous().to(gpu_device)
    m.get_semantic_tokens({"feat": feat})
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tok = m.get_semantic_tokens({"feat": feat})
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert tok.shape == (16, 299) and int(tok.min()) >= 0 and int(tok.max()) < espec.codebook_size
    assert len(torch.unique(tok)) >= 1000
    assert dt < 2.0, dt  # generous: the encoder is ~57 MFLOP per frame, 0.3 TFLOP in all


def test_tokenizer_front_end_from_a_model_directory(qa_lib, gpu_device, tmp_path):
    """BiCodecTokenizer(model_dir): {model_dir}/BiCodec and, loaded on the first semantic call, {model_dir}/wav2vec2-large-xlsr-53
    (audio_tokenizer.py:44-52).  normalise -> XLSR-53 states 11 / 14 / 16 -> encoder -> VQ equals the in-memory path, and the
    features equal the CPU oracle's on the normalised rows."""
    import dataclasses
    import json

    import unified_audio_amd as qa
    from oracle import ssl_ref as SR
    from safetensors.torch import save_file

    xs = SR.SSLSpec(conv_dim=(32,) * 7, conv_bias=True, feat_extract_norm="layer", hidden_size=96, num_hidden_layers=16, num_attention_heads=3,
                    intermediate_size=192, do_stable_layer_norm=True, num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=2,
                    pad=0, select=(11, 14, 16), compress_exponent=0.0)
    ssl_sd = SR.synth_state_dict(101, xs, "wav2vec2")
    for sub in ("BiCodec", "wav2vec2-large-xlsr-53"):
        (tmp_path / sub).mkdir()
    config = copy.deepcopy(RC.small_bicodec_config())
    config["audio_tokenizer"]["encoder"].update(input_channels=96, vocos_dim=32, vocos_intermediate_dim=64, vocos_num_layers=2, out_channels=64)
    config["audio_tokenizer"]["speaker_encoder"].update(latent_dim=32, token_num=4)
    config["audio_tokenizer"]["prenet"].update(vocos_dim=32, vocos_intermediate_dim=64, vocos_num_layers=2)
    config["audio_tokenizer"]["decoder"].update(channels=256, rates=[4, 5, 2], kernel_sizes=[8, 11, 4])
    espec = qa.BiCodecEncoderSpec.from_config(config["audio_tokenizer"])
    assert espec == dataclasses.replace(_espec(**SMALL), input_channels=96, spk_latent_dim=32, token_num=4)
    dspec = _dspec(espec)
    assert qa.BiCodecSpec.from_config(config["audio_tokenizer"]) == dspec
    sd = _full_sd(espec, 102)
    (tmp_path / "BiCodec" / "config.yaml").write_text(yaml.safe_dump(config))
    save_file({k: v.contiguous() for k, v in sd.items()}, str(tmp_path / "BiCodec" / "model.safetensors"))
    (tmp_path / "config.yaml").write_text(yaml.safe_dump(RC.SPARKTTS_CONFIG))
    (tmp_path / "wav2vec2-large-xlsr-53" / "config.json").write_text(json.dumps(SR.hf_config(xs, "wav2vec2").to_dict(), default=str))
    save_file({k: v.contiguous() for k, v in ssl_sd.items()}, str(tmp_path / "wav2vec2-large-xlsr-53" / "model.safetensors"))

    tok = qa.BiCodecTokenizer(str(tmp_path), device=gpu_device)
    assert tok._feature_extractor is None  # constructing a tokenizer does not load XLSR-53
    wav = synth.synth_wav(103, 2, 16000)
    got = tok.get_semantic_tokens(wav.to(gpu_device))
    assert got.shape == (2, 49) and got.dtype == torch.int64
    qspec = qa.SSLSpec(**{f.name: getattr(xs, f.name) for f in dataclasses.fields(xs)})
    fx = qa.SSLFeatureExtractor(qspec, device=gpu_device).load_state_dict(ssl_sd)
    mem = qa.BiCodecTokenizer(model=_model(espec, sd, gpu_device), feature_extractor=fx)
    assert torch.equal(mem.get_semantic_tokens(wav.to(gpu_device)), got)
    feats = tok.extract_wav2vec2_features(wav.to(gpu_device))
    want = SR.extract_features(ssl_sd, T.wav_normalize(wav.double()).float(), xs)
    assert rel_err(feats, want) < 1e-4
    # the extractor H-Codec 1.5 uses (160-sample pad, |x|^0.3) is refused by name; so is a clip shorter than one frame
    with pytest.raises(qa.QuarkAudioError, match="SPEC_XLSR53_BICODEC"):
        qa.BiCodecTokenizer(model=mem.model, feature_extractor=qa.SSLFeatureExtractor(dataclasses.replace(qspec, pad=160, compress_exponent=0.3),
                                                                                      device=gpu_device))
    with pytest.raises(qa.QuarkAudioError, match="400 samples"):
        tok.get_semantic_tokens(wav[:, :399].to(gpu_device))
    # BiCodecTokenizer.tokenize: (global int32 [B, 1, 32], semantic int64 [B, N]); the 6 s reference clip is the 1 s row tiled
    glob, sem = tok.tokenize(wav.to(gpu_device))
    assert glob.dtype == torch.int32 and glob.shape == (2, 1, 4) and torch.equal(sem, got)
    assert tok.ref_segment_length == 96000
    assert torch.equal(glob, mem.model.get_global_tokens({"ref_wav": T.ref_clip(wav, 96000).to(gpu_device)}))


def _fsq_digits(tok, levels):
    basis = np.cumprod([1] + list(levels[:-1]))
    t = np.asarray(tok, np.int64).reshape(-1, 1)
    return (t // basis) % np.asarray(levels) - np.asarray(levels) // 2


def _audit_fsq(bounded, got, want, levels, tol=1e-3, max_frac=0.002):
    """An FSQ digit may differ from the oracle's only where the oracle's bounded value lies within tol of a k + 0.5 boundary."""
    b = bounded.reshape(-1, len(levels)).double().numpy()
    g, w = _fsq_digits(got.cpu(), levels), _fsq_digits(want.cpu(), levels)
    differ = g != w
    margin = np.abs(np.abs(b - np.floor(b)) - 0.5)
    assert (margin[differ] <= tol).all(), f"decisive FSQ digit mismatches: margins {margin[differ]}"
    frac = float(differ.any(1).mean())
    assert frac <= max_frac, frac
    return frac


GTAPS = ("mel", "ecapa.layer1", "ecapa.layers234", "ecapa.latent", "perceiver.out", "fsq.bounded")


def _global_parity(m, sd, espec, wav, ref_len, device):
    taps = {}
    clip = T.ref_clip(wav, ref_len) if ref_len else wav
    want = T.get_global_tokens(T.cast(sd), clip.double(), espec.mel_params, espec.fsq_levels, taps=taps)
    m.enable_taps()
    got = m.get_global_tokens({"ref_wav": wav.to(device)}, ref_len)
    torch.cuda.synchronize()
    assert got.dtype == torch.int32 and got.shape == (wav.shape[0], 1, espec.token_num)
    taps["ecapa.layers234"] = torch.cat([taps[f"ecapa.layer{i}"] for i in (2, 3, 4)], -1)
    report = {k: rel_err(m.tap(k), taps[k].float().flatten()) for k in GTAPS}
    frac = _audit_fsq(taps["fsq.bounded"], got[:, 0], want, espec.fsq_levels)
    return report, frac, got, want


def test_global_tokens_stage_parity(qa_lib, gpu_device):
    import unified_audio_amd as qa

    espec = qa.SPEC_BICODEC_ENCODER
    sd = _full_sd(espec, 111)
    m = _model(espec, sd, gpu_device)
    wav = synth.synth_wav(112, 3, 16000 + 123) * torch.tensor([[1.0], [0.3], [2.0]])
    report, frac, got, want = _global_parity(m, sd, espec, wav, 0, gpu_device)
    print(report, frac)
    assert all(v < WIDE_TOL for v in report.values()), report


@pytest.mark.parametrize("seconds", [1.5, 8.0])
def test_reference_clip_tiled_and_truncated(qa_lib, gpu_device, seconds):
    """get_ref_clip as index arithmetic: a row shorter than 6 s is tiled, a longer one truncated (audio_tokenizer.py:54-72)."""
    import unified_audio_amd as qa

    espec = qa.SPEC_BICODEC_ENCODER
    sd = _full_sd(espec, 121)
    m = _model(espec, sd, gpu_device)
    wav = synth.synth_wav(122, 2, int(16000 * seconds))
    report, frac, got, want = _global_parity(m, sd, espec, wav, 96000, gpu_device)
    assert all(v < WIDE_TOL for v in report.values()), report
    assert torch.equal(got, m.get_global_tokens({"ref_wav": T.ref_clip(wav, 96000).to(gpu_device)}))


def test_global_batch_invariance_and_repeatability(qa_lib, gpu_device):
    import unified_audio_amd as qa

    espec = qa.SPEC_BICODEC_ENCODER
    m = _model(espec, _full_sd(espec, 131), gpu_device)
    wav = synth.synth_wav(132, 4, 20000).to(gpu_device)
    full = m.get_global_tokens({"ref_wav": wav})
    assert torch.equal(full, m.get_global_tokens({"ref_wav": wav}))
    for b in range(4):
        assert torch.equal(m.get_global_tokens({"ref_wav": wav[b:b + 1]})[0], full[b]), b


def test_published_round_trip_matches_the_oracle_round_trip(qa_lib, gpu_device):
    """detokenize(tokenize(batch)) on the GPU against the same round trip of the CPU oracle (restatement + oracle/bicodec_ref.py)."""
    import unified_audio_amd as qa

    espec = qa.SPEC_BICODEC_ENCODER
    sd = _full_sd(espec, 141)
    m = _model(espec, sd, gpu_device)
    feat = synth.synth_feat(142, 1, 49, espec.input_channels).transpose(1, 2).contiguous()
    wav = synth.synth_wav(143, 1, 16000)
    sem, glob = m.tokenize({"feat": feat.to(gpu_device), "ref_wav": wav.to(gpu_device), "wav": wav.to(gpu_device)}, ref_len=96000)
    assert sem.dtype == torch.int64 and sem.shape == (1, 49) and glob.dtype == torch.int32 and glob.shape == (1, 1, 32)
    sd64 = T.cast(sd)
    sem_o = T.get_semantic_tokens(sd64, feat.double(), espec.vocos_layers)
    glob_o = T.get_global_tokens(sd64, T.ref_clip(wav, 96000).double(), espec.mel_params, espec.fsq_levels).unsqueeze(1)
    wav_gpu = m.detokenize(sem, glob).cpu()
    wav_ref = BR.detokenize(sd, sem_o, glob_o.long(), BR.SPEC_BICODEC)
    assert wav_gpu.shape == wav_ref.shape == (1, 1, 49 * 320)
    if torch.equal(sem.cpu(), sem_o) and torch.equal(glob.cpu(), glob_o):  # an audited near-tie flip changes the waveform by design
        assert rel_err(wav_gpu, wav_ref) < 1e-4


def test_published_tokenize_16_rows_of_6_seconds(qa_lib, gpu_device):
    """BiCodec.tokenize at the published shapes, 16 rows x 6 s: runs, tokens in range, the FSQ levels and codebook used."""
    import unified_audio_amd as qa

    espec = qa.SPEC_BICODEC_ENCODER
    m = _model(espec, _full_sd(espec, 151), gpu_device)
    feat = synth.synth_feat(152, 16, 299, 1024).transpose(1, 2).contiguous().to(gpu_device)
    wav = synth.synth_wav(153, 16, 96000).to(gpu_device)
    batch = {"feat": feat, "ref_wav": wav, "wav": wav}
    m.tokenize(batch)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sem, glob = m.tokenize(batch)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert int(sem.min()) >= 0 and int(sem.max()) < espec.codebook_size and len(torch.unique(sem)) >= 1000
    assert int(glob.min()) >= 0 and int(glob.max()) < 4 ** 6
    digits = _fsq_digits(glob.cpu(), espec.fsq_levels)
    assert all(len(np.unique(digits[:, d])) >= 3 for d in range(6)), [len(np.unique(digits[:, d])) for d in range(6)]
    assert dt < 2.0, dt


def test_golden_global_tokens_reproduced(qa_lib, gpu_device):
    """The reference's own SpeakerEncoder.tokenize on the mel of a tiled 6 s reference clip (tools/gen_golden_bicodec_tokenize.py)."""
    import importlib.util

    spec_ = importlib.util.spec_from_file_location("gen_golden_bicodec_tokenize", os.path.join(HERE, "..", "tools", "gen_golden_bicodec_tokenize.py"))
    G = importlib.util.module_from_spec(spec_)
    spec_.loader.exec_module(G)
    espec, spk_sd, wav, ref_len = G.global_case_inputs("bicodec_tokenize_global_published")
    g = np.load(os.path.join(HERE, "golden", "bicodec_tokenize_global_published.npz"))
    sd = {**synth.bicodec_state_dict(3, _dspec(espec)), **synth.bicodec_encoder_state_dict(4, espec), **spk_sd}
    m = _model(espec, sd, gpu_device).enable_taps()
    got = m.get_global_tokens({"ref_wav": wav.to(gpu_device)}, ref_len)
    mel = m.tap("mel").reshape(wav.shape[0], -1, espec.mel_dim)[:, ::10].cpu()
    assert rel_err(mel, torch.from_numpy(g["mel"])) < STAGE_TOL
    assert got.shape == g["tokens"].shape
    _audit_fsq(torch.from_numpy(g["bounded"]), got[:, 0], torch.from_numpy(g["tokens"])[:, 0], espec.fsq_levels)
