"""Pins tests/bicodec_tokenize_ref.py (BiCodec.tokenize) to the reference's OWN Encoder, FactorizedVectorQuantize and SpeakerEncoder
(QuarkAudio-UniSE/model/bicodec/modules/*, skipped where the reference tree is absent), its normalisation to transformers'
Wav2Vec2FeatureExtractor and its mel front to transformers.audio_utils, and checks BiCodecEncoderSpec.from_config."""
import copy
import warnings

import numpy as np
import pytest
import torch

from oracle import ref_bicodec_shim as RS
from tests import bicodec_tokenize_ref as T
from tests import ref_configs as RC
from unified_audio_amd import synth
from unified_audio_amd.bicodec import SPEC_BICODEC_ENCODER, BiCodecEncoderSpec

SMALL = BiCodecEncoderSpec(input_channels=64, vocos_dim=32, vocos_inter=64, vocos_layers=2, latent_dim=64, codebook_size=128, codebook_dim=8)
need_ref = pytest.mark.skipif(not RS.reference_available(), reason="reference tree not present")


def _reference_modules(spec):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        enc = RS._import("encoder_decoder.feat_encoder")
        fvq = RS._import("vq.factorized_vector_quantize")
        m = torch.nn.Module()
        m.encoder = enc.Encoder(input_channels=spec.input_channels, vocos_dim=spec.vocos_dim, vocos_intermediate_dim=spec.vocos_inter,
                                vocos_num_layers=spec.vocos_layers, out_channels=spec.latent_dim, sample_ratios=[1, 1])
        m.quantizer = fvq.FactorizedVectorQuantize(input_dim=spec.latent_dim, codebook_size=spec.codebook_size,
                                                   codebook_dim=spec.codebook_dim, commitment=0.25)
    return m.eval()


@need_ref
@pytest.mark.parametrize("which", ["small", "published"])
def test_restatement_matches_reference_encoder_and_quantizer(which):
    spec = SMALL if which == "small" else SPEC_BICODEC_ENCODER
    sd = synth.bicodec_encoder_state_dict(5, spec)
    m = _reference_modules(spec)
    want_keys = {k for k in m.state_dict() if not k.endswith("cluster_size") and "out_project" not in k}
    assert set(sd) == want_keys, set(sd) ^ want_keys
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.endswith("cluster_size") or "out_project" in k for k in missing), (missing, unexpected)
    B, N = 2, 40 if which == "small" else 60
    feat = synth.synth_feat(6, B, N, spec.input_channels).transpose(1, 2).contiguous()  # [B, N, C_in]
    with torch.no_grad():
        z_ref = m.encoder(feat.transpose(1, 2))                                        # bicodec.py:170, [B, latent, N]
        tok_ref = m.quantizer.tokenize(z_ref)                                          # bicodec.py:171
    taps = {}
    tok = T.get_semantic_tokens(sd, feat, spec.vocos_layers, taps)
    assert torch.allclose(taps["enc.out"], z_ref.transpose(1, 2), rtol=1e-5, atol=1e-5)
    assert tok.dtype == tok_ref.dtype == torch.int64 and torch.equal(tok, tok_ref)
    # the fp64 restatement the GPU tests compare against picks the same codes
    tok64 = T.get_semantic_tokens(T.cast(sd), feat.double(), spec.vocos_layers)
    assert float((tok64 == tok_ref).double().mean()) >= 0.99
    assert len(torch.unique(tok_ref)) >= min(spec.codebook_size // 4, B * N // 3)  # seeded weights give diverse tokens


def test_normalisation_matches_wav2vec2_feature_extractor():
    tf = pytest.importorskip("transformers")
    fe = tf.Wav2Vec2FeatureExtractor(feature_size=1, sampling_rate=16000, padding_value=0.0, do_normalize=True, return_attention_mask=True)
    wav = (synth.synth_wav(3, 3, 16000 + 77) * torch.tensor([[1.0], [0.01], [3.0]]) + 0.2).float()
    want = fe(wav.numpy(), sampling_rate=16000, return_tensors="pt", padding=True).input_values  # audio_tokenizer.py:78-84
    got = T.wav_normalize(wav.double()).float()
    assert want.shape == got.shape
    assert float((got - want).abs().max()) < 2e-5


def test_encoder_spec_from_config_published_and_small():
    assert BiCodecEncoderSpec.from_config(RC.BICODEC_CONFIG["audio_tokenizer"]) == SPEC_BICODEC_ENCODER
    c = copy.deepcopy(RC.BICODEC_CONFIG["audio_tokenizer"])
    c["encoder"].update(input_channels=64, vocos_dim=32, vocos_intermediate_dim=64, vocos_num_layers=2, out_channels=64)
    c["quantizer"].update(input_dim=64, codebook_size=128)
    assert BiCodecEncoderSpec.from_config(c) == SMALL


def test_encoder_spec_refuses_by_name():
    import unified_audio_amd as qa

    base = RC.BICODEC_CONFIG["audio_tokenizer"]
    for block, key, value, word in (("encoder", "sample_ratios", [2, 2], "sample_ratios"), ("quantizer", "codebook_dim", 1024, "codebook_dim")):
        c = copy.deepcopy(base)
        c[block][key] = value
        with pytest.raises(qa.QuarkAudioError, match=word):
            BiCodecEncoderSpec.from_config(c)
    c = copy.deepcopy(base)
    c["encoder"]["out_channels"] = 512
    with pytest.raises(ValueError, match="out_channels"):
        BiCodecEncoderSpec.from_config(c)
    c = copy.deepcopy(base)
    c["encoder"]["use_tanh_at_final"] = True
    with pytest.raises(TypeError, match="unexpected"):
        BiCodecEncoderSpec.from_config(c)
    c = copy.deepcopy(base)
    del c["encoder"]["vocos_dim"]
    with pytest.raises(TypeError, match="missing"):
        BiCodecEncoderSpec.from_config(c)
    with pytest.raises(KeyError):
        BiCodecEncoderSpec.from_config({k: v for k, v in base.items() if k != "encoder"})


def test_synth_encoder_weights_are_seeded():
    a = synth.bicodec_encoder_state_dict(9, SMALL)
    b = synth.bicodec_encoder_state_dict(9, SMALL)
    assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)
    assert not torch.equal(a["encoder.project.weight"], synth.bicodec_encoder_state_dict(10, SMALL)["encoder.project.weight"])
    assert np.isfinite(sum(float(v.abs().sum()) for v in a.values()))


@need_ref
def test_global_restatement_matches_reference_speaker_encoder():
    """SpeakerEncoder.tokenize (speaker_encoder.py, the reference's own ECAPA-TDNN / PerceiverResampler / ResidualFSQ) on mel input."""
    spec = SPEC_BICODEC_ENCODER
    sd = synth.bicodec_speaker_state_dict(5, spec)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        spk = RS._import("speaker.speaker_encoder").SpeakerEncoder(input_dim=spec.mel_dim, out_dim=1024, latent_dim=spec.spk_latent_dim,
                                                                  token_num=spec.token_num, fsq_levels=list(spec.fsq_levels),
                                                                  fsq_num_quantizers=1).eval()
    ref_sd = spk.state_dict()
    head = ("speaker_encoder.pool.", "speaker_encoder.bn.", "speaker_encoder.linear.", "quantizer.project_out.", "project.")
    want = {"speaker_encoder." + k for k in ref_sd if not k.startswith(head)}
    assert set(sd) == want, set(sd) ^ want  # every tensor get_global_tokens reads, and nothing else
    missing, unexpected = spk.load_state_dict({k[len("speaker_encoder."):]: v for k, v in sd.items()}, strict=False)
    assert not unexpected and all(k.startswith(head) for k in missing)
    wav = synth.synth_wav(6, 3, 24000)
    mel = T.mel_spectrogram(wav.double(), spec.mel_params).float()                 # [B, frames, mels]
    with torch.no_grad():
        tok_ref = spk.tokenize(mel)                                                # bicodec.py:177
    assert tok_ref.dtype == torch.int32 and tok_ref.shape == (3, 1, spec.token_num)
    taps = {}
    tok = T.fsq(sd, T.perceiver(sd, T.ecapa_latent(sd, mel, taps)), spec.fsq_levels, taps)
    assert torch.equal(tok, tok_ref[:, 0])
    lat64 = T.perceiver(T.cast(sd), T.ecapa_latent(T.cast(sd), mel.double()))
    assert float((T.fsq(T.cast(sd), lat64, spec.fsq_levels) == tok_ref[:, 0]).double().mean()) >= 0.95
    digits = torch.round(taps["fsq.bounded"]).reshape(-1, len(spec.fsq_levels))
    assert all(len(torch.unique(digits[:, d])) >= 3 for d in range(digits.shape[1]))  # seeded weights use the FSQ levels


def test_mel_matches_transformers_audio_utils():
    au = pytest.importorskip("transformers.audio_utils")
    mp = SPEC_BICODEC_ENCODER.mel_params
    fb = T.mel_filterbank(mp["n_fft"], mp["num_mels"], mp["sample_rate"], mp["mel_fmin"], mp["mel_fmax"])
    hz = au.mel_filter_bank(mp["n_fft"] // 2 + 1, mp["num_mels"], mp["mel_fmin"], mp["sample_rate"] / 2, mp["sample_rate"], norm="slaney",
                            mel_scale="slaney", triangularize_in_mel_space=False)
    assert np.abs(fb.numpy() - hz).max() < 1e-7 * np.abs(hz).max()  # torchaudio's triangles are in Hz between mel-spaced edges
    mel_space = au.mel_filter_bank(mp["n_fft"] // 2 + 1, mp["num_mels"], mp["mel_fmin"], mp["sample_rate"] / 2, mp["sample_rate"],
                                   norm="slaney", mel_scale="slaney", triangularize_in_mel_space=True)
    assert np.abs(fb.numpy() - mel_space).max() > 1e-3 * np.abs(hz).max()
    wav = synth.synth_wav(8, 2, 96000).double()
    got = T.mel_spectrogram(wav, mp)
    assert got.shape == (2, 301, 128)
    window = au.window_function(mp["win_length"], "hann", frame_length=mp["n_fft"], center=True, periodic=True)
    for b in range(2):
        want = au.spectrogram(wav[b].numpy(), window, frame_length=mp["n_fft"], hop_length=mp["hop_length"], power=1.0, center=True,
                              pad_mode="reflect", mel_filters=hz)
        assert np.abs(got[b].numpy().T - want).max() < 1e-6 * np.abs(want).max()  # transformers frames in float32


def test_ref_clip_matches_reference_rule():
    wav = torch.arange(1000, dtype=torch.float32).reshape(2, 500)
    short = T.ref_clip(wav, 1280)                                  # tiled: 500 -> 1500 -> 1280
    assert short.shape == (2, 1280) and torch.equal(short[:, 500:1000], wav) and torch.equal(short[:, 1000:], wav[:, :280])
    assert torch.equal(T.ref_clip(wav, 320), wav[:, :320])         # truncated
    assert SPEC_BICODEC_ENCODER.ref_segment_length(RC.SPARKTTS_CONFIG["ref_segment_duration"], RC.SPARKTTS_CONFIG["latent_hop_length"]) == 96000


def test_encoder_spec_global_fields_from_config_and_refusals():
    import unified_audio_amd as qa

    base = RC.BICODEC_CONFIG["audio_tokenizer"]
    s = BiCodecEncoderSpec.from_config(base)
    assert (s.n_fft, s.win_length, s.hop_length, s.mel_dim, s.mel_fmin, s.mel_fmax, s.token_num, s.fsq_levels) == (1024, 640, 320, 128, 10.0, 0.0,
                                                                                                                      32, (4,) * 6)
    for block, key, value, word in (("mel_params", "win_length", 1024, "win_length"), ("speaker_encoder", "fsq_num_quantizers", 2, "fsq_num_quantizers"),
                                    ("speaker_encoder", "fsq_levels", [1, 4], "fsq_levels")):
        c = copy.deepcopy(base)
        c[block][key] = value
        with pytest.raises(qa.QuarkAudioError, match=word):
            BiCodecEncoderSpec.from_config(c)
    c = copy.deepcopy(base)
    c["speaker_encoder"]["input_dim"] = 80
    with pytest.raises(ValueError, match="num_mels"):
        BiCodecEncoderSpec.from_config(c)
