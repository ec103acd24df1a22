"""Per-clip lengths of the SSL front-end, the parts that need no GPU.

(a) The semantics pin.  "Row b is the clip alone" is not an invention for the LayerNorm flavour (wav2vec 2.0 large / XLSR): transformers'
    own `attention_mask` path computes it.  A zero-padded batch whose mask covers pad + len_b + pad samples of row b gives, on row b's
    valid frames, every hidden state of the oracle (oracle/ssl_ref.hidden_states) on that clip alone.  Bound 1e-5 (max abs / max abs per
    hidden state): an order above the 6.8e-7 .. 9.6e-7 measured on CPU, four orders below what zero-padding WITHOUT a mask costs (0.085
    relative RMS for this flavour, 0.34 for the GroupNorm flavour, where transformers offers nothing and the clip alone is the definition).
(b) The drivers' host logic on stand-ins: a front-end whose __call__ takes `lengths` gets ONE call with the right vector; one without
    gets the loop over distinct lengths.
"""
import torch

from oracle import ssl_ref as S

SMALL = dict(conv_dim=(64,) * 7, hidden_size=128, num_hidden_layers=3, num_attention_heads=2, intermediate_size=256,
             num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=2, conv_bias=True, feat_extract_norm="layer",
             do_stable_layer_norm=True, select=(1, 3))


def _frames(spec, n):
    L = n + 2 * spec.pad
    for k, s in zip(spec.conv_kernel, spec.conv_stride):
        L = (L - k) // s + 1
    return L


def test_attention_mask_of_transformers_is_the_clip_alone_for_the_layer_norm_flavour():
    from transformers import Wav2Vec2Model

    spec = S.SSLSpec(**SMALL)
    sd = S.synth_state_dict(5, spec, "wav2vec2")
    model = Wav2Vec2Model(S.hf_config(spec, "wav2vec2")).eval()
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and all("masked_spec_embed" in m for m in missing), (missing, unexpected)
    lengths = [320 * 70 + 57, 320 * 34 - 57, 320 * 33 + 70]
    assert [_frames(spec, n) for n in lengths] == [70, 34, 33]
    g = torch.Generator().manual_seed(0)
    clips = [torch.randn(n, generator=g) * 0.3 for n in lengths]
    T = max(lengths) + 2 * spec.pad
    batch = torch.zeros(len(clips), T)
    mask = torch.zeros(len(clips), T, dtype=torch.long)
    for b, c in enumerate(clips):
        batch[b, spec.pad:spec.pad + len(c)] = c   # pad zeros, the clip, pad zeros, then the batch's own zero padding
        mask[b, :len(c) + 2 * spec.pad] = 1
    with torch.no_grad():
        hf = model(batch, attention_mask=mask, output_hidden_states=True).hidden_states
        padded = model(batch, output_hidden_states=True).hidden_states  # zero-padding without a mask: NOT the clip alone
        for b, c in enumerate(clips):
            alone = S.hidden_states(sd, torch.nn.functional.pad(c[None], (spec.pad, spec.pad)), spec)
            n = _frames(spec, len(c))
            assert len(alone) == len(hf) == spec.num_hidden_layers + 1
            for i, (a, h) in enumerate(zip(alone, hf)):
                assert a.shape[1] == n
                e = float((h[b, :n] - a[0]).abs().max() / a[0].abs().max())
                print(f"clip {b} hidden state {i}: {e:.2e}")
                assert e < 1e-5, (b, i, e)
            if b > 0:  # the shorter clips: the unmasked batch is far from them
                e = float((padded[-1][b, :n] - alone[-1][0]).abs().max() / alone[-1][0].abs().max())
                assert e > 1e-3, e


HOP = 320


class _NoLM:
    def generate(self, task_name, enroll_mel, enroll_feats, mix_mel, mix_feats, do_sample, enroll_lengths=None):
        raise AssertionError("not called")


def _front_end(log, ragged):
    """Frame t of a clip carries its sample 320 t; a clip of n samples has n // 320 frames."""

    def feats(wavs, n):
        return wavs[:, :n * HOP:HOP].unsqueeze(-1).repeat(1, 1, 4)

    class Plain:
        def __call__(self, wavs):
            log.append((tuple(wavs.shape), None))
            return feats(wavs, wavs.shape[1] // HOP)

    class Ragged:
        def frames(self, n):
            return n // HOP

        def __call__(self, wavs, lengths=None):
            log.append((tuple(wavs.shape), None if lengths is None else list(lengths)))
            out = feats(wavs, wavs.shape[1] // HOP)
            for b, n in enumerate(lengths or []):
                out[b, n // HOP:] = 0
            return out

    return Ragged() if ragged else Plain()


def test_unise_enrollments_take_one_call_where_the_front_end_has_lengths():
    from unified_audio_amd import unise as U

    enrs = [torch.full((1, n), float(i + 1)) for i, n in enumerate((32000, 48000, 32000, 80000))]
    log_r, log_p = [], []
    ragged, plain = U.UniSE(_NoLM(), _front_end(log_r, True)), U.UniSE(_NoLM(), _front_end(log_p, False))
    assert ragged._ssl_ragged_ok and not plain._ssl_ragged_ok
    ef, n_enr, frames = ragged._enroll_features(enrs)
    assert log_r == [((4, 80000), [32000, 48000, 32000, 80000])]
    ef2, n2, frames2 = plain._enroll_features(enrs)
    assert sorted(log_p) == [((1, 48000), None), ((1, 80000), None), ((2, 32000), None)]
    assert (n_enr, frames) == (n2, frames2) == (80000, [100, 150, 100, 250])
    assert torch.equal(ef, ef2) and ef.shape == (4, 250, 4)
    for i, n in enumerate(frames):
        assert (ef[i, :n] == float(i + 1)).all() and (ef[i, n:] == 0).all()
    # equal lengths: the plain call, no keyword
    log_r.clear()
    ragged._enroll_features(enrs[::2])
    assert log_r == [((2, 32000), None)]


def test_tokenizer_loop_stays_for_a_front_end_without_lengths():
    """HCodecTokenizer._ragged_front_end: only the library's own SSLFeatureExtractor, and only without resampling."""
    from unified_audio_amd.hcodec import HCodecTokenizer
    from unified_audio_amd.ssl import SSLFeatureExtractor

    class Tok:
        _ragged_front_end = HCodecTokenizer._ragged_front_end

    t = Tok()
    t.feature_extractor, t.sampling_rate = _front_end([], True), 16000
    assert not t._ragged_front_end()
    t.feature_extractor = SSLFeatureExtractor.__new__(SSLFeatureExtractor)
    assert t._ragged_front_end()
    t.sampling_rate = 48000
    assert not t._ragged_front_end()
