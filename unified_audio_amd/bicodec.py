"""Python mirror of the reference's BiCodec, backed by libquarkaudio_hip.so.

    BiCodec.detokenize           <->  QuarkAudio-UniSE/model/bicodec/bicodec.py:182-199
    BiCodecTokenizer.detokenize  <->  QuarkAudio-UniSE/model/bicodec/audio_tokenizer.py (called at model/model.py:193,223)
    wav_normalize                <->  the Wav2Vec2FeatureExtractor normalisation in front of XLSR-53 (audio_tokenizer.py:74-90)

The decode side is the UniSE inference path (the LM produces the tokens); `tokenize` builds the LM's training targets
(model/model.py:96-160) and turns a speaker prompt into its 32 global tokens.

    BiCodec.tokenize / get_semantic_tokens / get_global_tokens  <->  bicodec.py:151-180
    BiCodecTokenizer.tokenize                                    <->  audio_tokenizer.py:93-103
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Any, Dict, Mapping, Tuple

import torch

from . import _lib


@dataclass(frozen=True)
class BiCodecSpec:
    """`audio_tokenizer` section of the Spark-TTS BiCodec `config.yaml` the reference loads from `codec_ckpt_dir`
    (bicodec.py:80-87; the file itself is not in the reference tree)."""

    latent_dim: int = 1024
    codebook_size: int = 8192
    codebook_dim: int = 8
    mel_dim: int = 128  # encoder side only
    spk_latent_dim: int = 128
    token_num: int = 32
    fsq_levels: Tuple[int, ...] = (4, 4, 4, 4, 4, 4)
    vocos_dim: int = 384
    vocos_inter: int = 2048
    vocos_layers: int = 12
    gen_channels: int = 1536
    rates: Tuple[int, ...] = (8, 5, 4, 2)
    kernel_sizes: Tuple[int, ...] = (16, 11, 8, 4)

    @property
    def hop(self) -> int:
        h = 1
        for r in self.rates:
            h *= r
        return h

    @property
    def global_size(self) -> int:
        n = 1
        for lv in self.fsq_levels:
            n *= lv
        return n

    @classmethod
    def from_config(cls, audio_tokenizer: Mapping[str, Any]) -> "BiCodecSpec":
        """The `audio_tokenizer` section of `{model_dir}/config.yaml`, block by block as `BiCodec.load_from_checkpoint` hands it to its
        module constructors (bicodec.py:80-87): `quantizer` -> FactorizedVectorQuantize (factorized_vector_quantize.py:37-48),
        `speaker_encoder` -> SpeakerEncoder (speaker_encoder.py:48-56), `prenet` -> Decoder (feat_decoder.py:37-47), `decoder` ->
        WaveGenerator (wave_generator.py:60-67).  A missing required key is a TypeError and an unknown key in a block whose constructor
        takes no **kwargs is a TypeError, as in the reference; a value the detokenizer kernels have no path for is refused by name
        (QuarkAudioError -4) instead of being ignored.  `mel_params` and `encoder` configure the encoder side (tokenize) and are not
        read; the keys of `postnet` are checked as Decoder(**postnet) checks them (BiCodecForwardSpec.from_config), its values only
        when the forward head is built."""
        def block(name, required, optional=(), open_kwargs=False):
            if name not in audio_tokenizer:
                raise KeyError(f"config.yaml: audio_tokenizer.{name} is missing (bicodec.py:80-87 reads it)")
            b = dict(audio_tokenizer[name])
            missing = [k for k in required if k not in b]
            if missing:
                raise TypeError(f"audio_tokenizer.{name}: missing required argument(s) {missing}")
            unknown = [k for k in b if k not in required and k not in optional]
            if unknown and not open_kwargs:
                raise TypeError(f"audio_tokenizer.{name}: unexpected keyword argument(s) {unknown}")
            return b

        def refuse(what):
            raise _lib.QuarkAudioError(-4, f"BiCodec config.yaml: {what} - the MI355X detokenizer has no path for it")

        q = block("quantizer", ("input_dim", "codebook_size", "codebook_dim", "commitment"), open_kwargs=True)  # **kwargs: training-side keys pass
        spk = block("speaker_encoder", (), ("input_dim", "out_dim", "latent_dim", "token_num", "fsq_levels", "fsq_num_quantizers"))
        pre = block("prenet", ("input_channels", "vocos_dim", "vocos_intermediate_dim", "vocos_num_layers", "out_channels"),
                    ("condition_dim", "sample_ratios", "use_tanh_at_final"))
        dec = block("decoder", ("input_channel", "channels", "rates", "kernel_sizes"), ("d_out",))
        BiCodecForwardSpec.from_config(audio_tokenizer)
        latent = int(q["input_dim"])
        if int(q["codebook_dim"]) == latent:
            refuse("quantizer.input_dim == codebook_dim (Identity projections, factorized_vector_quantize.py:59-65)")
        spk_out = int(spk.get("out_dim", 512))
        if int(spk.get("fsq_num_quantizers", 1)) != 1:
            refuse(f"speaker_encoder.fsq_num_quantizers = {spk['fsq_num_quantizers']} (one FSQ stage is built)")
        levels = tuple(int(v) for v in spk.get("fsq_levels", (4, 4, 4, 4, 4, 4)))
        if not 1 <= len(levels) <= 8:
            refuse(f"speaker_encoder.fsq_levels with {len(levels)} entries (1 .. 8)")
        if [int(r) for r in pre.get("sample_ratios", (1, 1))] != [1, 1]:
            refuse(f"prenet.sample_ratios = {list(pre['sample_ratios'])} (the two ratio-1 SamplingBlocks of the published model are built)")
        if bool(pre.get("use_tanh_at_final", False)):
            refuse("prenet.use_tanh_at_final = true")
        if int(dec.get("d_out", 1)) != 1:
            refuse(f"decoder.d_out = {dec['d_out']} (mono)")
        rates, ks = tuple(int(v) for v in dec["rates"]), tuple(int(v) for v in dec["kernel_sizes"])
        if len(rates) != len(ks) or not 1 <= len(rates) <= 8:
            refuse(f"decoder.rates / kernel_sizes of lengths {len(rates)} / {len(ks)} (equal, 1 .. 8)")
        # the tensors that meet in detokenize (bicodec.py:193-199): z_q [latent] -> prenet -> + d_vector [spk_out] -> decoder
        widths = {"quantizer.input_dim": latent, "prenet.input_channels": int(pre["input_channels"]), "prenet.out_channels": int(pre["out_channels"]),
                  "prenet.condition_dim": int(pre["condition_dim"]) if pre.get("condition_dim") is not None else None,
                  "speaker_encoder.out_dim": spk_out, "decoder.input_channel": int(dec["input_channel"])}
        if widths["prenet.condition_dim"] is None:
            refuse("prenet.condition_dim = null (detokenize conditions the prenet on the d-vector)")
        if len(set(widths.values())) != 1:
            raise ValueError(f"BiCodec config.yaml: widths that must agree in detokenize differ: {widths}")
        mel = audio_tokenizer.get("mel_params") or {}
        return cls(latent_dim=latent, codebook_size=int(q["codebook_size"]), codebook_dim=int(q["codebook_dim"]),
                   mel_dim=int(spk.get("input_dim", mel.get("num_mels", 100))), spk_latent_dim=int(spk.get("latent_dim", 128)),
                   token_num=int(spk.get("token_num", 32)), fsq_levels=levels, vocos_dim=int(pre["vocos_dim"]),
                   vocos_inter=int(pre["vocos_intermediate_dim"]), vocos_layers=int(pre["vocos_num_layers"]),
                   gen_channels=int(dec["channels"]), rates=rates, kernel_sizes=ks)

    def to_c(self) -> "_lib.qa_bicodec_spec":
        s = _lib.qa_bicodec_spec()
        s.latent_dim, s.codebook_size, s.codebook_dim = self.latent_dim, self.codebook_size, self.codebook_dim
        s.spk_latent_dim, s.token_num, s.n_levels = self.spk_latent_dim, self.token_num, len(self.fsq_levels)
        for i, v in enumerate(self.fsq_levels):
            s.levels[i] = v
        s.vocos_dim, s.vocos_inter, s.vocos_layers = self.vocos_dim, self.vocos_inter, self.vocos_layers
        s.gen_channels, s.n_rates = self.gen_channels, len(self.rates)
        for i, (r, k) in enumerate(zip(self.rates, self.kernel_sizes)):
            s.rates[i], s.kernel_sizes[i] = r, k
        return s


SPEC_BICODEC = BiCodecSpec()


@dataclass(frozen=True)
class BiCodecEncoderSpec:
    """The `encoder`, `quantizer`, `mel_params` and `speaker_encoder` blocks of the BiCodec `config.yaml` as `BiCodec.tokenize` uses them
    (Encoder, feat_encoder.py:29-92; FactorizedVectorQuantize.tokenize, factorized_vector_quantize.py:148-152,169-187; MelSpectrogram,
    bicodec.py:201-221; SpeakerEncoder.tokenize, speaker_encoder.py)."""

    input_channels: int = 1024  # XLSR-53 hidden width
    vocos_dim: int = 384
    vocos_inter: int = 2048
    vocos_layers: int = 12
    latent_dim: int = 1024      # encoder.out_channels = quantizer.input_dim
    codebook_size: int = 8192
    codebook_dim: int = 8
    # global tokens: mel_params (bicodec.py:201-221), speaker_encoder (speaker_encoder.py:33-60; ECAPA width and perceiver shape are
    # fixed there: ECAPA_TDNN_GLOB_c512, PerceiverResampler defaults)
    sample_rate: int = 16000
    n_fft: int = 1024
    win_length: int = 640
    hop_length: int = 320
    mel_fmin: float = 10.0
    mel_fmax: float = 0.0       # 0: sample_rate / 2 (mel_fmax: null)
    mel_dim: int = 128          # mel_params.num_mels = speaker_encoder.input_dim
    ecapa_channels: int = 512
    spk_latent_dim: int = 128
    token_num: int = 32
    fsq_levels: Tuple[int, ...] = (4, 4, 4, 4, 4, 4)
    perceiver_depth: int = 2
    perceiver_heads: int = 8
    perceiver_dim_head: int = 64

    @property
    def mel_params(self) -> Dict[str, Any]:
        return dict(sample_rate=self.sample_rate, n_fft=self.n_fft, win_length=self.win_length, hop_length=self.hop_length,
                    mel_fmin=self.mel_fmin, mel_fmax=self.mel_fmax or None, num_mels=self.mel_dim)

    @classmethod
    def from_spec(cls, spec: BiCodecSpec, input_channels: int = 1024) -> "BiCodecEncoderSpec":
        """The published model's encoder shares its widths with the prenet, the quantizer and the speaker encoder of `spec`."""
        return cls(input_channels=input_channels, vocos_dim=spec.vocos_dim, vocos_inter=spec.vocos_inter, vocos_layers=spec.vocos_layers,
                   latent_dim=spec.latent_dim, codebook_size=spec.codebook_size, codebook_dim=spec.codebook_dim, mel_dim=spec.mel_dim,
                   spk_latent_dim=spec.spk_latent_dim, token_num=spec.token_num, fsq_levels=spec.fsq_levels)

    def ref_segment_length(self, ref_segment_duration: float = 6, latent_hop_length: int = 320) -> int:
        """BiCodecTokenizer.get_ref_clip's clip length (audio_tokenizer.py:60-64): 96 000 samples for the published configuration."""
        return int(self.sample_rate * ref_segment_duration) // latent_hop_length * latent_hop_length

    @classmethod
    def from_config(cls, audio_tokenizer: Mapping[str, Any]) -> "BiCodecEncoderSpec":
        """The `audio_tokenizer` section of `{model_dir}/config.yaml`: `encoder` -> Encoder(**encoder), `quantizer` ->
        FactorizedVectorQuantize(**quantizer), `mel_params` -> MelSpectrogram, `speaker_encoder` -> SpeakerEncoder (bicodec.py:62-87).
        A value the kernels have no path for is refused by name (QuarkAudioError -4)."""
        def refuse(what):
            raise _lib.QuarkAudioError(-4, f"BiCodec config.yaml: {what} - the MI355X tokenizer has no path for it")

        for name in ("encoder", "quantizer"):
            if name not in audio_tokenizer:
                raise KeyError(f"config.yaml: audio_tokenizer.{name} is missing (bicodec.py:80-87 reads it)")
        enc, q = dict(audio_tokenizer["encoder"]), dict(audio_tokenizer["quantizer"])
        required = ("input_channels", "vocos_dim", "vocos_intermediate_dim", "vocos_num_layers", "out_channels")
        missing = [k for k in required if k not in enc]
        if missing:
            raise TypeError(f"audio_tokenizer.encoder: missing required argument(s) {missing}")
        unknown = [k for k in enc if k not in required and k != "sample_ratios"]
        if unknown:
            raise TypeError(f"audio_tokenizer.encoder: unexpected keyword argument(s) {unknown}")
        missing = [k for k in ("input_dim", "codebook_size", "codebook_dim") if k not in q]
        if missing:
            raise TypeError(f"audio_tokenizer.quantizer: missing required argument(s) {missing}")
        if [int(r) for r in enc.get("sample_ratios", (1, 1))] != [1, 1]:
            refuse(f"encoder.sample_ratios = {list(enc['sample_ratios'])} (the two ratio-1 SamplingBlocks of the published model are built)")
        if int(q["codebook_dim"]) == int(q["input_dim"]):
            refuse("quantizer.input_dim == codebook_dim (Identity projections, factorized_vector_quantize.py:59-65)")
        if int(enc["out_channels"]) != int(q["input_dim"]):
            raise ValueError(f"BiCodec config.yaml: encoder.out_channels = {enc['out_channels']} and quantizer.input_dim = {q['input_dim']} "
                             "must agree (get_semantic_tokens feeds one into the other)")
        mel = dict(audio_tokenizer.get("mel_params") or {})
        spk = dict(audio_tokenizer.get("speaker_encoder") or {})
        d = cls()
        mkw = dict(sample_rate=int(mel.get("sample_rate", d.sample_rate)), n_fft=int(mel.get("n_fft", d.n_fft)),
                   win_length=int(mel.get("win_length", d.win_length)), hop_length=int(mel.get("hop_length", d.hop_length)),
                   mel_fmin=float(mel.get("mel_fmin", d.mel_fmin)), mel_fmax=float(mel.get("mel_fmax") or 0.0),
                   mel_dim=int(mel.get("num_mels", d.mel_dim)))
        if mkw["win_length"] != 2 * mkw["hop_length"] or mkw["hop_length"] % 32 or mkw["n_fft"] < mkw["win_length"] or (mkw["n_fft"] - mkw["win_length"]) % 2:
            refuse(f"mel_params.win_length = {mkw['win_length']}, hop_length = {mkw['hop_length']}, n_fft = {mkw['n_fft']} (the mel front "
                   "frames the signal as 2 hops of a multiple of 32 samples)")
        if int(spk.get("fsq_num_quantizers", 1)) != 1:
            refuse(f"speaker_encoder.fsq_num_quantizers = {spk['fsq_num_quantizers']} (one FSQ stage is built)")
        BiCodecForwardSpec.from_config(audio_tokenizer)  # the postnet's keys; its values matter only to forward
        if int(spk.get("input_dim", mkw["mel_dim"])) != mkw["mel_dim"]:
            raise ValueError(f"BiCodec config.yaml: speaker_encoder.input_dim = {spk['input_dim']} and mel_params.num_mels = "
                             f"{mkw['mel_dim']} must agree (get_global_tokens feeds one into the other)")
        levels = tuple(int(v) for v in spk.get("fsq_levels", d.fsq_levels))
        if not 1 <= len(levels) <= 8 or min(levels) < 2:
            refuse(f"speaker_encoder.fsq_levels = {list(levels)} (1 .. 8 levels of at least 2)")
        return cls(input_channels=int(enc["input_channels"]), vocos_dim=int(enc["vocos_dim"]), vocos_inter=int(enc["vocos_intermediate_dim"]),
                   vocos_layers=int(enc["vocos_num_layers"]), latent_dim=int(enc["out_channels"]), codebook_size=int(q["codebook_size"]),
                   codebook_dim=int(q["codebook_dim"]), spk_latent_dim=int(spk.get("latent_dim", d.spk_latent_dim)),
                   token_num=int(spk.get("token_num", d.token_num)), fsq_levels=levels, **mkw)

    def to_c(self) -> "_lib.qa_bicodec_enc_spec":
        s = _lib.qa_bicodec_enc_spec()
        s.input_channels, s.vocos_dim, s.vocos_inter, s.vocos_layers = self.input_channels, self.vocos_dim, self.vocos_inter, self.vocos_layers
        s.latent_dim, s.codebook_size, s.codebook_dim = self.latent_dim, self.codebook_size, self.codebook_dim
        s.sample_rate, s.n_fft, s.win_length, s.hop_length = self.sample_rate, self.n_fft, self.win_length, self.hop_length
        s.mel_fmin, s.mel_fmax, s.mel_dim, s.ecapa_channels = self.mel_fmin, self.mel_fmax, self.mel_dim, self.ecapa_channels
        s.spk_latent_dim, s.token_num, s.n_levels = self.spk_latent_dim, self.token_num, len(self.fsq_levels)
        for i, v in enumerate(self.fsq_levels):
            s.levels[i] = v
        s.perceiver_depth, s.perceiver_heads, s.perceiver_dim_head = self.perceiver_depth, self.perceiver_heads, self.perceiver_dim_head
        return s


SPEC_BICODEC_ENCODER = BiCodecEncoderSpec()

POSTNET_REQUIRED = ("input_channels", "vocos_dim", "vocos_intermediate_dim", "vocos_num_layers", "out_channels")
POSTNET_OPTIONAL = ("condition_dim", "sample_ratios", "use_tanh_at_final")


@dataclass(frozen=True)
class BiCodecForwardSpec:
    """What `BiCodec.forward` needs beyond tokenize and detokenize (bicodec.py:113-149): the `postnet` block of the `config.yaml`
    (feat_decoder.Decoder, feat_decoder.py:37-47, called without a condition) and `speaker_encoder.out_dim`, the width of the x-vector
    (ECAPA_TDNN's Linear(3072 -> out_dim), ecapa_tdnn.py:188).  The published values are the defaults."""

    input_channels: int = 1024  # = latent_dim: the postnet reads the prenet output
    vocos_dim: int = 384
    vocos_inter: int = 2048
    vocos_layers: int = 6
    out_channels: int = 1024    # the XLSR-53 feature width pred_feat predicts
    use_tanh_at_final: bool = False
    sample_ratios: Tuple[int, ...] = (1, 1)
    condition_dim: Any = None
    xvector_dim: int = 1024     # speaker_encoder.out_dim

    @classmethod
    def from_spec(cls, spec: BiCodecSpec, encoder_spec: BiCodecEncoderSpec) -> "BiCodecForwardSpec":
        """The published postnet (6 ConvNeXt layers at the prenet's widths, latent -> XLSR-53 width) of a model of `spec`."""
        return cls(input_channels=spec.latent_dim, vocos_dim=spec.vocos_dim, vocos_inter=spec.vocos_inter,
                   out_channels=encoder_spec.input_channels, xvector_dim=spec.latent_dim)

    @classmethod
    def from_config(cls, audio_tokenizer: Mapping[str, Any]) -> "BiCodecForwardSpec | None":
        """The `postnet` block as `Decoder(**config["postnet"])` takes it (bicodec.py:86) and `speaker_encoder.out_dim`; None without a
        `postnet` block.  A missing required key or an unknown key is a TypeError, as in the reference.  A value the forward kernels have
        no path for is NOT refused here (tokenize and detokenize never read the postnet): `unsupported()` names it, and forward refuses."""
        if "postnet" not in audio_tokenizer:
            return None
        b = dict(audio_tokenizer["postnet"])
        missing = [k for k in POSTNET_REQUIRED if k not in b]
        if missing:
            raise TypeError(f"audio_tokenizer.postnet: missing required argument(s) {missing}")
        unknown = [k for k in b if k not in POSTNET_REQUIRED and k not in POSTNET_OPTIONAL]
        if unknown:
            raise TypeError(f"audio_tokenizer.postnet: unexpected keyword argument(s) {unknown}")
        spk = dict(audio_tokenizer.get("speaker_encoder") or {})
        return cls(input_channels=int(b["input_channels"]), vocos_dim=int(b["vocos_dim"]), vocos_inter=int(b["vocos_intermediate_dim"]),
                   vocos_layers=int(b["vocos_num_layers"]), out_channels=int(b["out_channels"]),
                   use_tanh_at_final=bool(b.get("use_tanh_at_final", False)),
                   sample_ratios=tuple(int(r) for r in b.get("sample_ratios", (1, 1))), condition_dim=b.get("condition_dim"),
                   xvector_dim=int(spk.get("out_dim", 512)))

    def unsupported(self, latent_dim: int) -> "str | None":
        """Why the forward kernels cannot run this postnet, or None."""
        if list(self.sample_ratios) != [1, 1]:
            return f"postnet.sample_ratios = {list(self.sample_ratios)} (the two ratio-1 SamplingBlocks of the published model are built)"
        if self.condition_dim is not None:
            return f"postnet.condition_dim = {self.condition_dim} (BiCodec.forward calls the postnet without a condition, bicodec.py:135)"
        if self.input_channels != latent_dim:
            return f"postnet.input_channels = {self.input_channels} (it reads the prenet output of width {latent_dim})"
        for name, v in (("postnet.vocos_dim", self.vocos_dim), ("postnet.vocos_intermediate_dim", self.vocos_inter),
                        ("postnet.out_channels", self.out_channels), ("speaker_encoder.out_dim", self.xvector_dim)):
            if v <= 0 or v % 32:
                return f"{name} = {v} (a positive multiple of 32)"
        if self.vocos_layers < 1:
            return f"postnet.vocos_num_layers = {self.vocos_layers}"
        return None

    def to_c(self) -> "_lib.qa_bicodec_forward_spec":
        s = _lib.qa_bicodec_forward_spec()
        s.postnet_input_channels, s.postnet_vocos_dim, s.postnet_vocos_inter = self.input_channels, self.vocos_dim, self.vocos_inter
        s.postnet_vocos_layers, s.postnet_out_channels = self.vocos_layers, self.out_channels
        s.postnet_tanh, s.xvector_dim = int(self.use_tanh_at_final), self.xvector_dim
        return s
# the entry whose presence makes load_state_dict build the tokenizer (then every encoder.*, quantizer.in_project.*, speaker_encoder.*
# tensor it reads must be there); stray encoder-side entries without it are ignored, as they always were
ENCODER_KEY = "encoder.encoder.embed.weight"


def clip_lengths(lengths, B: int, lo: int, hi: int, what: str, hi_name: str = "T"):
    """The length vector of a per-clip call as a host int64 array: B entries (list / tuple / tensor), each in
    lo .. hi.  Checked here, before anything is launched, in the words of the library's own check (QuarkAudioError -1 names the row and
    its value); the C entry points check again for callers of the C-ABI."""
    lens = [int(v) for v in (lengths.tolist() if torch.is_tensor(lengths) else lengths)]
    if len(lens) != B:
        raise _lib.QuarkAudioError(-1, f"{what}: lengths has {len(lens)} entries for a batch of B = {B}")
    for b, v in enumerate(lens):
        if not lo <= v <= hi:
            raise _lib.QuarkAudioError(-1, f"{what}: lengths[{b}] = {v} is outside {lo} .. {hi_name} = {hi}")
    return lens, (C.c_int64 * B)(*lens)


@torch.no_grad()
def wav_normalize(wav: torch.Tensor, eps: float = 1e-7, lengths=None) -> torch.Tensor:
    """Wav2Vec2FeatureExtractor(do_normalize=True) on equal-length rows (audio_tokenizer.py:74-90, padding=True pads nothing):
    wav [B, T] (or [T]) on the GPU -> (wav - mean) / sqrt(var + eps) per row, fp32, on the same device.

    lengths: the rows' lengths in SAMPLES (host list / tensor, B entries, 1 .. T).  Row b is then normalised
    over its own lengths[b] samples, exactly as the clip alone would be, and is exactly 0 behind them; what wav holds there is never
    read.  None: every row has T samples."""
    if wav.dim() not in (1, 2) or wav.shape[-1] == 0:
        raise _lib.QuarkAudioError(-1, f"wav must be [B, T] or [T] with T > 0, got {tuple(wav.shape)}")
    if wav.device.type != "cuda":
        raise _lib.QuarkAudioError(-1, "wav_normalize runs on the GPU: move wav to a HIP device first")
    x = wav.to(torch.float32).contiguous()
    B, T = (1, x.shape[0]) if x.dim() == 1 else x.shape
    arr = None if lengths is None else clip_lengths(lengths, B, 1, T, "wav_normalize")[1]
    out = torch.empty_like(x)
    stream = torch.cuda.current_stream(x.device).cuda_stream
    lib = _lib.load_library()
    if arr is None:
        _lib.check(lib.qa_wav_normalize(x.data_ptr(), B, T, out.data_ptr(), float(eps), stream))
    else:
        _lib.check(lib.qa_wav_normalize_ragged(x.data_ptr(), B, T, arr, out.data_ptr(), float(eps), stream))
    return out


def load_config(config_path) -> Dict[str, Any]:
    """utils/file.py:116-130 (`OmegaConf.load` + the optional `base_config` merge) with PyYAML: omegaconf is not a dependency here.  A
    value that uses OmegaConf interpolation (`${...}`) cannot be resolved by a plain YAML reader and is refused rather than passed on."""
    import yaml

    def read(path):
        with open(path, "r") as f:
            cfg = yaml.safe_load(f) or {}
        if not isinstance(cfg, dict):
            raise ValueError(f"{path}: a mapping is expected at the top level")
        return cfg

    def merge(base, over):  # OmegaConf.merge: mappings merge key by key, everything else is replaced
        out = dict(base)
        for k, v in over.items():
            out[k] = merge(out[k], v) if isinstance(v, dict) and isinstance(out.get(k), dict) else v
        return out

    def check(node, where):
        if isinstance(node, dict):
            for k, v in node.items():
                check(v, f"{where}.{k}")
        elif isinstance(node, (list, tuple)):
            for i, v in enumerate(node):
                check(v, f"{where}[{i}]")
        elif isinstance(node, str) and "${" in node:
            raise _lib.QuarkAudioError(-4, f"{config_path}: {where} = {node!r} uses OmegaConf interpolation, which this loader does not resolve")

    cfg = read(config_path)
    if cfg.get("base_config") is not None:
        cfg = merge(read(cfg["base_config"]), cfg)
    check(cfg, "config")
    return cfg


class BiCodec(torch.nn.Module):
    """`detokenize(semantic_tokens, global_tokens)` and `tokenize(batch)` / `get_semantic_tokens` / `get_global_tokens` of the reference's
    BiCodec.  Weights in the reference's key layout (`BiCodec.state_dict()` / the `model.safetensors` of the checkpoint).  The tokenizer
    is built when the state dict holds encoder.encoder.embed.weight (then it needs encoder.*, quantizer.in_project.* and the
    speaker_encoder's ECAPA / perceiver / project_in entries); a detokenize-only state dict loads as before.  `forward(batch)` (bicodec.py:
    113-149) additionally needs the x-vector head (speaker_encoder.speaker_encoder.{pool, bn, linear}.*) and postnet.*: they are
    attached when the tokenizer is built and they are present; without them everything else loads and runs as before and only forward
    refuses, naming the first missing or mis-shaped key."""

    def __init__(self, spec: BiCodecSpec = SPEC_BICODEC, *, device: str | torch.device = "cuda:0", check_tokens: bool = True,
                 encoder_spec: BiCodecEncoderSpec | None = None, forward_spec: BiCodecForwardSpec | None = None):
        super().__init__()
        self.spec = spec
        self.encoder_spec = encoder_spec or BiCodecEncoderSpec.from_spec(spec)
        self.forward_spec = forward_spec or BiCodecForwardSpec.from_spec(spec, self.encoder_spec)
        self.device = torch.device(device)
        self.check_tokens = check_tokens
        self._lib = _lib.load_library()
        self._handle = C.c_void_p()
        self._enc = C.c_void_p()
        self._forward_error = None  # (status, message): why forward cannot run

    @classmethod
    def load_from_checkpoint(cls, model_dir, device="cuda:0", spec: BiCodecSpec | None = None, **kwargs) -> "BiCodec":
        """bicodec.py:69-115: the architecture from `{model_dir}/config.yaml['audio_tokenizer']` (BiCodecSpec.from_config), the weights
        from `{model_dir}/model.safetensors`; missing detokenizer tensors are reported by name by qa_bicodec_create (the reference prints
        them and goes on with random weights, bicodec.py:103-108).  `spec=` overrides the file (a directory without config.yaml)."""
        from safetensors.torch import load_file

        sd = load_file(f"{model_dir}/model.safetensors")
        encoder_spec = forward_spec = None
        if spec is None:
            cfg = load_config(f"{model_dir}/config.yaml")["audio_tokenizer"]
            spec = BiCodecSpec.from_config(cfg)
            if ENCODER_KEY in sd:  # the tokenizer's config blocks are read only when the tokenizer is built
                encoder_spec = BiCodecEncoderSpec.from_config(cfg)
                forward_spec = BiCodecForwardSpec.from_config(cfg)
        return cls(spec, device=device, encoder_spec=encoder_spec, forward_spec=forward_spec).load_state_dict(sd)

    def load_state_dict(self, state_dict: Dict[str, torch.Tensor], strict: bool = False, assign: bool = False):
        _lib.require_device()
        self._free()
        table, n, keep = _lib.tensor_table(state_dict)
        handle = C.c_void_p()
        cspec = self.spec.to_c()
        _lib.check(self._lib.qa_bicodec_create(C.byref(handle), C.byref(cspec), table, n, self.device.index or 0))
        self._handle = handle
        if ENCODER_KEY in state_dict:  # the tokenizer: a missing tensor is named by the library
            enc = C.c_void_p()
            espec = self.encoder_spec.to_c()
            _lib.check(self._lib.qa_bicodec_enc_create(C.byref(enc), C.byref(espec), table, n, self.device.index or 0))
            self._enc = enc
            # the forward head is optional: nothing else reads it, and a state dict without (all of) it still loads
            why = self.forward_spec.unsupported(self.spec.latent_dim)
            if why is not None:
                self._forward_error = (-4, f"BiCodec config.yaml: {why} - the MI355X forward has no path for it")
            else:
                fspec = self.forward_spec.to_c()
                st = self._lib.qa_bicodec_load_forward(self._handle, self._enc, C.byref(fspec), table, n)
                self._forward_error = None if st == 0 else (st, self._lib.qa_last_error().decode("utf-8", "replace"))
        else:
            self._forward_error = (-3, f"BiCodec has no tokenizer: the state dict held no {ENCODER_KEY} (a detokenize-only checkpoint)")
        del keep
        return self

    @property
    def has_forward(self) -> bool:
        return bool(self._handle.value and self._enc.value) and self._lib.qa_bicodec_has_forward(self._handle, self._enc) == 1

    @torch.no_grad()
    def forward(self, batch: Mapping[str, torch.Tensor]) -> Dict[str, Any]:
        """BiCodec.forward in eval mode (bicodec.py:113-149) -> the reference's dict: vq_loss (0-dim NaN: the mean of the two empty eval
        losses, factorized_vector_quantize.py:121-131), perplexity and cluster_size (0-dim fp32, the code statistics over all B * N
        semantic tokens of the batch), recons [B, 1, N * hop] (= detokenize(*tokenize(batch)) bit for bit), pred_feat [B, out_channels, N]
        (the postnet on the prenet output before the d-vector add), x_vector / d_vector [B, out_dim], audios = batch["wav"].unsqueeze(1)
        and with_speaker_loss = False.  batch: "feat" [B, N, input_channels], "ref_wav" [B, T] (the whole rows, as get_global_tokens with
        ref_len = 0; the mel is the library's, not torchaudio's), "wav"."""
        if not self._handle.value:
            raise _lib.QuarkAudioError(-3, "BiCodec has no weights: call load_state_dict first")
        feat, ref, wav = batch["feat"], batch["ref_wav"], batch["wav"]
        self._require_tokenizer()
        if self._forward_error is not None:
            st, msg = self._forward_error
            raise _lib.QuarkAudioError(st, f"BiCodec.forward needs the x-vector head and postnet weights: {msg}")
        if feat.dim() != 3 or feat.shape[2] != self.encoder_spec.input_channels or feat.shape[1] == 0:
            raise _lib.QuarkAudioError(-1, f"feat must be [B, N, {self.encoder_spec.input_channels}] with N > 0, got {tuple(feat.shape)}")
        if ref.dim() != 2 or ref.shape[0] != feat.shape[0] or ref.shape[1] == 0:
            raise _lib.QuarkAudioError(-1, f"ref_wav must be [B, T] with B = {feat.shape[0]}, got {tuple(ref.shape)}")
        feat = feat.to(device=self.device, dtype=torch.float32).contiguous()
        ref = ref.to(device=self.device, dtype=torch.float32).contiguous()
        B, N, _ = feat.shape
        fs, dev = self.forward_spec, self.device
        sem = torch.empty((B, N), dtype=torch.int64, device=dev)
        glob = torch.empty((B, self.spec.token_num), dtype=torch.int64, device=dev)
        recons = torch.empty((B, 1, N * self.spec.hop), dtype=torch.float32, device=dev)
        pred = torch.empty((B, fs.out_channels, N), dtype=torch.float32, device=dev)
        x_vector = torch.empty((B, fs.xvector_dim), dtype=torch.float32, device=dev)
        d_vector = torch.empty((B, self.spec.latent_dim), dtype=torch.float32, device=dev)
        stats = torch.empty(2, dtype=torch.float32, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(self._lib.qa_bicodec_forward(self._handle, self._enc, feat.data_ptr(), B, N, ref.data_ptr(), ref.shape[1], sem.data_ptr(),
                                                glob.data_ptr(), recons.data_ptr(), pred.data_ptr(), x_vector.data_ptr(), d_vector.data_ptr(),
                                                stats[0:1].data_ptr(), stats[1:2].data_ptr(), stream))
        return {"vq_loss": torch.full((), float("nan"), dtype=torch.float32, device=dev), "perplexity": stats[0], "cluster_size": stats[1],
                "recons": recons, "pred_feat": pred, "x_vector": x_vector, "d_vector": d_vector,
                "audios": wav.to(dev).unsqueeze(1), "with_speaker_loss": False}

    def train(self, mode: bool = True):
        if mode:
            raise _lib.QuarkAudioError(-4, "unified_audio_amd.BiCodec is the inference path")
        return super().train(False)

    def remove_weight_norm(self):  # bicodec.py:113: weight norm is folded when the weights are loaded
        return self

    @torch.no_grad()
    def detokenize(self, semantic_tokens: torch.Tensor, global_tokens: torch.Tensor, lengths=None) -> torch.Tensor:
        """semantic_tokens [B, T] int64, global_tokens [B, 1, token_num] (or [B, token_num]) int64 -> wav [B, 1, T * hop] float32.

        lengths: the clips' lengths in TOKENS (host list / tensor, B entries, 1 .. T).  Row b is then the
        waveform of semantic_tokens[b, :lengths[b]] alone in its first lengths[b] * hop samples and exactly 0 behind them; entries at
        or behind lengths[b] are ignored, whatever they hold (-1 included), and the range check masks them.  None: the rectangular
        call."""
        if not self._handle.value:
            raise _lib.QuarkAudioError(-3, "BiCodec has no weights: call load_state_dict first")
        sem = semantic_tokens.to(device=self.device, dtype=torch.int64).contiguous()
        glob = global_tokens.to(device=self.device, dtype=torch.int64).contiguous()
        if sem.dim() != 2:
            raise _lib.QuarkAudioError(-1, f"semantic_tokens must be [B, T], got {tuple(sem.shape)}")
        B, T = sem.shape
        glob = glob.reshape(B, -1)
        if glob.shape[1] != self.spec.token_num:
            raise _lib.QuarkAudioError(-1, f"global_tokens must hold {self.spec.token_num} tokens per item, got {tuple(global_tokens.shape)}")
        lens = arr = None
        if lengths is not None:  # checked before anything is launched
            lens, arr = clip_lengths(lengths, B, 1, T, "BiCodec.detokenize")
        stream = torch.cuda.current_stream(self.device).cuda_stream
        if self.check_tokens:  # F.embedding / the implicit FSQ codebook gather would refuse out-of-range ids: ONE check (one host
            # sync) for both tensors - the global ids are scaled onto the semantic range so that a single limit serves
            lim_s, lim_g = self.spec.codebook_size, self.spec.global_size
            live = sem
            if lens is not None:  # entries behind a clip's end count as valid, as Codec.decode(lengths=...) masks them
                keep = torch.arange(T, device=self.device).unsqueeze(0) < torch.tensor(lens, device=self.device).unsqueeze(1)
                live = torch.where(keep, sem, 0)
            both = torch.cat([live.reshape(-1), torch.where((glob >= 0) & (glob < lim_g), 0, lim_s).reshape(-1)])
            bad = C.c_int64(0)
            _lib.check(self._lib.qa_codes_check(both.data_ptr(), both.numel(), lim_s, C.byref(bad), stream))
            if bad.value:
                n_g = int(((glob < 0) | (glob >= lim_g)).sum())
                raise IndexError(f"{bad.value - n_g} semantic_tokens out of range [0, {lim_s}), {n_g} global_tokens out of range [0, {lim_g})")
        wav = torch.empty((B, 1, T * self.spec.hop), dtype=torch.float32, device=self.device)
        if arr is None:
            _lib.check(self._lib.qa_bicodec_detokenize(self._handle, sem.data_ptr(), glob.data_ptr(), B, T, wav.data_ptr(), stream))
        else:
            _lib.check(self._lib.qa_bicodec_detokenize_ragged(self._handle, sem.data_ptr(), glob.data_ptr(), B, T, arr, wav.data_ptr(), stream))
        return wav

    @property
    def has_tokenizer(self) -> bool:
        return bool(self._enc.value)

    def _require_tokenizer(self):
        if not self._enc.value:
            raise _lib.QuarkAudioError(-3, f"BiCodec has no tokenizer: the state dict held no {ENCODER_KEY} (a detokenize-only checkpoint); "
                                           "tokenize needs the encoder.*, quantizer.in_project.* and speaker_encoder.* weights")

    def _feat(self, batch):
        self._require_tokenizer()
        feat = batch["feat"]
        if feat.dim() != 3 or feat.shape[2] != self.encoder_spec.input_channels or feat.shape[1] == 0:
            raise _lib.QuarkAudioError(-1, f"feat must be [B, N, {self.encoder_spec.input_channels}] with N > 0, got {tuple(feat.shape)}")
        return feat.to(device=self.device, dtype=torch.float32).contiguous()

    def _ref_wav(self, batch):
        self._require_tokenizer()
        wav = batch["ref_wav"]
        if wav.dim() != 2 or wav.shape[1] == 0:
            raise _lib.QuarkAudioError(-1, f"ref_wav must be [B, T], got {tuple(wav.shape)}")
        return wav.to(device=self.device, dtype=torch.float32).contiguous()

    @torch.no_grad()
    def get_semantic_tokens(self, batch: Mapping[str, torch.Tensor], lengths=None) -> torch.Tensor:
        """bicodec.py:167-172: batch["feat"] [B, N, input_channels] (the XLSR-53 hidden-state mix) -> semantic tokens int64 [B, N].

        lengths: the clips' lengths in FEATURE FRAMES (host list / tensor, B entries, 1 .. N).  Row b then holds
        the tokens of feat[b, :lengths[b]] alone and -1 behind them; rows of feat behind a clip's end are never read."""
        feat = self._feat(batch)
        B, N, _ = feat.shape
        arr = None if lengths is None else clip_lengths(lengths, B, 1, N, "BiCodec.get_semantic_tokens", "N")[1]
        out = torch.empty((B, N), dtype=torch.int64, device=self.device)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        if arr is None:
            _lib.check(self._lib.qa_bicodec_get_semantic_tokens(self._enc, feat.data_ptr(), B, N, out.data_ptr(), stream))
        else:
            _lib.check(self._lib.qa_bicodec_get_semantic_tokens_ragged(self._enc, feat.data_ptr(), B, N, arr, out.data_ptr(), stream))
        return out

    @torch.no_grad()
    def get_global_tokens(self, batch: Mapping[str, torch.Tensor], ref_len: int = 0, lengths=None) -> torch.Tensor:
        """bicodec.py:174-178: batch["ref_wav"] [B, T] -> global tokens int32 [B, 1, token_num].  ref_len > 0 takes the mel spectrogram of
        BiCodecTokenizer.get_ref_clip(ref_wav) of that length (tile a short row, truncate a long one) without materialising the clip.

        lengths: the clips' lengths in SAMPLES (host list / tensor, B entries, 1 .. T); needs ref_len > 0.  The
        reference clip of row b is then get_ref_clip(ref_wav[b, :lengths[b]]): it tiles by its own length, and samples behind it are
        never read."""
        wav = self._ref_wav(batch)
        B, T = wav.shape
        arr = None if lengths is None else clip_lengths(lengths, B, 1, T, "BiCodec.get_global_tokens")[1]
        out = torch.empty((B, 1, self.encoder_spec.token_num), dtype=torch.int32, device=self.device)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        if arr is None:
            _lib.check(self._lib.qa_bicodec_get_global_tokens(self._enc, wav.data_ptr(), B, T, int(ref_len), out.data_ptr(), stream))
        else:
            _lib.check(self._lib.qa_bicodec_get_global_tokens_ragged(self._enc, wav.data_ptr(), B, T, arr, int(ref_len), out.data_ptr(), stream))
        return out

    @torch.no_grad()
    def tokenize(self, batch: Mapping[str, torch.Tensor], ref_len: int = 0, lengths=None, frame_lengths=None):
        """bicodec.py:151-165: (semantic_tokens int64 [B, N], global_tokens int32 [B, 1, token_num]).

        Per-clip calls pass both vectors: `lengths`, the clips' samples in batch["ref_wav"] (as
        get_global_tokens), and `frame_lengths`, their frames in batch["feat"] (as get_semantic_tokens) - the front-end's frame rule
        relates the two (SSLFeatureExtractor.frames, BiCodecTokenizer.token_frames).  Both are checked before anything is launched,
        and the call is ONE library call."""
        if lengths is None and frame_lengths is None:
            return self.get_semantic_tokens(batch), self.get_global_tokens(batch, ref_len)
        if lengths is None or frame_lengths is None:
            raise _lib.QuarkAudioError(-1, "BiCodec.tokenize: a per-clip call needs lengths (samples of ref_wav) and frame_lengths (frames of "
                                           "feat) together")
        feat, wav = self._feat(batch), self._ref_wav(batch)
        B, N, _ = feat.shape
        if wav.shape[0] != B:
            raise _lib.QuarkAudioError(-1, f"ref_wav must be [B, T] with B = {B}, got {tuple(wav.shape)}")
        T = wav.shape[1]
        sarr = clip_lengths(lengths, B, 1, T, "BiCodec.tokenize")[1]
        farr = clip_lengths(frame_lengths, B, 1, N, "BiCodec.tokenize: frame_lengths", "N")[1]
        sem = torch.empty((B, N), dtype=torch.int64, device=self.device)
        glob = torch.empty((B, 1, self.encoder_spec.token_num), dtype=torch.int32, device=self.device)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        _lib.check(self._lib.qa_bicodec_tokenize_ragged(self._enc, feat.data_ptr(), B, N, farr, wav.data_ptr(), T, sarr, int(ref_len),
                                                        sem.data_ptr(), glob.data_ptr(), stream))
        return sem, glob

    def enable_taps(self, on: bool = True):
        _lib.check(self._lib.qa_bicodec_enable_taps(self._handle, int(on)))
        if self._enc.value:
            _lib.check(self._lib.qa_bicodec_enc_enable_taps(self._enc, int(on)))
        return self

    def tap(self, name: str) -> torch.Tensor:
        """Intermediates of the last call: detokenize's (z_q, prenet.*, gen.block{i}, ...), get_semantic_tokens' (enc.*, vq.latent) and
        get_global_tokens' (mel, ecapa.*, perceiver.out, fsq.bounded); forward adds ecapa.pool [B, 3072], x_vector and postnet.out
        [B, N, out_channels]."""
        encoder_side = name.startswith(("enc.", "vq.", "mel", "ecapa.", "perceiver.", "fsq.", "x_vector"))
        h, fn = (self._enc, self._lib.qa_bicodec_enc_tap) if encoder_side else (self._handle, self._lib.qa_bicodec_tap)
        n = fn(h, name.encode(), None, 0, None)
        if n < 0:
            _lib.check(int(n))
        out = torch.empty(int(n), dtype=torch.float32, device=self.device)
        n2 = fn(h, name.encode(), out.data_ptr(), n, torch.cuda.current_stream(self.device).cuda_stream)
        if n2 < 0:
            _lib.check(int(n2))
        return out

    def _free(self):
        if getattr(self, "_handle", None) is not None and self._handle.value:
            self._lib.qa_bicodec_destroy(self._handle)
            self._handle = C.c_void_p()
        if getattr(self, "_enc", None) is not None and self._enc.value:
            self._lib.qa_bicodec_enc_destroy(self._enc)
            self._enc = C.c_void_p()

    def __del__(self):
        try:
            self._free()
        except Exception:
            pass


class BiCodecTokenizer(torch.nn.Module):
    """The reference's BiCodecTokenizer (QuarkAudio-UniSE/model/bicodec/audio_tokenizer.py): `detokenize(global_tokens [B, 1, 32],
    semantic_tokens [B, T]) -> wav [B, 1, T * 320]`, the call `Model.test_step` makes, and `tokenize(wav) -> (global int32 [B, 1, 32],
    semantic int64 [B, N])` with its parts `extract_wav2vec2_features(wav)` (normalise + XLSR-53 hidden states 11 / 14 / 16) and
    `get_semantic_tokens(wav)`.  The XLSR-53 front-end is `feature_extractor=` (an SSLFeatureExtractor built with SPEC_XLSR53_BICODEC)
    or, loaded on first use, `{model_dir}/wav2vec2-large-xlsr-53` (audio_tokenizer.py:47-52)."""

    def __init__(self, model_dir=None, device="cuda:0", *, model: BiCodec | None = None, spec: BiCodecSpec | None = None,
                 feature_extractor=None, **kwargs):
        super().__init__()
        self.model_dir = model_dir
        self.config = None
        if feature_extractor is not None:
            self._check_extractor(feature_extractor)
        self._feature_extractor = feature_extractor
        if model is None:
            if model_dir is None:
                raise ValueError("BiCodecTokenizer needs model_dir (with BiCodec/config.yaml and BiCodec/model.safetensors) or model=")
            import os

            if os.path.isfile(f"{model_dir}/config.yaml"):  # audio_tokenizer.py:40 (sample_rate, ref_segment_duration, latent_hop_length: tokenize side)
                self.config = load_config(f"{model_dir}/config.yaml")
            model = BiCodec.load_from_checkpoint(f"{model_dir}/BiCodec", device=device, spec=spec)  # audio_tokenizer.py:45
        self.model = model
        self.device = model.device

    @torch.no_grad()
    def detokenize(self, global_tokens: torch.Tensor, semantic_tokens: torch.Tensor, lengths=None) -> torch.Tensor:
        """lengths: the clips' lengths in TOKENS (`token_frames(sample_lengths)` for the output of `tokenize(wav, lengths=...)`), as
        BiCodec.detokenize takes them."""
        return self.model.detokenize(semantic_tokens, global_tokens, lengths=lengths)

    def token_frames(self, sample_lengths):
        """Semantic tokens per clip for clips of these many samples: the XLSR-53 front-end's frame rule (floor), clip by clip."""
        fx = self.feature_extractor
        return [fx.frames(int(n)) for n in (sample_lengths.tolist() if torch.is_tensor(sample_lengths) else sample_lengths)]

    @staticmethod
    def _check_extractor(fx):
        from .ssl import SSLFeatureExtractor

        if not isinstance(fx, SSLFeatureExtractor):
            raise _lib.QuarkAudioError(-1, f"feature_extractor must be an SSLFeatureExtractor (SPEC_XLSR53_BICODEC), got {type(fx).__name__}")
        want = {"select": (11, 14, 16), "pad": 0, "compress_exponent": 0.0}
        have = {k: (tuple(getattr(fx.spec, k)) if k == "select" else getattr(fx.spec, k)) for k in want}
        if have != want:
            raise _lib.QuarkAudioError(-1, f"BiCodec averages XLSR-53 hidden states 11 / 14 / 16 of the unpadded, uncompressed input "
                                           f"({want}); the SSLFeatureExtractor was built with {have} - use SPEC_XLSR53_BICODEC")

    @property
    def feature_extractor(self):
        if self._feature_extractor is None:
            if self.model_dir is None:
                raise _lib.QuarkAudioError(-3, "no XLSR-53 front-end: pass feature_extractor= or a model_dir with wav2vec2-large-xlsr-53/")
            import dataclasses
            import json
            import os

            from .ssl import SPEC_XLSR53_BICODEC, SSLFeatureExtractor, SSLSpec

            path = f"{self.model_dir}/wav2vec2-large-xlsr-53"
            spec = SPEC_XLSR53_BICODEC
            if os.path.isfile(f"{path}/config.json"):  # the snapshot's Wav2Vec2Config, with what BiCodecTokenizer does around the model
                with open(f"{path}/config.json") as f:
                    cfg = json.load(f)
                names = {fl.name for fl in dataclasses.fields(SSLSpec)}
                kw = {k: (tuple(v) if isinstance(v, list) else v) for k, v in cfg.items() if k in names}
                spec = dataclasses.replace(SSLSpec(**kw), select=SPEC_XLSR53_BICODEC.select, pad=0, compress_exponent=0.0)
            self._feature_extractor = SSLFeatureExtractor.from_pretrained(path, spec, device=self.device)
        return self._feature_extractor

    @torch.no_grad()
    def extract_wav2vec2_features(self, wavs: torch.Tensor, lengths=None) -> torch.Tensor:
        """audio_tokenizer.py:74-90: wavs [B, T] -> (hidden_states[11] + [14] + [16]) / 3 of the normalised rows, [B, N, 1024].
        lengths (samples, 400 .. T each): every row normalised over, and its features taken of, its own samples; one front-end call."""
        wavs = wavs.to(device=self.device, dtype=torch.float32)
        if wavs.dim() == 1:
            wavs = wavs.unsqueeze(0)
        fx = self.feature_extractor
        if wavs.dim() != 2 or wavs.shape[-1] < 400:  # the 10-sample / stride-5 conv stack needs 400 samples for one frame
            raise _lib.QuarkAudioError(-1, f"wav must be [B, T] with T >= 400 samples (one XLSR-53 frame at 16 kHz), got {tuple(wavs.shape)}")
        if lengths is None:
            return fx(wav_normalize(wavs))
        lens = clip_lengths(lengths, wavs.shape[0], 400, wavs.shape[1], "BiCodecTokenizer")[0]
        return fx(wav_normalize(wavs, lengths=lens), lengths=lens)

    @property
    def ref_segment_length(self) -> int:
        """audio_tokenizer.py:60-64 from `{model_dir}/config.yaml` (sample_rate, ref_segment_duration, latent_hop_length); the published
        values (16 kHz, 6 s, 320) without one."""
        c = self.config or {}
        spec = self.model.encoder_spec
        return int(c.get("sample_rate", spec.sample_rate) * c.get("ref_segment_duration", 6)) // int(c.get("latent_hop_length", 320)) \
            * int(c.get("latent_hop_length", 320))

    @torch.no_grad()
    def get_semantic_tokens(self, wavs: torch.Tensor) -> torch.Tensor:
        """The semantic half of tokenize (audio_tokenizer.py:95-103 + bicodec.py:167-172): wavs [B, T] -> semantic tokens int64 [B, N]."""
        return self.model.get_semantic_tokens({"feat": self.extract_wav2vec2_features(wavs)})

    @torch.no_grad()
    def tokenize(self, wav: torch.Tensor, lengths=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """audio_tokenizer.py:93-103: wav [B, T] -> (global_tokens int32 [B, 1, token_num], semantic_tokens int64 [B, N]).  The reference
        clip (get_ref_clip) is formed inside the mel kernel.

        lengths: the clips' lengths in SAMPLES (host list / tensor, B entries, 400 .. T), clip b in
        wav[b, :lengths[b]].  Row b then holds what tokenize(wav[b:b+1, :lengths[b]]) returns - its own normalisation, its own
        features, its own reference clip - in the first token_frames(lengths)[b] semantic tokens, and -1 behind them.  One
        normalisation, one front-end call, one codec call; what wav holds behind a clip's end is never read."""
        wav = wav.to(device=self.device, dtype=torch.float32)
        if wav.dim() == 1:
            wav = wav.unsqueeze(0)
        if lengths is None:
            feat = self.extract_wav2vec2_features(wav)
            semantic, global_tokens = self.model.tokenize({"feat": feat, "ref_wav": wav, "wav": wav}, ref_len=self.ref_segment_length)
            return global_tokens, semantic
        feat = self.extract_wav2vec2_features(wav, lengths=lengths)  # checks the lengths before anything is launched
        lens = [int(v) for v in (lengths.tolist() if torch.is_tensor(lengths) else lengths)]
        semantic, global_tokens = self.model.tokenize({"feat": feat, "ref_wav": wav, "wav": wav}, ref_len=self.ref_segment_length,
                                                      lengths=lens, frame_lengths=self.token_frames(lens))
        return global_tokens, semantic
