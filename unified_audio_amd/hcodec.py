"""Python mirror of the reference's H-Codec interface, backed by libquarkaudio_hip.so.

    Codec            <-> QuarkAudio-HCodec/HCodec-1.0/vq/codec.py:21-187        (encode / decode / load_state_dict)
    HCodecTokenizer  <-> QuarkAudio-HCodec/HCodec-1.0/audio_tokenizer.py:18-66  (pad_wav / tokenize / detokenize)

Tensors stay PyTorch-ROCm CUDA tensors (allocation + streams only); all arithmetic happens in the HIP library.
"""
from __future__ import annotations

import ctypes as C
import math
from contextlib import contextmanager
from dataclasses import dataclass
from typing import Callable, Dict, Optional, Tuple

import torch

from . import _lib


@dataclass(frozen=True)
class HCodecSpec:
    """Architecture constants of H-Codec 1.0, hard-coded in the reference at vq/codec.py:30-136."""

    n_filters: int = 32
    ratios: Tuple[int, ...] = (2, 4, 5, 8)  # encoder order (codec.py:33 lists [8,5,4,2]; seanet.py:114 reverses)
    dimension: int = 512
    enc_heads: int = 8
    enc_layers: int = 2
    sem_in: int = 768
    sem_ch: int = 768
    sem_strides: Tuple[int, ...] = (2, 1)
    code_dim: int = 512
    codebook_size: int = 1024
    num_quantizers: int = 4
    dec_dim: int = 768
    dec_inter: int = 2304
    dec_heads: int = 8
    dec_layers: int = 2
    convnext_layers: int = 12
    n_fft: int = 1280
    hop: int = 320
    gn_groups: int = 32
    # H-Codec 1.5 (QuarkAudio-HCodec/HCodec-1.5/conf/config_adaptive_v3.yaml:65-111); adaptive=False is H-Codec 1.0
    adaptive: bool = False
    agg_layers: int = 32
    agg_heads: int = 8
    agg_ff: int = 2048
    bt_layers: int = 32
    bt_heads: int = 8
    bt_ff: int = 2048
    threshold: float = 0.6
    max_tokens_per_group: int = 8
    # H-Codec 2.0 (QuarkAudio-HCodec/HCodec-2.0/conf/large_12.5hz_config.yaml); version 10 = SEANet family (1.0 / 1.5)
    version: int = 10
    enc_dim: int = 1536
    enc_inter: int = 4608
    enc_convnext_layers: int = 24
    frame_stride: int = 4
    tr_inter_cap: int = 0  # transformer MLP width = min(4 d, cap); 0 = 4 d
    # the causal variant every block of the SEANet family parameterises (encoder_modules/conv.py:203-206, vq/conv.py:44-47,76-79,
    # encoder_modules/transformer.py:470-475); vq/codec.py:31 ships False
    causal: bool = False
    # H-Codec 1.5: `causal` / `context_frames` of the aggregators, `causal` / `context` of the bottleneck transformer
    # (config_adaptive_v3.yaml:84-105; shipped causal: false, where mimi/transformer.py:403-413 ignores the context)
    agg_causal: bool = False
    agg_context: int = 16
    bt_causal: bool = False
    bt_context: int = 16

    @property
    def enc_hop(self) -> int:
        """samples per code frame"""
        if self.version == 20:
            return self.hop * self.frame_stride
        return int(math.prod(self.ratios)) * 2

    @property
    def dec_upsample(self) -> int:
        return self.frame_stride if self.version == 20 else 2

    def to_c(self) -> "_lib.qa_hcodec_spec":
        s = _lib.qa_hcodec_spec()
        s.n_filters, s.n_ratios = self.n_filters, len(self.ratios)
        for i, r in enumerate(self.ratios):
            s.ratios[i] = r
        s.dimension, s.enc_heads, s.enc_layers = self.dimension, self.enc_heads, self.enc_layers
        s.sem_in, s.sem_ch, s.n_sem_strides = self.sem_in, self.sem_ch, len(self.sem_strides)
        for i, r in enumerate(self.sem_strides):
            s.sem_strides[i] = r
        s.code_dim, s.codebook_size, s.num_quantizers = self.code_dim, self.codebook_size, self.num_quantizers
        s.dec_dim, s.dec_inter, s.dec_heads, s.dec_layers = self.dec_dim, self.dec_inter, self.dec_heads, self.dec_layers
        s.convnext_layers, s.n_fft, s.hop, s.gn_groups = self.convnext_layers, self.n_fft, self.hop, self.gn_groups
        s.adaptive, s.agg_layers, s.agg_heads, s.agg_ff = int(self.adaptive), self.agg_layers, self.agg_heads, self.agg_ff
        s.bt_layers, s.bt_heads, s.bt_ff = self.bt_layers, self.bt_heads, self.bt_ff
        s.max_tokens_per_group, s.threshold = self.max_tokens_per_group, self.threshold
        s.version, s.enc_dim, s.enc_inter = self.version, self.enc_dim, self.enc_inter
        s.enc_convnext_layers, s.frame_stride, s.tr_inter_cap = self.enc_convnext_layers, self.frame_stride, self.tr_inter_cap
        s.causal = int(self.causal)
        s.agg_causal, s.agg_context, s.bt_causal, s.bt_context = int(self.agg_causal), self.agg_context, int(self.bt_causal), self.bt_context
        return s


SPEC_10 = HCodecSpec()
# H-Codec 1.5: SEANet stride order 8,5,4,2 (config lists [2,4,5,8], seanet.py:114 reverses it), XLSR features, decoder 1024
SPEC_15 = HCodecSpec(ratios=(8, 5, 4, 2), sem_in=1024, sem_ch=1024, dec_dim=1024, dec_inter=2304, adaptive=True)
# H-Codec 2.0: 48 kHz, 12.5 Hz frames, STFT/ConvNeXt encoder, 16 + 16 codebooks
SPEC_20 = HCodecSpec(version=20, enc_dim=1536, enc_inter=4608, enc_convnext_layers=24, enc_layers=2, frame_stride=4,
                     tr_inter_cap=4096, dimension=512, sem_in=768, sem_ch=1536, sem_strides=(2, 1, 2), num_quantizers=16,
                     dec_dim=1536, dec_inter=4608, dec_heads=24, dec_layers=2, convnext_layers=32, n_fft=1920, hop=960)


@dataclass(frozen=True)
class SemanticDecoderSpec:
    """`semantic_module.Decoder` (QuarkAudio-HCodec/HCodec-1.0/vq/semantic_module.py:247-300): the codec's semantic decoder, which rebuilds
    the SSL features from the summed semantic code vectors (`pred_feat` of `Codec.forward`).  Every shipped configuration mirrors the
    semantic encoder: output = sem_in, width = sem_ch, strides = sem_strides, channel ratios all 1 (`from_codec_spec`)."""

    code_dim: int = 512
    output_channels: int = 768
    decode_channels: int = 768
    channel_ratios: Tuple[float, ...] = (1, 1)
    strides: Tuple[int, ...] = (2, 1)

    @staticmethod
    def from_codec_spec(spec: HCodecSpec) -> "SemanticDecoderSpec":
        return SemanticDecoderSpec(code_dim=spec.code_dim, output_channels=spec.sem_in, decode_channels=spec.sem_ch,
                                   channel_ratios=(1,) * len(spec.sem_strides), strides=tuple(spec.sem_strides))

    @staticmethod
    def from_kwargs(kw: dict) -> "SemanticDecoderSpec":
        """The reference's constructor keywords (decoder_config.semantic_decoder of the 1.5 YAML, semantic_decoder_config of 2.0)."""
        strides = tuple(kw.get("strides", (1, 1)))
        return SemanticDecoderSpec(code_dim=kw["code_dim"], output_channels=kw["output_channels"], decode_channels=kw["decode_channels"],
                                   channel_ratios=tuple(kw.get("channel_ratios", (1,) * len(strides))), strides=strides)

    @property
    def widths(self) -> Tuple[int, ...]:
        """output width of every DecoderBlock (semantic_module.py:276-281)"""
        n, dc, r = len(self.strides), self.decode_channels, self.channel_ratios
        return tuple(int(dc * r[i + 1]) if i < n - 1 else dc for i in range(n))

    def to_c(self) -> "_lib.qa_semantic_decoder_spec":
        if len(self.channel_ratios) != len(self.strides) or not 1 <= len(self.strides) <= 4:
            raise _lib.QuarkAudioError(-1, f"semantic decoder: {len(self.strides)} strides / {len(self.channel_ratios)} channel ratios")
        s = _lib.qa_semantic_decoder_spec()
        s.code_dim, s.channels, s.n_blocks = self.code_dim, int(self.decode_channels * self.channel_ratios[0]), len(self.strides)
        for i, (st, w) in enumerate(zip(self.strides, self.widths)):
            s.strides[i], s.widths[i] = st, w
        s.output_channels = self.output_channels
        return s


def code_frames(sample_lengths, hop: int):
    """Code frames of clips of `sample_lengths` samples: ceil(len / hop) each, as `HCodecTokenizer.pad_wav` pads a clip alone.  A list of
    ints; every length must be positive."""
    out = []
    for i, n in enumerate(_int_list(sample_lengths, "lengths")):
        if n < 1:
            raise _lib.QuarkAudioError(-1, f"lengths[{i}] = {n}: a clip needs at least one sample")
        out.append(-(-n // hop))
    return out


def _int_list(values, what: str):
    """A 1-D sequence / tensor of integers as a list of Python ints (host side: the lengths of a ragged call are host memory)."""
    if torch.is_tensor(values):
        if values.dim() != 1 or values.is_floating_point() or values.is_complex():
            raise _lib.QuarkAudioError(-1, f"{what} must be a 1-D integer tensor, got {values.dtype} {tuple(values.shape)}")
        values = values.tolist()
    out = []
    for i, v in enumerate(values):
        if isinstance(v, bool) or int(v) != v:
            raise _lib.QuarkAudioError(-1, f"{what}[{i}] = {v!r} is not an integer")
        out.append(int(v))
    return out


def _frames_arg(lengths, B: int, what: str = "lengths"):
    """The `frames` argument of qa_hcodec_encode_ragged / _decode_ragged: a host int64[B] from a list or tensor of code-frame counts.  The
    range check (1 .. N, naming the row) is the library's; this only refuses what cannot be passed on."""
    vals = _int_list(lengths, what)
    if len(vals) != B:
        raise _lib.QuarkAudioError(-1, f"{what} has {len(vals)} entries for a batch of {B}")
    return (C.c_int64 * B)(*vals)


MAX_STREAM_FRAMES = 4096  # code frames a stream can hold: the encoder Transformer's 8192 positions at two per code frame


class _DefaultInt(int):
    """A default argument that can be told from the same number given by the caller (`x is DEFAULT`)."""


_DEFAULT_STREAM_FRAMES = _DefaultInt(MAX_STREAM_FRAMES)


def _stream_ptr(device: torch.device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def _semantic_decoder_spec_from_config(config: dict) -> Optional[SemanticDecoderSpec]:
    """SemanticDecoderSpec from the reference's YAML dictionaries (1.5: decoder_config.semantic_decoder, 2.0: semantic_decoder_config);
    None when they carry none."""
    kw = config.get("semantic_decoder_config") or (config.get("decoder_config") or {}).get("semantic_decoder")
    return SemanticDecoderSpec.from_kwargs(kw) if isinstance(kw, dict) else None


def _spec_from_config(config: dict, device=None) -> HCodecSpec:
    """HCodecSpec from the reference's YAML dictionaries: HCodec-1.5/conf/config_adaptive_v3.yaml (keys encoder_config /
    decoder_config / quantizer_config / adaptive_config) or HCodec-2.0/conf/large_12.5hz_config.yaml (encoder_config with
    n_fft / target_frame_rate, semantic_encoder_config)."""
    enc, dec, qz = config["encoder_config"], config["decoder_config"], config["quantizer_config"]
    if "adaptive_config" in config:  # H-Codec 1.5
        e, se, d, q, ad = enc["encoder"], enc["semantic_encoder"], dec["decoder"], qz["quantizer"], config["adaptive_config"]
        agg, tk = ad["aggregators"]["semantic_aggregator"], ad["transformer_kwargs"]
        thr = ad.get("manual_threshold")
        return HCodecSpec(n_filters=e["n_filters"], ratios=tuple(reversed(e["ratios"])), dimension=e["dimension"],
                          sem_in=se["input_channels"], sem_ch=se["encode_channels"], sem_strides=tuple(se["strides"]),
                          code_dim=q["dim"], codebook_size=q["codebook_size"], num_quantizers=q["num_quantizers"],
                          dec_dim=d["dim"], dec_inter=d["intermediate_dim"], adaptive=True, agg_layers=agg["num_layers"],
                          agg_heads=agg["num_heads"], agg_ff=agg["dim_feedforward"], bt_layers=tk["num_layers"],
                          bt_heads=tk["num_heads"], bt_ff=tk["dim_feedforward"],
                          threshold=float(thr if thr is not None else ad["similarity_threshold"]),
                          max_tokens_per_group=ad["max_tokens_per_group"],
                          agg_causal=bool(agg.get("causal", False)), agg_context=int(agg.get("context_frames") or 0),
                          bt_causal=bool(tk.get("causal", False)), bt_context=int(tk.get("context") or 0))
    se = config["semantic_encoder_config"]  # H-Codec 2.0
    stride = int(50 / enc["target_frame_rate"])
    return HCodecSpec(version=20, enc_dim=enc["dim"], enc_inter=enc["intermediate_dim"], enc_convnext_layers=enc["convnext_layers"],
                      enc_layers=enc["transformer_layers"], frame_stride=stride, tr_inter_cap=4096, dimension=enc["dimension"],
                      sem_in=se["input_channels"], sem_ch=se["encode_channels"], sem_strides=tuple(se["strides"]),
                      code_dim=qz["dim"], codebook_size=qz["codebook_size"], num_quantizers=qz["num_quantizers"],
                      dec_dim=dec["dim"], dec_inter=dec["intermediate_dim"], dec_heads=dec["dim"] // 64,
                      dec_layers=dec["transformer_layers"], convnext_layers=dec["convnext_layers"], n_fft=enc["n_fft"],
                      hop=enc["hop_length"], causal=bool(enc.get("causal", False)))


class Codec(torch.nn.Module):
    """Drop-in for `vq.Codec` on the inference path: `encode(x, feat)` / `decode(acoustic_codes, semantic_codes)`.

    The constructor keeps the reference's positional kwargs dicts (1.0: codec.py:22-27, ignored - the architecture is hard-coded
    there; 1.5: encoder / decoder / quantizer / adaptive configs; 2.0: + semantic encoder / decoder configs): when the YAML
    dictionaries are given the architecture is read from them, otherwise from `spec`.  Weights come through `load_state_dict`
    in the reference's own key layout (weight_g / weight_v, `layers.{q}._codebook.embed`).  It is an `nn.Module` without
    parameters of its own (the folded weights live in the library's device blob): `.eval()`, `.requires_grad_()`,
    `.to(device)` / `.cuda()` work as for the reference module - moving to another GPU re-creates the handle there from the
    state_dict it was loaded with - and `.train()` / `.half()` raise: this is the fp32 inference path.
    """

    def __init__(self, encoder_kwargs=None, decoder_kwargs=None, quantizer_kwargs=None, adaptive_kwargs=None,
                 semantic_decoder_kwargs=None, *, spec: Optional[HCodecSpec] = None,
                 semantic_decoder_spec: Optional[SemanticDecoderSpec] = None,
                 device: str | torch.device = "cuda:0", check_codes: bool = True):
        super().__init__()
        adaptive_cfg = isinstance(encoder_kwargs, dict) and isinstance(adaptive_kwargs, dict) and "aggregators" in adaptive_kwargs
        if spec is None:
            if adaptive_cfg:
                spec = _spec_from_config({"encoder_config": encoder_kwargs, "decoder_config": decoder_kwargs,
                                          "quantizer_config": quantizer_kwargs, "adaptive_config": adaptive_kwargs})
            elif isinstance(encoder_kwargs, dict) and "n_fft" in encoder_kwargs:  # 2.0: Codec(enc, dec, quant, sem_enc, sem_dec)
                spec = _spec_from_config({"encoder_config": encoder_kwargs, "decoder_config": decoder_kwargs,
                                          "quantizer_config": quantizer_kwargs, "semantic_encoder_config": adaptive_kwargs})
            else:
                spec = SPEC_10
        if semantic_decoder_spec is None:
            semantic_decoder_spec = _semantic_decoder_spec_from_config(
                {"decoder_config": decoder_kwargs if isinstance(decoder_kwargs, dict) else None,
                 "semantic_decoder_config": semantic_decoder_kwargs if isinstance(semantic_decoder_kwargs, dict) else None})
        self.spec = spec
        self.semantic_decoder_spec = semantic_decoder_spec or SemanticDecoderSpec.from_codec_spec(spec)
        # the 1.5 dynamic-threshold draw (codec_adaptive.py:91-95: infer_using_dynamic_threshold without a manual_threshold) is random
        # per call; forward refuses it rather than use a fixed threshold
        self.dynamic_threshold = bool(adaptive_cfg and adaptive_kwargs.get("infer_using_dynamic_threshold")
                                      and adaptive_kwargs.get("manual_threshold") is None)
        self.device = torch.device(device)
        self.check_codes = check_codes  # decode(): refuse out-of-range codes like F.embedding (one tiny kernel + one sync)
        self._handle = C.c_void_p()
        self._lib = _lib.load_library()
        self._state = None
        self._semantic_decoder_error = None  # why forward cannot run (no / incomplete semantic_decoder.* weights)
        self._streaming_batch = 0  # > 0: inside streaming() (encode_stream)

    # -- weights -------------------------------------------------------------------------------------
    def load_state_dict(self, state_dict: Dict[str, torch.Tensor], strict: bool = True, assign: bool = False):
        _lib.require_device()
        if self.device.type != "cuda":
            raise _lib.QuarkAudioError(-1, f"Codec lives on a HIP device, got {self.device}")
        self._free()
        table, n, keep = _lib.tensor_table(state_dict)
        spec_c = self.spec.to_c()
        handle = C.c_void_p()
        _lib.check(self._lib.qa_hcodec_create(C.byref(handle), C.byref(spec_c), table, n, self.device.index or 0))
        self._handle = handle
        # the semantic decoder (forward's pred_feat) is optional: encode / decode never read it, and a checkpoint without (all of) its
        # weights still loads - forward then raises naming the first missing or mis-shaped key
        try:
            sd_c = self.semantic_decoder_spec.to_c()
            st = self._lib.qa_hcodec_load_semantic_decoder(handle, C.byref(sd_c), table, n)
            self._semantic_decoder_error = None if st == 0 else (st, self._lib.qa_last_error().decode("utf-8", "replace"))
        except _lib.QuarkAudioError as e:
            self._semantic_decoder_error = (e.status, str(e))
        del keep
        self._state = state_dict  # a reference, not a copy: lets .to(other_gpu) rebuild the handle there
        return self

    def state_dict(self, *args, destination=None, prefix: str = "", keep_vars: bool = False):
        """The state_dict this handle was loaded with (reference key layout)."""
        out = destination if destination is not None else {}
        for k, v in (self._state or {}).items():
            out[prefix + k] = v
        return out

    def train(self, mode: bool = True):
        if mode:
            raise _lib.QuarkAudioError(-4, "unified_audio_amd.Codec is the inference path (the reference calls .eval(), audio_tokenizer.py:26)")
        return super().train(False)  # nn.Module bookkeeping: self.training = False, recursion into (no) children

    def to(self, *args, **kwargs):
        device = kwargs.get("device")
        dtype = kwargs.get("dtype")
        for a in args:
            if isinstance(a, (str, torch.device, int)):
                device = a
            elif isinstance(a, torch.dtype):
                dtype = a
        if dtype is not None and dtype != torch.float32:
            raise _lib.QuarkAudioError(-4, f"the path computes in fp32 like the reference; {dtype} is not supported")
        if device is None:
            return self
        device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device() if torch.cuda.is_available() else 0)
        if device.type != "cuda":
            raise _lib.QuarkAudioError(-1, f"there is no CPU path: Codec cannot move to {device}")
        if device != self.device:
            self.device = device
            if self._state is not None:
                self.load_state_dict(self._state)
        return self

    def cuda(self, device=None):
        return self.to(torch.device("cuda", device if device is not None else (self.device.index or 0)))

    def cpu(self):
        raise _lib.QuarkAudioError(-1, "there is no CPU path")

    def half(self):
        return self.to(torch.float16)

    def float(self):
        return self

    @torch.no_grad()
    def forward(self, x: torch.Tensor, feat: Optional[torch.Tensor] = None, use_mask=False, domain_split=None):
        """Codec.forward in eval mode: 1.0 codec.py:138-162, 2.0 codec.py:54-72 -> (recon [B, T], pred_feat [B, sem_in, N_feat],
        commit_loss); 1.5 codec_adaptive.py:100-148 -> {'recon', 'pred_feat', 'commit_loss', 'token_lengths' [B, G] int64}.

        recon is decode(encode(x, feat)) bit for bit (the same kernels on the same device-resident codes); pred_feat is the semantic
        decoder on the summed semantic code vectors (1.5: de-aggregated back to the 25 Hz frames first).  commit_loss is a 0-dim 0.:
        the checked-in vector_quantize_pytorch stand-in returns zero losses, and upstream ResidualVQ (1.22.x, recalled, not diffed here)
        adds its commitment terms only under `self.training`, which this inference module never is.  `use_mask` / `domain_split`
        are accepted and ignored, as by the reference.  All outputs are fp32 tensors on the codec's device."""
        self._require_loaded()
        if self._semantic_decoder_error is not None:
            st, msg = self._semantic_decoder_error
            raise _lib.QuarkAudioError(st, f"Codec.forward needs the semantic decoder weights (semantic_decoder.*): {msg}")
        if feat is None:
            raise _lib.QuarkAudioError(-1, "Codec.forward(x, feat): feat (the SSL features) is required")
        if self.spec.adaptive and self.dynamic_threshold:
            raise _lib.QuarkAudioError(-4, "Codec.forward: the config draws a random similarity threshold per call "
                                           "(infer_using_dynamic_threshold without manual_threshold); set manual_threshold")
        if x.dim() == 2:  # H-Codec 2.0 passes wav without the channel dim
            x = x.unsqueeze(1)
        if x.dim() != 3 or x.shape[1] != 1:
            raise _lib.QuarkAudioError(-1, f"forward expects x of shape [B,1,T], got {tuple(x.shape)}")
        if feat.dim() != 3 or feat.shape[0] != x.shape[0] or feat.shape[1] != self.spec.sem_in:
            raise _lib.QuarkAudioError(-1, f"forward expects feat of shape [B,{self.spec.sem_in},N], got {tuple(feat.shape)}")
        x = x.to(device=self.device, dtype=torch.float32).contiguous()
        feat = feat.to(device=self.device, dtype=torch.float32)
        B, _, T = x.shape
        n25 = T // self.spec.enc_hop
        sds = self.semantic_decoder_spec
        recon = torch.empty((B, n25 * self.spec.dec_upsample * self.spec.hop), dtype=torch.float32, device=self.device)
        pred = torch.empty((B, sds.output_channels, n25 * int(math.prod(sds.strides))), dtype=torch.float32, device=self.device)
        commit_loss = torch.zeros((), dtype=torch.float32, device=self.device)
        sb, sch, st = feat.stride()
        if self.spec.adaptive:
            tl = torch.empty((B, max(n25, 1)), dtype=torch.int64, device=self.device)
            g = C.c_int64(0)
            _lib.check(self._lib.qa_hcodec_forward_adaptive(self._handle, x.data_ptr(), B, T, feat.data_ptr(), sb, sch, st, feat.shape[2],
                                                            recon.data_ptr(), pred.data_ptr(), tl.data_ptr(), C.byref(g),
                                                            _stream_ptr(self.device)))
            G = int(g.value)
            return {"recon": recon, "pred_feat": pred, "commit_loss": commit_loss, "token_lengths": tl.view(-1)[: B * G].view(B, G)}
        _lib.check(self._lib.qa_hcodec_forward(self._handle, x.data_ptr(), B, T, feat.data_ptr(), sb, sch, st, feat.shape[2],
                                               recon.data_ptr(), pred.data_ptr(), _stream_ptr(self.device)))
        return recon, pred, commit_loss

    @property
    def has_semantic_decoder(self) -> bool:
        return bool(self._handle.value) and self._lib.qa_hcodec_has_semantic_decoder(self._handle) == 1

    def _free(self):
        if getattr(self, "_handle", None) is not None and self._handle.value:
            self._lib.qa_hcodec_destroy(self._handle)  # a stream of the handle goes with it
            self._handle = C.c_void_p()
        self._streaming_batch = 0

    def __del__(self):
        try:
            self._free()
        except Exception:
            pass

    def _require_loaded(self):
        if not self._handle.value:
            raise _lib.QuarkAudioError(-3, "Codec has no weights: call load_state_dict first")

    def _check_range_begin(self, tensors, limit: int, lo: int = 0):
        """F.embedding's range check (reference: IndexError on the host, device-side assert on a GPU), first half: one tiny counting kernel
        per code tensor into a device counter - NO host synchronisation here.  `_check_range_end` reads the counter behind a
        synchronisation the decode performs anyway (the in-launch LSTM's ticket, or H-Codec 1.5's frame-count read-back), so a decode costs
        one host round trip less than with the synchronous check of round 3.  `check_codes=False` skips it (the kernels clamp indices for
        memory safety)."""
        if not self.check_codes:
            return None
        bad = torch.zeros(1, dtype=torch.int64, device=self.device)
        for t in tensors:
            _lib.check(self._lib.qa_codes_check_async(t.data_ptr(), t.numel(), lo, limit, bad.data_ptr(), _stream_ptr(self.device)))
        return bad, lo, limit

    @staticmethod
    def _check_range_end(pending):
        if pending is None:
            return
        bad, lo, limit = pending
        n = int(bad.item())
        if n:
            raise IndexError(f"{n} code indices out of range [{lo}, {limit})")

    # -- hot path ------------------------------------------------------------------------------------
    @torch.no_grad()
    def encode(self, x: torch.Tensor, feat: torch.Tensor, use_mask=False, domain_split=None, threshold: float = 0.0, lengths=None):
        """codec.py:166-175.  x [B,1,T] fp32, feat [B, sem_in, N50] fp32 (any strides) -> two int64 [B, nq, N25].

        lengths (non-causal H-Codec 1.0): the clips' lengths in CODE frames, a host list / tensor of B values in 1 .. N25.  Row b then
        equals encode of that clip alone at its own length; samples and feature frames behind it are never read, codes behind it are
        -1 (the dropped code).  None: the rectangular call, exactly as before.  H-Codec 1.5 refuses `lengths=` here (its codes are a
        dict of [B, nq, G] tensors): `encode_ragged` / `decode_ragged` are its per-clip calls.  H-Codec 2.0 refuses `lengths=` here too,
        with status -4 and before any library call, although `encode_ragged` serves it through the very same entry point: that refusal
        is pinned by tests/test_hcodec_ragged_gpu.py::test_refusals_and_checks_come_before_any_launch, and a change that may edit that
        test can collapse the two doors."""
        if lengths is not None and self.spec.version == 20:
            raise _lib.QuarkAudioError(-4, "Codec.encode(lengths=...): on an H-Codec 2.0 model the per-clip calls are "
                                           "Codec.encode_ragged / Codec.decode_ragged")
        return self._encode(x, feat, threshold, lengths)

    def _encode(self, x, feat, threshold, lengths):
        """encode's body; lengths: code frames per clip (non-causal H-Codec 1.0 / 2.0: qa_hcodec_encode_ragged) or None."""
        self._require_loaded()
        if self.spec.version == 20 and x.dim() == 2:  # H-Codec 2.0 passes wav without the channel dim (audio_tokenizer.py:73)
            x = x.unsqueeze(1)
        if x.dim() != 3 or x.shape[1] != 1:
            raise _lib.QuarkAudioError(-1, f"encode expects x of shape [B,1,T], got {tuple(x.shape)}")
        if feat.dim() != 3 or feat.shape[0] != x.shape[0] or feat.shape[1] != self.spec.sem_in:
            raise _lib.QuarkAudioError(-1, f"encode expects feat of shape [B,{self.spec.sem_in},N], got {tuple(feat.shape)}")
        x = x.to(device=self.device, dtype=torch.float32).contiguous()
        feat = feat.to(device=self.device, dtype=torch.float32)
        B, _, T = x.shape
        n25 = T // self.spec.enc_hop
        q = self.spec.num_quantizers
        ac = torch.empty((B, q, n25), dtype=torch.int64, device=self.device)
        sc = torch.empty((B, q, n25), dtype=torch.int64, device=self.device)
        sb, sch, st = feat.stride()
        if lengths is not None:
            frames = _frames_arg(lengths, B)
            # (an H-Codec 1.5 handle is refused by the library with status -4, naming encode_ragged / decode_ragged)
            _lib.check(self._lib.qa_hcodec_encode_ragged(self._handle, x.data_ptr(), B, T, frames, feat.data_ptr(), sb, sch, st,
                                                         feat.shape[2], ac.data_ptr(), sc.data_ptr(), _stream_ptr(self.device)))
            return ac, sc
        if self.spec.adaptive:
            # codec_adaptive.py:150-178: dict of length-injected codes [B, nq, G]; G is data dependent (host sync, as in the
            # reference: modeling_flexicodec_new.py:910)
            assert 0 <= threshold <= 1.0  # codec_adaptive.py:151; 0 = the model's manual_threshold (:158)
            g = C.c_int64(0)
            _lib.check(self._lib.qa_hcodec_encode_adaptive(self._handle, x.data_ptr(), B, T, feat.data_ptr(), sb, sch, st,
                                                           feat.shape[2], ac.data_ptr(), sc.data_ptr(), C.byref(g),
                                                           float(threshold), _stream_ptr(self.device)))
            G = int(g.value)
            return {"acoustic_codes": ac.view(-1)[: B * q * G].view(B, q, G), "semantic_codes": sc.view(-1)[: B * q * G].view(B, q, G)}
        _lib.check(self._lib.qa_hcodec_encode(self._handle, x.data_ptr(), B, T, feat.data_ptr(), sb, sch, st,
                                              feat.shape[2], ac.data_ptr(), sc.data_ptr(), _stream_ptr(self.device)))
        return ac, sc

    @torch.no_grad()
    def decode(self, acoustic_codes: torch.Tensor, semantic_codes: torch.Tensor, token_lengths: Optional[torch.Tensor] = None, *,
               lengths=None):
        """codec.py:178-187.  int64 [B, nq, N25] x2 -> wav [B, N25 * 2 * hop].  H-Codec 1.5 (codec_adaptive.py:181-199):
        length-injected codes [B, nq, G] (or plain codes + token_lengths [B, G]).
        Codes: -1 = dropped (zero vector, as upstream's ResidualVQ masks it; 1.0 / 2.0 only - in the 1.5 wire format negative values carry
        the group lengths).  Any other value outside [0, codebook_size) raises IndexError like F.embedding - AFTER the decode has run on
        clamped indices (r04: the counter is read behind the decode's own host synchronisation, so the failing path costs a full decode;
        `check_codes=False` skips the check).

        lengths (keyword only; non-causal H-Codec 1.0): the clips' lengths in code frames, a host list / tensor of B values in 1 .. N.
        Row b then equals decode of its first lengths[b] frames alone; entries behind them are ignored whatever they hold (the range
        check does not count them), and the waveform is exactly zero from sample lengths[b] * 2 * hop on.  H-Codec 1.5 refuses `lengths=`
        here: its codes carry their lengths, and `decode_ragged` is its per-clip call.  H-Codec 2.0 refuses `lengths=` here as `encode`
        does (status -4, before any library call; pinned by the same test): `decode_ragged` is its per-clip call."""
        if lengths is not None and self.spec.version == 20:
            raise _lib.QuarkAudioError(-4, "Codec.decode(lengths=...): on an H-Codec 2.0 model the per-clip calls are "
                                           "Codec.encode_ragged / Codec.decode_ragged")
        self._require_loaded()
        if self.spec.adaptive and lengths is None:
            return self._decode_adaptive(acoustic_codes, semantic_codes, token_lengths)
        return self._decode(acoustic_codes, semantic_codes, lengths)

    def _decode(self, acoustic_codes, semantic_codes, lengths):
        """decode's body for H-Codec 1.0 / 2.0 codes; lengths: code frames per clip (qa_hcodec_decode_ragged) or None."""
        q = self.spec.num_quantizers
        if acoustic_codes.shape != semantic_codes.shape or acoustic_codes.dim() != 3 or acoustic_codes.shape[1] != q:
            raise _lib.QuarkAudioError(-1, f"decode expects two [B,{q},N] code tensors, got "
                                           f"{tuple(acoustic_codes.shape)} / {tuple(semantic_codes.shape)}")
        ac = acoustic_codes.to(device=self.device, dtype=torch.int64).contiguous()
        sc = semantic_codes.to(device=self.device, dtype=torch.int64).contiguous()
        B, _, N = ac.shape
        wav = torch.empty((B, N * self.spec.dec_upsample * self.spec.hop), dtype=torch.float32, device=self.device)
        if lengths is not None:
            frames = _frames_arg(lengths, B)
            pending = None
            if self.check_codes:  # the entries behind a clip's end are not codes: the check sees them as dropped
                fr = torch.tensor(list(frames), dtype=torch.int64, device=self.device)
                live = (torch.arange(N, device=self.device)[None, :] < fr[:, None])[:, None, :]
                pending = self._check_range_begin((torch.where(live, ac, -1), torch.where(live, sc, -1)), self.spec.codebook_size, lo=-1)
            _lib.check(self._lib.qa_hcodec_decode_ragged(self._handle, ac.data_ptr(), sc.data_ptr(), B, N, frames, wav.data_ptr(),
                                                         _stream_ptr(self.device)))
            self._check_range_end(pending)
            return wav
        # -1 is legal: a dropped code, masked to a zero vector by the third-party get_output_from_indices (INTEGRATION.md "Edge semantics")
        pending = self._check_range_begin((ac, sc), self.spec.codebook_size, lo=-1)
        _lib.check(self._lib.qa_hcodec_decode(self._handle, ac.data_ptr(), sc.data_ptr(), B, N, wav.data_ptr(),
                                              _stream_ptr(self.device)))
        self._check_range_end(pending)  # IndexError like the reference's F.embedding, raised behind the decode's own synchronisation
        return wav

    # -- per-clip lengths, every model ---------------------------------------------------------------
    @torch.no_grad()
    def encode_ragged(self, x: torch.Tensor, feat: torch.Tensor, lengths, threshold: float = 0.0):
        """One encode of clips of unequal length.  lengths: code frames per clip, a host list / tensor of B values in 1 .. N.

        H-Codec 1.5: {'acoustic_codes', 'semantic_codes'} as int64 [B, nq, G], G the largest group count of the
        batch.  Row b equals `encode` of clip b alone (B = 1) at its own length - its own alignment, its own group count, no padded query
        token among its keys, which the rectangular `encode` does not give even for clips of equal length.  Entries behind a clip's own
        groups are -1, a legal entry of length 0, so the dict is valid input for `decode` and `decode_ragged` alike.
        H-Codec 1.0: `encode(x, feat, lengths=lengths)`.
        H-Codec 2.0 (non-causal): two int64 [B, nq, N] tensors, row b the codes of clip b alone at its own length,
        -1 behind them; x is [B, T] or [B, 1, T] with T = 3840 N, feat [B, sem_in, 4 N].  This is the 2.0 model's only per-clip encode:
        `encode(lengths=...)` refuses it (see there)."""
        if not self.spec.adaptive:
            return self._encode(x, feat, 0.0, lengths)
        if x.dim() != 3 or x.shape[1] != 1:
            raise _lib.QuarkAudioError(-1, f"encode_ragged expects x of shape [B,1,T], got {tuple(x.shape)}")
        if feat.dim() != 3 or feat.shape[0] != x.shape[0] or feat.shape[1] != self.spec.sem_in:
            raise _lib.QuarkAudioError(-1, f"encode_ragged expects feat of shape [B,{self.spec.sem_in},N], got {tuple(feat.shape)}")
        if not 0 <= threshold <= 1.0:
            raise _lib.QuarkAudioError(-1, f"encode_ragged: threshold {threshold} outside [0, 1]")
        B, _, T = x.shape
        frames = _frames_arg(lengths, B)
        self._require_loaded()
        x = x.to(device=self.device, dtype=torch.float32).contiguous()
        feat = feat.to(device=self.device, dtype=torch.float32)
        n25 = T // self.spec.enc_hop
        q = self.spec.num_quantizers
        ac = torch.empty((B, q, max(n25, 1)), dtype=torch.int64, device=self.device)
        sc = torch.empty((B, q, max(n25, 1)), dtype=torch.int64, device=self.device)
        sb, sch, st = feat.stride()
        g = C.c_int64(0)
        _lib.check(self._lib.qa_hcodec_encode_adaptive_ragged(self._handle, x.data_ptr(), B, T, frames, feat.data_ptr(), sb, sch, st,
                                                              feat.shape[2], ac.data_ptr(), sc.data_ptr(), C.byref(g), float(threshold),
                                                              _stream_ptr(self.device)))
        G = int(g.value)
        return {"acoustic_codes": ac.view(-1)[: B * q * G].view(B, q, G), "semantic_codes": sc.view(-1)[: B * q * G].view(B, q, G)}

    # -- the causal acoustic encoder as a stream --------------------------------
    @property
    def is_streaming(self) -> bool:
        return self._streaming_batch > 0

    @property
    def streaming_offset(self) -> int:
        """Code frames streamed since `streaming()` / `reset_streaming()`; -1 when not streaming."""
        return int(self._lib.qa_hcodec_stream_offset(self._handle)) if self._handle.value else -1

    @property
    def stream_first_min_frames(self) -> int:
        """The fewest code frames the first chunk of a stream may have (2 for the shipped geometry): it pads its left edge with the
        reflection of its own frames, which equals the offline padding only from this length on.  Raises for a model that cannot stream."""
        spec_c = self.spec.to_c()
        first = C.c_int64(0)
        _lib.check(self._lib.qa_hcodec_stream_geometry(C.byref(spec_c), None, C.byref(first), None, 0, None))
        return int(first.value)

    def streaming_forever(self, batch_size: int, max_frames: int = _DEFAULT_STREAM_FRAMES, *, left_context: Optional[int] = None,
                          max_chunk: Optional[int] = None):
        """Enter streaming mode (causal H-Codec 1.0): `encode_stream(x)` is then one step on the next samples of `batch_size` rows.
        `max_frames` is the capacity in CODE frames (at most 4096, 163.84 s: the encoder's Transformer holds 8192 positions at two per code
        frame); a step that would pass it is refused and leaves the state as it was.  Offline `encode` / `decode` / `forward` stay
        allowed meanwhile: the stream's state is its own allocation.  On a codec that already streams, the old stream is freed.

        `left_context` and `max_chunk` (both or neither, and then no `max_frames`): a stream WITHOUT an end.  The
        encoder's Transformer runs under a sliding window of `left_context` Transformer frames (two per code frame) over a ring of K / V
        rows, and a step takes at most `max_chunk` code frames per row.  This is NOT the shipped full-causal model: it equals the SEANet
        encoder whose `Transformer` was built with `use_sliding_window=True, left_context=left_context` - a parameter the reference's block
        takes and `vq/codec.py` never sets - and its embeddings and codes differ from the full-causal ones by a few percent."""
        if (left_context is None) != (max_chunk is None):
            raise _lib.QuarkAudioError(-1, "Codec.streaming: left_context and max_chunk come together (a ring stream) or not at all")
        if max_chunk is not None and max_frames is not _DEFAULT_STREAM_FRAMES:
            raise _lib.QuarkAudioError(-1, "Codec.streaming: max_frames is the capacity of a linear stream and max_chunk that of a ring's "
                                           "steps - give one of them")
        self._require_loaded()
        with torch.cuda.device(self.device):
            if max_chunk is None:
                _lib.check(self._lib.qa_hcodec_stream_begin(self._handle, int(batch_size), int(max_frames)))
            else:
                _lib.check(self._lib.qa_hcodec_stream_begin_ring(self._handle, int(batch_size), int(left_context), int(max_chunk)))
        self._streaming_batch = int(batch_size)

    @property
    def streaming_capacity(self) -> int:
        """The code frames the stream's K / V rows hold: `max_frames` of a linear stream, the ring of a windowed one; -1 when not streaming."""
        return int(self._lib.qa_hcodec_stream_capacity(self._handle)) if self._handle.value else -1

    def _stop_streaming(self):
        if self._handle.value:
            _lib.check(self._lib.qa_hcodec_stream_end(self._handle))
        self._streaming_batch = 0

    @contextmanager
    def streaming(self, batch_size: int, max_frames: int = _DEFAULT_STREAM_FRAMES, *, left_context: Optional[int] = None,
                  max_chunk: Optional[int] = None):
        self.streaming_forever(batch_size, max_frames, left_context=left_context, max_chunk=max_chunk)
        try:
            yield
        finally:
            self._stop_streaming()

    @property
    def streaming_offsets(self):
        """The code frames of every row since `streaming()` / its own reset, a list of B ints (`streaming_offset` is the largest)."""
        if not self.is_streaming:
            raise _lib.QuarkAudioError(-1, "Codec.streaming_offsets: not streaming - call it inside `with codec.streaming(batch_size):`")
        out = (C.c_int64 * self._streaming_batch)()
        _lib.check(self._lib.qa_hcodec_stream_offsets(self._handle, out))
        return [int(v) for v in out]

    def reset_streaming(self, rows=None):
        """Back to offset 0: the next `encode_stream` is a first step again (reflect fill, LSTM state zeroed, earlier K / V rows invisible).
        `rows` (a list / tensor of distinct row indices): only those rows go back, all others continue."""
        self._require_loaded()
        if rows is None:
            _lib.check(self._lib.qa_hcodec_stream_reset(self._handle))
            return
        vals = _int_list(rows, "rows")
        _lib.check(self._lib.qa_hcodec_stream_reset_rows(self._handle, (C.c_int64 * max(len(vals), 1))(*vals), len(vals)))

    @torch.no_grad()
    def encode_stream(self, x: torch.Tensor, return_emb: bool = False, lengths=None):
        """The next chunk of every row of a stream: x [B, 1, n] or [B, n] fp32 with n a positive multiple of the samples of a code frame
        (`spec.enc_hop`, 640) -> acoustic codes int64 [B, nq, n / hop], in the layout of `encode`'s first output; with `return_emb` also the
        embeddings in front of the quantizer, emb [B, n / hop, code_dim].  Concatenated over the steps, both equal what one offline causal
        `encode` of the concatenated waveform gives.  The first chunk needs at least `stream_first_min_frames` code frames.  A trailing
        partial frame is the caller's to zero-pad, as `HCodecTokenizer.pad_wav` does - and only at the END of a stream: zeros in the middle
        are signal.  The semantic codes have no stream (their encoder is not causal and the SSL features are whole-utterance).
        `lengths`: a host list / tensor of B code-frame counts, row b consuming only its first lengths[b] frames of
        the rectangle at ITS OWN offset; 0 lets the row idle (state and offset untouched), a row at offset 0 needs at least
        `stream_first_min_frames`.  Samples behind a row's frames are never read; there the codes are -1 and emb is 0.  Each row's
        outputs, concatenated over its steps between two of its resets, equal the offline causal `encode` of its own waveform."""
        if not self.is_streaming:
            raise _lib.QuarkAudioError(-1, "Codec.encode_stream: not streaming - call it inside `with codec.streaming(batch_size):` "
                                           "(or use encode for a whole utterance)")
        if x.dim() == 3 and x.shape[1] == 1:
            x = x[:, 0]
        if x.dim() != 2:
            raise _lib.QuarkAudioError(-1, f"encode_stream expects x of shape [B,1,n] or [B,n], got {tuple(x.shape)}")
        if x.shape[0] != self._streaming_batch:
            raise _lib.QuarkAudioError(-1, f"streaming state was created for batch {self._streaming_batch}, got {x.shape[0]}")
        x = x.to(device=self.device, dtype=torch.float32).contiguous()
        B, n = x.shape
        # the library refuses a partial frame before it writes anything; max(.., 1): a chunk below one frame still gets its message
        frames = max(n // self.spec.enc_hop, 1)
        ac = torch.empty((B, self.spec.num_quantizers, frames), dtype=torch.int64, device=self.device)
        emb = torch.empty((B, frames, self.spec.code_dim), dtype=torch.float32, device=self.device) if return_emb else None
        with torch.cuda.device(self.device):
            if lengths is None:
                _lib.check(self._lib.qa_hcodec_stream_encode(self._handle, x.data_ptr(), n, ac.data_ptr(),
                                                             emb.data_ptr() if return_emb else None, _stream_ptr(self.device)))
            else:
                _lib.check(self._lib.qa_hcodec_stream_encode_rows(self._handle, x.data_ptr(), n, _frames_arg(lengths, B), ac.data_ptr(),
                                                                  emb.data_ptr() if return_emb else None, _stream_ptr(self.device)))
        return (ac, emb) if return_emb else ac

    def _adaptive_codes(self, acoustic_codes, semantic_codes, token_lengths, what: str):
        """The two code tensors of an H-Codec 1.5 decode on the device, length-injected (codec_adaptive.py:68-73)."""
        q, K = self.spec.num_quantizers, self.spec.codebook_size
        if acoustic_codes.shape != semantic_codes.shape or acoustic_codes.dim() != 3 or acoustic_codes.shape[1] != q:
            raise _lib.QuarkAudioError(-1, f"{what} expects two [B,{q},G] code tensors")
        ac = acoustic_codes.to(device=self.device, dtype=torch.int64).contiguous()
        sc = semantic_codes.to(device=self.device, dtype=torch.int64).contiguous()
        if token_lengths is not None:  # plain codes + explicit lengths: inject, exactly what encode emits
            tl = token_lengths.to(device=self.device, dtype=torch.int64).unsqueeze(1)
            ac, sc = (tl - 1) * K + ac, (tl - 1) * K + sc
        return ac, sc

    @torch.no_grad()
    def adaptive_frames(self, semantic_codes: torch.Tensor):
        """Code frames per clip of length-injected H-Codec 1.5 codes [B, nq, G]: the sum of the group lengths of every row, a list of B
        ints (one host synchronisation)."""
        if not self.spec.adaptive:
            raise _lib.QuarkAudioError(-4, "adaptive_frames: this is not an H-Codec 1.5 model")
        if semantic_codes.dim() != 3 or semantic_codes.shape[1] != self.spec.num_quantizers or semantic_codes.shape[2] < 1:
            raise _lib.QuarkAudioError(-1, f"adaptive_frames expects [B,{self.spec.num_quantizers},G] codes, got {tuple(semantic_codes.shape)}")
        self._require_loaded()
        sc = semantic_codes.to(device=self.device, dtype=torch.int64).contiguous()
        B, _, G = sc.shape
        out = (C.c_int64 * B)()
        _lib.check(self._lib.qa_hcodec_adaptive_clip_frames(self._handle, sc.data_ptr(), B, G, out, _stream_ptr(self.device)))
        return [int(v) for v in out]

    @torch.no_grad()
    def decode_ragged(self, acoustic_codes: torch.Tensor, semantic_codes: torch.Tensor, token_lengths: Optional[torch.Tensor] = None, *,
                      lengths=None):
        """One decode of clips of unequal length.

        H-Codec 1.5: length-injected codes [B, nq, G] (or plain codes + token_lengths [B, G]); the lengths ride in the codes, so
        `lengths` stays None.  Row b equals `decode` of clip b alone (B = 1): its bottleneck transformer and decoder see its own frames
        only.  Returns wav [B, max(frames) * 2 * hop], exactly zero behind every clip; a row whose codes hold no frame is an error.
        H-Codec 1.0: `decode(acoustic_codes, semantic_codes, lengths=lengths)`.
        H-Codec 2.0 (non-causal): codes [B, nq, N] and `lengths` in code frames -> wav [B, 3840 N]; row b is the
        decode of its first lengths[b] frames alone, entries behind them are ignored whatever they hold (the range check does not count
        them), and the waveform is exactly zero from sample 3840 * lengths[b] on.  `decode(lengths=...)` refuses a 2.0 model."""
        if not self.spec.adaptive:
            if token_lengths is not None:
                raise _lib.QuarkAudioError(-1, "decode_ragged: token_lengths belong to H-Codec 1.5 codes")
            self._require_loaded()
            return self._decode(acoustic_codes, semantic_codes, lengths)
        if lengths is not None:
            raise _lib.QuarkAudioError(-1, "decode_ragged: H-Codec 1.5 codes carry their lengths (adaptive_frames), pass none")
        q = self.spec.num_quantizers
        if acoustic_codes.shape != semantic_codes.shape or acoustic_codes.dim() != 3 or acoustic_codes.shape[1] != q:
            raise _lib.QuarkAudioError(-1, f"decode_ragged expects two [B,{q},G] code tensors")
        self._require_loaded()
        ac, sc = self._adaptive_codes(acoustic_codes, semantic_codes, token_lengths, "decode_ragged")
        B, _, G = ac.shape
        K = self.spec.codebook_size
        pending = self._check_range_begin((ac, sc), K * self.spec.max_tokens_per_group, lo=-K)
        per_clip = self.adaptive_frames(sc)
        self._check_range_end(pending)  # behind the frame counts' synchronisation, before any decode work
        for b, n in enumerate(per_clip):
            if n < 1:
                raise _lib.QuarkAudioError(-1, f"decode_ragged: frames[{b}] = {n}: the codes of row {b} hold no frame")
        n = max(per_clip)
        frames = (C.c_int64 * B)(*per_clip)
        wav = torch.empty((B, n * 2 * self.spec.hop), dtype=torch.float32, device=self.device)
        _lib.check(self._lib.qa_hcodec_decode_adaptive_ragged(self._handle, ac.data_ptr(), sc.data_ptr(), B, G, n, frames, wav.data_ptr(),
                                                              _stream_ptr(self.device)))
        return wav

    def enable_taps(self, on: bool = True):
        """Test hook: make encode/decode snapshot their named intermediates (see DESIGN.md "taps")."""
        self._require_loaded()
        _lib.check(self._lib.qa_hcodec_enable_taps(self._handle, int(on)))
        return self

    def _decode_adaptive(self, acoustic_codes, semantic_codes, token_lengths):
        K = self.spec.codebook_size
        ac, sc = self._adaptive_codes(acoustic_codes, semantic_codes, token_lengths, "decode")
        B, _, G = ac.shape
        # length-injected: code + (len - 1) * K with len in 0..max_tokens (len 0 = the padding groups of shorter clips: [-K, 0))
        pending = self._check_range_begin((ac, sc), K * self.spec.max_tokens_per_group, lo=-K)
        frames = C.c_int64(0)
        _lib.check(self._lib.qa_hcodec_adaptive_frames(self._handle, sc.data_ptr(), B, G, C.byref(frames), _stream_ptr(self.device)))
        self._check_range_end(pending)  # the frame count's read-back just synchronised the stream: the counter is there, before any decode work
        n = int(frames.value)
        wav = torch.empty((B, n * 2 * self.spec.hop), dtype=torch.float32, device=self.device)
        _lib.check(self._lib.qa_hcodec_decode_adaptive(self._handle, ac.data_ptr(), sc.data_ptr(), B, G, n, wav.data_ptr(),
                                                       _stream_ptr(self.device)))
        return wav

    def tap(self, name: str) -> torch.Tensor:
        """Test hook: flat fp32 copy of a named intermediate of the last encode/decode (channel-last layout)."""
        n = self._lib.qa_hcodec_tap(self._handle, name.encode(), None, 0, None)
        if n < 0:
            _lib.check(int(n))
        out = torch.empty(int(n), dtype=torch.float32, device=self.device)
        n2 = self._lib.qa_hcodec_tap(self._handle, name.encode(), out.data_ptr(), n, _stream_ptr(self.device))
        if n2 < 0:
            _lib.check(int(n2))
        return out


class HCodecTokenizer(torch.nn.Module):
    """Drop-in for the reference's three HCodecTokenizer classes, with their constructor signatures:

        HCodecTokenizer(pt_path)                                   H-Codec 1.0   HCodec-1.0/audio_tokenizer.py:18-33
        HCodecTokenizer(config=dict)   (config['ckpt_path'], ...)  H-Codec 1.5   HCodec-1.5/audio_tokenizer.py:38-51
        HCodecTokenizer(pt_path, config_path, device)              H-Codec 2.0   HCodec-2.0/audio_tokenizer.py:19-46

    plus keyword-only extras: `state_dict=` (instead of a checkpoint path), `spec=` (instead of a YAML config), `model=` (an already
    loaded `Codec`), `feature_extractor=`.  The reference downloads its SSL model (`AutoModel.from_pretrained`: hubert_base / XLSR-53); there is
    no network here, so the front-end is passed in: a `unified_audio_amd.SSLFeatureExtractor` (HuBERT / XLSR on the same HIP
    library - `tokenize(wav)` then never leaves the device path), or the reference's own PyTorch module
    (`feature_extractor(wav, output_hidden_states=True).hidden_states`), or precomputed features via `tokenize(wav, feats=...)`.
    Per version the tokenizer applies what the reference applies around it: mean of all hidden states (1.0, 2.0) or of states
    11 / 14 / 16 (1.5), |x|^0.3 compression, and for 2.0 the 48 kHz -> 16 kHz `Resample` in front (qa_resample).
    """

    def __init__(self, pt_path=None, config_path=None, device: str | torch.device = "cuda:0", *, config: Optional[dict] = None,
                 state_dict=None, feature_extractor: Optional[Callable] = None, spec: Optional[HCodecSpec] = None, model=None, **kwargs):
        super().__init__()
        self.config = config
        sampling_rate = 16000
        if config is None and config_path is not None:  # 2.0: YAML path
            import yaml

            with open(config_path, "r") as f:
                config = yaml.safe_load(f)
        if spec is None and config is not None:
            spec = _spec_from_config(config)
        if config is not None:
            sampling_rate = int(config.get("sampling_rate", 16000))
            if pt_path is None:
                pt_path = config.get("ckpt_path")  # 1.5: load_sub_weights(config['ckpt_path'], prefix=None)
        if spec is None and model is not None:
            spec = getattr(model, "spec", None)
        spec = spec or SPEC_10
        if spec.version == 20 and sampling_rate == 16000:
            sampling_rate = 48000  # large_12.5hz_config.yaml:1
        if model is not None:  # an already loaded Codec (or any object with its spec / encode / decode): nothing to read from disk
            self.device = torch.device(getattr(model, "device", device))
            self.model = model
        else:
            if state_dict is None:
                if pt_path is None:
                    raise ValueError("HCodecTokenizer needs pt_path, config['ckpt_path'] or state_dict")
                state_dict = torch.load(pt_path, map_location="cpu")  # audio_tokenizer.py:24
                if isinstance(state_dict, dict) and "state_dict" in state_dict:  # HCodec-1.5/audio_tokenizer.py:20-25
                    state_dict = state_dict["state_dict"]
            self.device = torch.device(device) if str(device) != "cpu" else torch.device("cuda:0")  # 2.0's default device='cpu': no CPU path
            self.model = Codec(None, None, None, spec=spec, device=self.device,
                               semantic_decoder_spec=_semantic_decoder_spec_from_config(config) if config is not None else None)
            ad = (config or {}).get("adaptive_config") or {}
            self.model.dynamic_threshold = bool(spec.adaptive and ad.get("infer_using_dynamic_threshold")
                                                and ad.get("manual_threshold") is None)
            self.model.load_state_dict(state_dict)
        self.feature_extractor = feature_extractor
        if isinstance(feature_extractor, torch.nn.Module):
            feature_extractor.eval()  # audio_tokenizer.py:28-29: the reference puts its SSL model in eval mode at construction
        self.sampling_rate = sampling_rate
        self.hop_length = spec.enc_hop  # 640 = 25 Hz (audio_tokenizer.py:31); 3840 = 12.5 Hz at 48 kHz (2.0 :46)
        # hidden states averaged by extract_wav2vec2_features when the extractor is the reference's own PyTorch module
        self.select_layers = (11, 14, 16) if spec.adaptive else None  # HCodec-1.5/audio_tokenizer.py:58-61

    def to(self, *args, **kwargs):
        self.model.to(*args, **kwargs)
        self.device = self.model.device
        fx = self.feature_extractor
        if fx is not None and hasattr(fx, "to"):
            self.feature_extractor = fx.to(self.device) or fx
        return self

    def train(self, mode: bool = True):
        """eval() must reach a PyTorch feature_extractor registered as a submodule (dropout / layerdrop of a HuBERT built in train
        mode); train(True) is refused like Codec's."""
        if mode:
            raise _lib.QuarkAudioError(-4, "unified_audio_amd.HCodecTokenizer is the inference path (the reference calls .eval())")
        return super().train(False)

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        """The tokenizer's weights are the codec's (audio_tokenizer.py:24-25 loads them into self.model): forward to it."""
        self.model.load_state_dict(state_dict)
        return self

    def resample(self, wavs: torch.Tensor, lengths=None) -> torch.Tensor:
        """torchaudio.transforms.Resample(sampling_rate, 16000) (HCodec-2.0/audio_tokenizer.py:44,51) on the device.
        lengths: the clips' lengths in samples at `sampling_rate` (host list / tensor): row b is then the resampled clip alone -
        `resampled_lengths(lengths)[b]` samples, exact zeros behind them, nothing behind wavs[b, :lengths[b]] read (qa_resample_ragged)."""
        if self.sampling_rate == 16000:
            return wavs
        x = wavs.to(device=self.device, dtype=torch.float32).contiguous()
        B, T = x.shape
        lib = self.model._lib
        n = int(lib.qa_resample_length(T, self.sampling_rate, 16000))
        out = torch.empty((B, n), dtype=torch.float32, device=self.device)
        if lengths is None:
            _lib.check(lib.qa_resample(x.data_ptr(), B, T, self.sampling_rate, 16000, out.data_ptr(), _stream_ptr(self.device)))
        else:
            _lib.check(lib.qa_resample_ragged(x.data_ptr(), B, T, _frames_arg(lengths, B), self.sampling_rate, 16000, out.data_ptr(),
                                              _stream_ptr(self.device)))
        return out

    def resampled_lengths(self, lengths):
        """Samples at 16 kHz of clips of `lengths` samples at `sampling_rate`: ceil(16000 * len / sampling_rate), as Resample cuts a
        clip alone.  A clip padded to its own code frames, f * 3840 samples at 48 kHz, gives f * 1280 samples: 4 f SSL frames."""
        g = math.gcd(self.sampling_rate, 16000)
        o, n = self.sampling_rate // g, 16000 // g
        return [-(-n * v // o) for v in _int_list(lengths, "lengths")]

    @torch.no_grad()
    def extract_wav2vec2_features(self, wavs: torch.Tensor, lengths=None) -> torch.Tensor:
        """1.0: audio_tokenizer.py:35-48 (pad (160,160), mean of all hidden states, sign*|x|^0.3); 1.5: hidden states 11 / 14 / 16
        (HCodec-1.5/audio_tokenizer.py:53-67); 2.0 (`extract_ssl_features`): Resample first (HCodec-2.0/audio_tokenizer.py:48-64).
        lengths (an SSLFeatureExtractor only, `_lengths_front_end`): the clips' lengths in samples at `sampling_rate`.  The 2.0 tokenizer
        resamples with them (`resample(wavs, lengths)`) and passes the 16 kHz lengths on; the others pass them on as they are."""
        if lengths is not None and not self._lengths_front_end():
            raise _lib.QuarkAudioError(-3, "per-clip lengths need an SSLFeatureExtractor as feature_extractor")
        if self.feature_extractor is None:
            raise _lib.QuarkAudioError(-3, "no feature_extractor was given; pass feats= to tokenize()")
        from .ssl import SSLFeatureExtractor

        if lengths is not None and not self._ragged_front_end():
            wavs, lengths = self.resample(wavs, lengths), self.resampled_lengths(lengths)
        else:
            wavs = self.resample(wavs)
        if isinstance(self.feature_extractor, SSLFeatureExtractor):  # padding, averaging and compression happen in the library
            fx = self.feature_extractor
            want = tuple(self.select_layers or ())
            have = tuple(fx.spec.select or ())
            if want != have:
                raise _lib.QuarkAudioError(-1, f"this tokenizer averages hidden states {want or 'all'} but the SSLFeatureExtractor was built "
                                               f"with select={have or 'all'} (H-Codec 1.5 needs SPEC_XLSR53, 1.0 / 2.0 SPEC_HUBERT_BASE)")
            return fx(wavs) if lengths is None else fx(wavs, lengths=lengths)
        wavs = torch.nn.functional.pad(wavs, (160, 160))
        feats = self.feature_extractor(wavs, output_hidden_states=True)
        hs = feats.hidden_states
        if self.select_layers is not None:
            feats_mix = sum(hs[i] for i in self.select_layers) / len(self.select_layers)
        else:
            feats_mix = torch.stack(hs, dim=1).mean(1)
        symbol = (feats_mix > 0).float() * 2 - 1
        return symbol * feats_mix.abs() ** 0.3

    extract_ssl_features = extract_wav2vec2_features  # the 2.0 tokenizer's name for it

    def _ragged_front_end(self) -> bool:
        """Whether the front-end takes per-clip lengths in one call (SSLFeatureExtractor.__call__(lengths=...)):
        the library's own extractor, fed the codec's waveform as it is.  Behind the 2.0 tokenizer's resampler see `_lengths_front_end`."""
        from .ssl import SSLFeatureExtractor

        return isinstance(self.feature_extractor, SSLFeatureExtractor) and self.sampling_rate == 16000

    def _lengths_front_end(self) -> bool:
        """Whether `extract_wav2vec2_features(wav, lengths=...)` is one front-end call: the library's own extractor, fed the waveform as it
        is (`_ragged_front_end`) or through the 2.0 tokenizer's resampler, which takes lengths too (qa_resample_ragged, DESIGN.md
        section 33)."""
        from .ssl import SSLFeatureExtractor

        return isinstance(self.feature_extractor, SSLFeatureExtractor)

    def pad_wav(self, wav: torch.Tensor) -> torch.Tensor:
        pad = math.ceil(wav.size(-1) / self.hop_length) * self.hop_length - wav.size(-1)
        return torch.nn.functional.pad(wav, (0, pad))

    def code_frames(self, lengths):
        """Code frames per clip for clip lengths in SAMPLES: ceil(len / hop) - what `tokenize(wav, lengths=...)` encodes and what
        `detokenize(..., lengths=...)` takes."""
        return code_frames(lengths, self.hop_length)

    @torch.no_grad()
    def _tokenize_ragged(self, wav: torch.Tensor, feats: Optional[torch.Tensor], lengths, threshold: float = 0.0):
        """tokenize with per-clip lengths in samples: wav [B, Tmax] holds clip b in wav[b, :lengths[b]].  Every clip is zero-padded to its
        own multiple of the hop, as pad_wav pads a clip alone; what lies behind that is never read."""
        hop = self.hop_length
        frames = self.code_frames(lengths)
        wav = wav.to(self.device)
        if wav.dim() != 2 or wav.shape[0] != len(frames):
            raise _lib.QuarkAudioError(-1, f"tokenize(lengths=...) expects wav [B, T] with B = {len(frames)}, got {tuple(wav.shape)}")
        lens = _int_list(lengths, "lengths")
        if max(lens) > wav.shape[1]:
            raise _lib.QuarkAudioError(-1, f"lengths: a clip of {max(lens)} samples does not fit wav [B, {wav.shape[1]}]")
        wav = self.pad_wav(wav)
        n = wav.shape[1] // hop
        pos = torch.arange(wav.shape[1], device=self.device)[None, :]
        ln = torch.tensor(lens, device=self.device)[:, None]
        end = torch.tensor(frames, device=self.device)[:, None] * hop
        wav = wav.masked_fill((pos >= ln) & (pos < end), 0.0)  # pad_wav of each clip alone: zeros up to its own hop multiple
        if feats is None and self._lengths_front_end():
            # ONE front-end call: row b is the clip padded to its own hop multiple, alone (its own padding, normalisation and keys)
            fpc = int(math.prod(self.model.spec.sem_strides))
            part = self.extract_wav2vec2_features(wav, lengths=[f * hop for f in frames])  # (b, t, d), zeros behind every clip's frames
            hop16 = hop if self.sampling_rate == 16000 else self.resampled_lengths([hop])[0]  # the front-end's samples per code frame
            short = [f for f in set(frames) if self.feature_extractor.frames(f * hop16) < fpc * f]
            if part.shape[1] < fpc * n or short:
                raise _lib.QuarkAudioError(-1, f"the feature extractor returned {part.shape[1]} frames for {n} code frames, need {fpc * n}")
            feats = part[:, : fpc * n]
        elif feats is None:
            # a front-end that takes no lengths (it is not causal): one pass per distinct padded length, scattered into one batch
            fpc = int(math.prod(self.model.spec.sem_strides))
            out = None
            for f in sorted(set(frames)):
                rows = [b for b, fb in enumerate(frames) if fb == f]
                part = self.extract_wav2vec2_features(wav[rows, : f * hop].contiguous())  # (b, t, d)
                if part.shape[1] < fpc * f:
                    raise _lib.QuarkAudioError(-1, f"the feature extractor returned {part.shape[1]} frames for {f} code frames, need {fpc * f}")
                if out is None:
                    out = torch.zeros((len(frames), fpc * n, part.shape[2]), dtype=torch.float32, device=self.device)
                out[rows, : fpc * f] = part[:, : fpc * f].to(device=self.device, dtype=torch.float32)
            feats = out
        feats = feats.to(self.device).transpose(-2, -1)
        if self.model.spec.adaptive:  # H-Codec 1.5: the dict of [B, nq, G] codes, -1 behind every clip's own groups
            return self.model.encode_ragged(wav.unsqueeze(1), feats, frames, threshold=threshold)
        if self.model.spec.version == 20:  # its per-clip door; 2.0 passes wav without the channel dim (audio_tokenizer.py:73)
            return self.model.encode_ragged(wav, feats, frames)
        return self.model.encode(wav.unsqueeze(1), feats, lengths=frames)

    @torch.no_grad()
    def tokenize(self, wav: torch.Tensor, feats: Optional[torch.Tensor] = None, threshold: float = 0.0, lengths=None):
        """lengths (non-causal H-Codec 1.0 / 1.5 / 2.0): the clips' lengths in SAMPLES (host list / tensor), wav [B, Tmax] with clip b in
        its first lengths[b] samples.  Codes of clip b then equal tokenize of that clip alone; `code_frames(lengths)` gives the frames per
        clip.  1.0 / 2.0: entries behind them are -1.  1.5: the dict of `Codec.encode_ragged`.  feats, when given, are [B, t, d] with clip
        b's frames first, and no front-end is touched; without them the 2.0 tokenizer resamples with the lengths (`resample`) in front of
        an SSLFeatureExtractor that takes the 16 kHz lengths: one front-end call."""
        if lengths is not None:
            return self._tokenize_ragged(wav, feats, lengths, threshold)
        wav = self.pad_wav(wav.to(self.device))
        if feats is None:
            feats = self.extract_wav2vec2_features(wav)  # (b, t, d)
        feats = feats.to(self.device).transpose(-2, -1)  # (b, d, t) view; the library reads it through its strides
        if self.model.spec.adaptive:
            return self.model.encode(wav.unsqueeze(1), feats, threshold=threshold)
        return self.model.encode(wav.unsqueeze(1), feats)

    @torch.no_grad()
    def detokenize(self, acoustic_codes: torch.Tensor, semantic_codes: torch.Tensor, token_lengths=None, lengths=None, ragged: bool = False):
        """1.0: audio_tokenizer.py:64-66; 1.5: HCodec-1.5/audio_tokenizer.py:83-86 (call as detokenize(**codes)).  lengths: the clips'
        lengths in CODE frames (`code_frames`), passed on to `Codec.decode`.  ragged=True: `Codec.decode_ragged` - for H-Codec 1.5 codes
        of `tokenize(..., lengths=...)`, whose lengths ride in the codes."""
        if ragged:
            return self.model.decode_ragged(acoustic_codes, semantic_codes, token_lengths, lengths=lengths)
        if lengths is not None and self.model.spec.version == 20:  # the 2.0 model's per-clip door
            return self.model.decode_ragged(acoustic_codes, semantic_codes, lengths=lengths)
        if lengths is not None:
            return self.model.decode(acoustic_codes, semantic_codes, lengths=lengths)
        if self.model.spec.adaptive:
            return self.model.decode(acoustic_codes, semantic_codes, token_lengths)
        return self.model.decode(acoustic_codes, semantic_codes)
