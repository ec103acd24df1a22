"""Python mirror of the codec's own Transformer block, backed by libquarkaudio_hip.so.

    Transformer.forward(inputs_embeds, past_key_values=None, use_cache=None)
        <->  QuarkAudio-HCodec/HCodec-1.0/vq/encoder_modules/transformer.py:396-489
    Transformer.streaming(B, max_frames=...) / .streaming_forever / .reset_streaming / .is_streaming / .streaming_offset
        -    no counterpart: the reference restarts its LSTM on every call (:133) and cannot combine its (T, T) mask with cached keys
             (:469-475), so it cannot stream this block; the causal graph can be streamed exactly, and this class does

Inside `Codec` the same block runs as part of encode / decode; this class exposes one stack on its own.  `prefix="encoder.model.14"` or
`"decoder.prior_net.3"` loads it out of an H-Codec 1.0 checkpoint.
"""
from __future__ import annotations

import ctypes as C
from contextlib import contextmanager
from typing import Dict, Optional

import torch

from . import _lib
from .hcodec import _DefaultInt, _frames_arg, _int_list

MAX_FRAMES = 8192  # the library's RoPE table: the most frames a cache or a linear stream can hold
_DEFAULT_FRAMES = _DefaultInt(MAX_FRAMES)


class TransformerCache:
    """past_key_values of `Transformer.forward(..., use_cache=True)`: per layer the roped K and V rows, owned by the library."""

    def __init__(self, model: "Transformer", batch_size: int, capacity: int):
        self._lib = model._lib
        self._handle = C.c_void_p()
        self.batch_size, self.capacity = int(batch_size), int(capacity)
        with torch.cuda.device(model.device):
            _lib.check(self._lib.qa_transformer_cache_create(model._handle, self.batch_size, self.capacity, C.byref(self._handle)))

    def get_seq_length(self) -> int:
        return int(self._lib.qa_transformer_cache_length(self._handle)) if self._handle else 0

    def reset(self) -> None:
        if not self._handle:
            raise _lib.QuarkAudioError(-1, "TransformerCache: the cache was freed")
        _lib.check(self._lib.qa_transformer_cache_reset(self._handle))

    def free(self) -> None:
        if getattr(self, "_handle", None):
            self._lib.qa_transformer_cache_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Transformer(torch.nn.Module):
    def __init__(self, hidden_size: int, intermediate_size: int, num_attention_heads: int, num_hidden_layers: int,
                 head_dim: Optional[int] = None, attention_dropout: float = 0.0, use_moe: bool = False,
                 max_position_embeddings: int = 4096, causal: bool = False, use_sliding_window: bool = False, left_context: int = 0, *,
                 device="cuda:0", prefix: str = ""):
        super().__init__()
        if use_moe:
            raise _lib.QuarkAudioError(-3, "Transformer: use_moe=True is not implemented (no H-Codec configuration uses it)")
        if head_dim is not None and head_dim != hidden_size // num_attention_heads:
            raise _lib.QuarkAudioError(-3, f"Transformer: head_dim {head_dim} != hidden_size / num_attention_heads is not implemented")
        if causal and use_sliding_window and left_context < 1:
            raise _lib.QuarkAudioError(-3, "Transformer: use_sliding_window needs left_context >= 1 (the reference's mask hides every key at 0)")
        self.hidden_size, self.intermediate_size = int(hidden_size), int(intermediate_size)
        self.num_attention_heads, self.num_hidden_layers = int(num_attention_heads), int(num_hidden_layers)
        self.attention_dropout, self.max_position_embeddings = attention_dropout, int(max_position_embeddings)  # inference: unused
        self.causal, self.use_sliding_window, self.left_context = bool(causal), bool(use_sliding_window), int(left_context)
        self.device = torch.device(device)
        self._prefix = prefix
        self._lib = _lib.load_library()
        self._handle: Optional[C.c_void_p] = None
        self._sd: Optional[Dict[str, torch.Tensor]] = None
        self._streaming_batch = 0

    # ---- weights
    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        _lib.require_device()
        self._free()
        p = self._prefix + "." if self._prefix else ""
        sd = {"t." + k[len(p):]: v for k, v in state_dict.items() if k.startswith(p)}
        table, n, keep = _lib.tensor_table(sd)
        # the reference builds its sliding-window mask only when causal and use_sliding_window are both set (transformer.py:470-474)
        window = self.left_context if (self.causal and self.use_sliding_window) else 0
        spec = _lib.qa_transformer_spec(self.hidden_size, self.intermediate_size, self.num_attention_heads, self.num_hidden_layers,
                                        int(self.causal), int(window))
        handle = C.c_void_p()
        _lib.check(self._lib.qa_transformer_create(C.byref(handle), C.byref(spec), table, n, b"t", self.device.index or 0))
        self._handle = handle
        self._sd = {k[2:]: v for k, v in sd.items()}
        return self

    def state_dict(self, *args, destination=None, prefix: str = "", keep_vars: bool = False):
        out = destination if destination is not None else {}
        for k, v in (self._sd or {}).items():
            out[prefix + k] = v
        return out

    def _free(self):
        if getattr(self, "_handle", None):
            self._lib.qa_transformer_destroy(self._handle)
            self._handle = None
        self._streaming_batch = 0

    def __del__(self):
        try:
            self._free()
        except Exception:
            pass

    def _require(self):
        if not self._handle:
            raise _lib.QuarkAudioError(-1, "Transformer: no weights loaded (call load_state_dict first)")

    # ---- streaming
    @property
    def is_streaming(self) -> bool:
        return self._streaming_batch > 0

    def streaming_forever(self, batch_size: int, max_frames: int = _DEFAULT_FRAMES, *, max_chunk: Optional[int] = None):
        """Enter streaming mode: `forward(x)` is then one step on the next x.shape[1] frames.  `max_frames` is the capacity of the K / V
        rows the stream keeps (at most 8192); a step that would pass it is refused and leaves the state as it was.
        `max_chunk` (in place of `max_frames`; needs causal, use_sliding_window and left_context): the K / V rows are a
        ring of `streaming_capacity` >= left_context + max_chunk rows and the stream has no end - a step takes at most `max_chunk` frames
        per row, at any offset below 2^24 frames."""
        if max_chunk is not None and max_frames is not _DEFAULT_FRAMES:
            raise _lib.QuarkAudioError(-1, "Transformer.streaming: max_frames is the capacity of a linear stream and max_chunk that of a "
                                           "ring's steps - give one of them")
        self._require()
        with torch.cuda.device(self.device):
            if max_chunk is None:
                _lib.check(self._lib.qa_transformer_stream_begin(self._handle, int(batch_size), int(max_frames)))
            else:
                _lib.check(self._lib.qa_transformer_stream_begin_ring(self._handle, int(batch_size), int(max_chunk)))
        self._streaming_batch = int(batch_size)

    @property
    def streaming_capacity(self) -> int:
        """The rows of the stream's K / V cache: `max_frames` of a linear stream, the ring of one begun with `max_chunk`; -1 when not
        streaming."""
        return int(self._lib.qa_transformer_stream_capacity(self._handle)) if self._handle else -1

    def _stop_streaming(self):
        if self._handle:
            _lib.check(self._lib.qa_transformer_stream_end(self._handle))
        self._streaming_batch = 0

    @contextmanager
    def streaming(self, batch_size: int, max_frames: int = _DEFAULT_FRAMES, *, max_chunk: Optional[int] = None):
        self.streaming_forever(batch_size, max_frames, max_chunk=max_chunk)
        try:
            yield
        finally:
            self._stop_streaming()

    def reset_streaming(self, rows=None):
        """Back to offset 0.  `rows` (a list / tensor of distinct row indices): only those rows, all others continue."""
        self._require()
        if rows is None:
            _lib.check(self._lib.qa_transformer_stream_reset(self._handle))
            return
        vals = _int_list(rows, "rows")
        _lib.check(self._lib.qa_transformer_stream_reset_rows(self._handle, (C.c_int64 * max(len(vals), 1))(*vals), len(vals)))

    @property
    def streaming_offsets(self):
        """The frames of every row since `streaming()` / its own reset, a list of B ints (`streaming_offset` is the largest)."""
        if not self.is_streaming:
            raise _lib.QuarkAudioError(-1, "Transformer.streaming_offsets: not streaming")
        out = (C.c_int64 * self._streaming_batch)()
        _lib.check(self._lib.qa_transformer_stream_offsets(self._handle, out))
        return [int(v) for v in out]

    @property
    def streaming_offset(self) -> int:
        return int(self._lib.qa_transformer_stream_offset(self._handle)) if self._handle else -1

    # ---- forward
    def new_cache(self, batch_size: int, capacity: Optional[int] = None) -> TransformerCache:
        """An empty cache for `batch_size` sequences; capacity defaults to max_position_embeddings (at most 8192 frames)."""
        self._require()
        return TransformerCache(self, batch_size, min(self.max_position_embeddings, MAX_FRAMES) if capacity is None else capacity)

    @torch.no_grad()
    def forward(self, inputs_embeds: torch.Tensor, past_key_values: Optional[TransformerCache] = None, use_cache: Optional[bool] = None,
                lengths=None):
        """`lengths` (streaming only): a host list / tensor of B frame counts - row b consumes its first lengths[b]
        frames of the rectangle at its own offset (0: the row idles); the output behind them is 0."""
        self._require()
        if lengths is not None and not self.is_streaming:
            raise _lib.QuarkAudioError(-1, "Transformer: lengths= belongs to a streaming step (inside streaming())")
        x = inputs_embeds
        if x.dim() != 3 or x.shape[-1] != self.hidden_size:
            raise _lib.QuarkAudioError(-1, f"Transformer expects [B, T, {self.hidden_size}], got {tuple(x.shape)}")
        x = x.to(device=self.device, dtype=torch.float32).contiguous()
        y = torch.empty_like(x)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        B, T, _ = x.shape
        with torch.cuda.device(self.device):
            if self.is_streaming:
                if past_key_values is not None or use_cache:
                    raise _lib.QuarkAudioError(-1, "Transformer: inside streaming() the stream owns the K / V rows; past_key_values / "
                                                   "use_cache belong to the non-streaming forward")
                if B != self._streaming_batch:
                    raise _lib.QuarkAudioError(-1, f"streaming state was created for batch {self._streaming_batch}, got {B}")
                if lengths is None:
                    _lib.check(self._lib.qa_transformer_stream_step(self._handle, x.data_ptr(), T, y.data_ptr(), stream))
                else:
                    _lib.check(self._lib.qa_transformer_stream_step_rows(self._handle, x.data_ptr(), T, _frames_arg(lengths, B), y.data_ptr(),
                                                                         stream))
                return y
            if use_cache and past_key_values is None:  # transformer.py:456-457
                past_key_values = self.new_cache(B)
            if past_key_values is None:
                _lib.check(self._lib.qa_transformer_forward(self._handle, x.data_ptr(), B, T, y.data_ptr(), stream))
                return y
            if not isinstance(past_key_values, TransformerCache) or not past_key_values._handle:
                raise _lib.QuarkAudioError(-1, "Transformer: past_key_values must be a live TransformerCache (Transformer.new_cache)")
            _lib.check(self._lib.qa_transformer_forward_cached(self._handle, past_key_values._handle, x.data_ptr(), B, T, y.data_ptr(), stream))
        return (y, past_key_values) if use_cache else y
