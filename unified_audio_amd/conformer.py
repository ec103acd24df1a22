"""Python mirror of the reference's Conformer condition encoder, backed by libquarkaudio_hip.so.

    ConformerEncoder  <->  QuarkAudio-UniSE/model/llm/conformer.py:447-484 (eval mode)
    ConditionEncoder  <->  cond_input_layer -> cond_encoder -> cond_output_layer of CustomLlamaModel (model/llm/llm.py:52-54,130-132)

The rotary embedding comes from the third-party `x_transformers` package in the reference (conformer.py:17).  `rope_interleaved`
selects how channels are paired: True rotates adjacent channels (2i, 2i + 1), False rotates (i, i + dim_head / 2); see INTEGRATION.md.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import torch

from . import _lib


class _CondHandle:
    """Shared plumbing of the two classes: one qa_cond_encoder handle."""

    _prefixes: tuple = ()

    def _init(self, spec: _lib.qa_cond_encoder_spec, device):
        self.device = torch.device(device)
        self._spec = spec
        self._lib = _lib.load_library()
        self._handle = C.c_void_p()

    def load_state_dict(self, state_dict: Dict[str, torch.Tensor], strict: bool = True):
        """`strict` exists for nn.Module's signature only: loading is always strict - a missing key, or a key under the module's
        prefixes that the model does not have, raises (qa_cond_encoder_create names it)."""
        _lib.require_device()
        sd = {(k[4:] if k.startswith("dnn.") else k): v for k, v in state_dict.items()}
        sd = {k: v for k, v in sd.items() if k.startswith(self._prefixes)}
        self._free()
        table, n, keep = _lib.tensor_table(sd)
        handle = C.c_void_p()
        _lib.check(self._lib.qa_cond_encoder_create(C.byref(handle), C.byref(self._spec), table, n, self.device.index or 0))
        del keep
        self._handle = handle
        return self

    def eval(self):
        return self

    def _free(self):
        if getattr(self, "_handle", None) is not None and self._handle.value:
            self._lib.qa_cond_encoder_destroy(self._handle)
            self._handle = C.c_void_p()

    def __del__(self):
        try:
            self._free()
        except Exception:
            pass

    def _run(self, fn, fn_ragged, x: torch.Tensor, mask: Optional[torch.Tensor], lengths, width_in: int, width_out: int) -> torch.Tensor:
        if not self._handle.value:
            raise _lib.QuarkAudioError(-3, f"{type(self).__name__} has no weights: call load_state_dict first")
        x = x.to(device=self.device, dtype=torch.float32).contiguous()
        if x.dim() != 3 or x.shape[-1] != width_in:
            raise _lib.QuarkAudioError(-1, f"input must be [B, T, {width_in}], got {tuple(x.shape)}")
        B, T, _ = x.shape
        if mask is not None and lengths is not None:
            raise _lib.QuarkAudioError(-1, "mask and lengths are two different functions (the mask never reaches the convolution module): "
                                           "pass one of them")
        _, lens = _lib.host_lengths("lengths", lengths, B)
        m = None
        if mask is not None:
            m = mask.to(device=self.device, dtype=torch.bool).contiguous()
            if tuple(m.shape) != (B, T):
                raise _lib.QuarkAudioError(-1, f"mask must be bool [B={B}, T={T}], got {tuple(m.shape)}")
        y = torch.empty((B, T, width_out), dtype=torch.float32, device=self.device)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        if lens is not None:
            _lib.check(fn_ragged(self._handle, x.data_ptr(), lens, B, T, y.data_ptr(), stream))
            return y
        _lib.check(fn(self._handle, x.data_ptr(), m.data_ptr() if m is not None else None, B, T, y.data_ptr(), stream))
        return y

    def __call__(self, *args, **kwargs):
        return self.forward(*args, **kwargs)

    def enable_taps(self, on: bool = True):
        """Test hook: record conformer.N.{ff1, attn, conv, out} of the next forward (qa_cond_encoder_enable_taps)."""
        _lib.check(self._lib.qa_cond_encoder_enable_taps(self._handle, int(on)))
        return self

    def tap(self, name: str) -> torch.Tensor:
        n = self._lib.qa_cond_encoder_tap(self._handle, name.encode(), None, 0, None)
        if n < 0:
            _lib.check(int(n))
        out = torch.empty(int(n), dtype=torch.float32, device=self.device)
        n2 = self._lib.qa_cond_encoder_tap(self._handle, name.encode(), out.data_ptr(), n, torch.cuda.current_stream(self.device).cuda_stream)
        if n2 < 0:
            _lib.check(int(n2))
        return out


def _spec(cond_dim, hidden_out, num_layers, dim, heads, dim_head, depthwise_conv_kernel_size, ff_mult, qk_norm, pe_attn_head,
          rope_interleaved) -> _lib.qa_cond_encoder_spec:
    if qk_norm not in (None, "rms_norm"):
        raise ValueError(f"Unimplemented qk_norm: {qk_norm}")  # conformer.py:83
    return _lib.qa_cond_encoder_spec(int(cond_dim), int(dim), int(num_layers), int(heads), int(dim_head), int(depthwise_conv_kernel_size),
                                     int(ff_mult), -1 if pe_attn_head is None else int(pe_attn_head), 1 if rope_interleaved else 0,
                                     int(hidden_out), 0 if qk_norm is None else 1)


class ConformerEncoder(_CondHandle):
    """conformer.py:447-484.  `dropout` is accepted for signature parity (eval mode).  Weights: `layers.N.*` (an optional
    `cond_encoder.` / `dnn.cond_encoder.` prefix is stripped)."""

    _prefixes = ("layers.",)

    def __init__(self, num_layers, dim, heads, dim_head, depthwise_conv_kernel_size=31, ff_mult=4, dropout=0.1, qk_norm=None,
                 pe_attn_head=None, *, rope_interleaved: bool = True, device: str | torch.device = "cuda:0"):
        self.dim = int(dim)
        self._init(_spec(0, 0, num_layers, dim, heads, dim_head, depthwise_conv_kernel_size, ff_mult, qk_norm, pe_attn_head,
                         rope_interleaved), device)

    def load_state_dict(self, state_dict, strict: bool = True):
        sd = {(k[4:] if k.startswith("dnn.") else k): v for k, v in state_dict.items()}
        if any(k.startswith("cond_encoder.") for k in sd):  # a whole LM state_dict: its own `layers.N.*` are the Llama body's
            sd = {k[len("cond_encoder."):]: v for k, v in sd.items() if k.startswith("cond_encoder.")}
        return super().load_state_dict(sd, strict)

    @torch.no_grad()
    def forward(self, x: torch.Tensor, mask: Optional[torch.Tensor] = None, *, lengths=None) -> torch.Tensor:
        """x [B, T, dim], mask bool [B, T] (True = valid) or None -> [B, T, dim].

        lengths (keyword only; B frame counts in 1 .. T): row b comes out as forward(x[b:b+1, :lengths[b]]) alone, exact zeros behind, and
        what x holds behind a row's length is never used.  This is NOT the mask: the reference's mask hides padded keys but never reaches
        the convolution module, whose k = 31 window then pulls padded frames into a row's last 15 valid ones.  One of the two at most."""
        return self._run(self._lib.qa_conformer_forward, self._lib.qa_conformer_forward_ragged, x, mask, lengths, self.dim, self.dim)


class ConditionEncoder(_CondHandle):
    """cond_output_layer(cond_encoder(cond_input_layer(cond))) of CustomLlamaModel (llm.py:130-132)."""

    _prefixes = ("cond_input_layer.", "cond_encoder.", "cond_output_layer.")

    def __init__(self, cond_dim: int, hidden_size: int, conformer_params: dict, *, rope_interleaved: bool = True,
                 device: str | torch.device = "cuda:0"):
        p = dict(conformer_params)
        self.cond_dim, self.hidden_size = int(cond_dim), int(hidden_size)
        self._init(_spec(cond_dim, hidden_size, p["num_layers"], p["dim"], p["heads"], p["dim_head"],
                         p.get("depthwise_conv_kernel_size", 31), p.get("ff_mult", 4), p.get("qk_norm"), p.get("pe_attn_head"),
                         rope_interleaved), device)

    @torch.no_grad()
    def forward(self, cond: torch.Tensor, mask: Optional[torch.Tensor] = None, *, lengths=None) -> torch.Tensor:
        """cond [B, T, cond_dim] (log-mel) -> [B, T, hidden_size]; `lengths` as ConformerEncoder.forward (zeros behind a row's length)"""
        return self._run(self._lib.qa_cond_encoder_forward, self._lib.qa_cond_encoder_forward_ragged, cond, mask, lengths, self.cond_dim,
                         self.hidden_size)
