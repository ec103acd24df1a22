"""Python mirror of the reference's UniSE AR-LM interface, backed by libquarkaudio_hip.so.

    LLM_SFT.generate  <->  QuarkAudio-UniSE/model/llm/llm_sft.py:93-195   (greedy path: model/model.py:173)
    LLM_SFT.forward   <->  QuarkAudio-UniSE/model/llm/llm_sft.py:37-90    (teacher-forced loss / accuracy: Model.validation_step)
    CustomLlamaModel  <->  QuarkAudio-UniSE/model/llm/llm.py:13-374       (the pre-training-stage model: condition encoder prompt or none)

Weights come in the reference's key layout (the Lightning checkpoint's `dnn.*` entries, prefix optional).
"""
from __future__ import annotations

import ctypes as C
import weakref
from types import SimpleNamespace
from typing import Dict, Optional, Sequence

import torch

from . import _lib

DEFAULT_TASK_MAP = {"se": 0, "tse": 1, "rtse": 2}  # conf/config.yaml:132-136


MAX_POSITION_EMBEDDINGS = 4096  # conf/config.yaml:146


class KVCache:
    """A key / value cache held across llm_forward calls (qa_lm_cache): what transformers' DynamicCache is to the reference's
    llm_forward, with a fixed capacity.  Device memory of its own; its batch and its rows' lengths are host state (every row has a
    length of its own: llm_forward(..., chunk_lengths=)).  Freed with this object, or with the model's handle, whichever goes first."""

    def __init__(self, lm, max_batch: int, max_len: int = MAX_POSITION_EMBEDDINGS):
        self._lm = lm._lm if isinstance(lm, CustomLlamaModel) else lm
        if not self._lm._handle.value:
            raise _lib.QuarkAudioError(-3, "KVCache: the model has no weights: call load_state_dict first")
        self._lib = self._lm._lib
        self._handle = C.c_void_p()
        _lib.check(self._lib.qa_lm_cache_create(self._lm._handle, int(max_batch), int(max_len), C.byref(self._handle)))
        self.max_batch, self.max_len = int(max_batch), int(max_len)
        self._lm._caches.add(self)

    def _ptr(self):
        if self._handle is None or not self._handle.value:
            raise _lib.QuarkAudioError(-1, "KVCache: the cache was freed (with its model's handle, or by free())")
        return self._handle

    def free(self):
        if getattr(self, "_handle", None) is not None and self._handle.value:
            self._lib.qa_lm_cache_destroy(self._handle)
        self._handle = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    def _stream(self):
        return torch.cuda.current_stream(self._lm.device).cuda_stream

    def get_seq_length(self) -> int:
        """Positions held; on a cache whose rows differ in length, the longest row's."""
        return int(self._lib.qa_lm_cache_length(self._ptr()))

    def get_seq_lengths(self) -> list:
        """Positions held by every row: batch_size ints."""
        arr = (C.c_int64 * max(self.batch_size, 1))()
        _lib.check(self._lib.qa_lm_cache_lengths(self._ptr(), arr))
        return [int(v) for v in arr[:self.batch_size]]

    def crop_rows(self, lengths: Sequence[int]):
        """Keep the first lengths[b] positions of row b (0 <= lengths[b] <= the row's length); batch_size ints."""
        lens = [int(v) for v in (lengths.tolist() if torch.is_tensor(lengths) else lengths)]
        if len(lens) != self.batch_size:
            raise _lib.QuarkAudioError(-1, f"KVCache.crop_rows: {len(lens)} lengths for a cache of {self.batch_size} rows")
        _lib.check(self._lib.qa_lm_cache_crop_rows(self._ptr(), (C.c_int64 * max(len(lens), 1))(*lens)))

    @property
    def batch_size(self) -> int:
        return int(self._lib.qa_lm_cache_batch(self._ptr()))

    def reset(self):
        _lib.check(self._lib.qa_lm_cache_reset(self._ptr()))

    def crop(self, max_length: int):
        """DynamicCache.crop: keep the first `max_length` positions (negative: drop that many from the end of the longest row); rows
        that are shorter already keep their length."""
        n = int(max_length)
        if n < 0:
            n = self.get_seq_length() + n
        _lib.check(self._lib.qa_lm_cache_crop(self._ptr(), n))

    def batch_select_indices(self, indices: Sequence[int]):
        """Row j becomes old row indices[j]; the batch becomes len(indices) (at most max_batch)."""
        idx = [int(i) for i in (indices.tolist() if torch.is_tensor(indices) else indices)]
        arr = (C.c_int64 * len(idx))(*idx)
        _lib.check(self._lib.qa_lm_cache_select(self._ptr(), arr, len(idx), self._stream()))

    def reorder_cache(self, beam_idx):
        self.batch_select_indices(beam_idx)

    def batch_repeat_interleave(self, repeats: int):
        self.batch_select_indices([b for b in range(self.batch_size) for _ in range(int(repeats))])


def _unsupported(**kw):
    for name, (value, default) in kw.items():
        if value is not default and value != default:
            raise _lib.QuarkAudioError(-4, f"llm_forward: {name} is not supported (attention is causal over the cache, positions follow "
                                           f"the cache length, attention weights are never materialised)")


def _call_seed(do_sample: bool):
    """(seed,) of a sampled call, () of a greedy one: the seed advances torch's CPU generator, once per call"""
    return (int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item()),) if do_sample else ()


def _generate_call(lib, family: str, lengths_arr, do_sample: bool):
    """The C function of a generate call - `family` (qa_lm_generate / qa_lm_generate_cond), _ragged with a per-row length array, _sampled
    when sampling - and what the variant adds to the family's arguments: (function, (lengths_arr,) or (), (seed,) or ()).  The seed of a
    sampled call advances torch's CPU generator, once per call: new draws per call, torch.manual_seed controls reproducibility."""
    fn = getattr(lib, family + ("_ragged" if lengths_arr is not None else "") + ("_sampled" if do_sample else ""))
    return fn, (lengths_arr,) if lengths_arr is not None else (), _call_seed(do_sample)


class LLM_SFT:
    def __init__(self, num_tasks: int = 3, task_map: Optional[Dict[str, int]] = None, feats_dim: int = 768,
                 llm_base_config: Optional[dict] = None, *, device: str | torch.device = "cuda:0"):
        cfg = dict(global_size=4096, semantic_size=8192, hidden_size=512, num_layers=12, num_attention_heads=8)
        cfg.update(llm_base_config or {})
        self.task_map = dict(task_map or DEFAULT_TASK_MAP)
        self.device = torch.device(device)
        s = _lib.qa_lm_spec()
        s.hidden, s.n_layers, s.n_heads = cfg["hidden_size"], cfg["num_layers"], cfg["num_attention_heads"]
        s.intermediate = 4 * cfg["hidden_size"]  # llm.py:69
        s.global_size, s.semantic_size = cfg["global_size"], cfg["semantic_size"]
        s.feats_dim, s.num_tasks = feats_dim, num_tasks
        s.rope_theta, s.rms_eps = 10000.0, 1e-6  # LlamaConfig defaults (llm.py:63-72)
        self._spec = s
        self.label_smoothing = float(cfg.get("label_smoothing", 0.1))  # llm.py:24 default, conf/config.yaml:147
        self.vocab_size = 3 + cfg["global_size"] + cfg["semantic_size"]
        self.global_offset = 3
        self.semantic_offset = 3 + cfg["global_size"]
        self._lib = _lib.load_library()
        self._handle = C.c_void_p()
        self._caches = weakref.WeakSet()  # live KVCache objects of the handle
        self.hidden_size = cfg["hidden_size"]
        self.num_layers = cfg["num_layers"]

    def load_state_dict(self, state_dict: Dict[str, torch.Tensor], strict: bool = True):
        _lib.require_device()
        sd = {(k[4:] if k.startswith("dnn.") else k): v for k, v in state_dict.items()}
        self._free()
        table, n, keep = _lib.tensor_table(sd)
        handle = C.c_void_p()
        _lib.check(self._lib.qa_lm_create(C.byref(handle), C.byref(self._spec), table, n, self.device.index or 0))
        del keep
        self._handle = handle
        return self

    def eval(self):
        return self

    def _free(self):
        if getattr(self, "_handle", None) is not None and self._handle.value:
            for cache in list(self._caches):  # qa_lm_destroy frees the handle's caches: do it first, so no KVCache keeps a dead pointer
                cache.free()
            self._lib.qa_lm_destroy(self._handle)
            self._handle = C.c_void_p()

    def __del__(self):
        try:
            self._free()
        except Exception:
            pass

    # ---- sessions: the body over a cache the caller holds, and LLM_SFT's submodules as device calls

    def _ready(self):
        if not self._handle.value:
            raise _lib.QuarkAudioError(-3, "LLM_SFT has no weights: call load_state_dict first")

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    @torch.no_grad()
    def llm_forward(self, inputs_embeds: torch.Tensor, attention_mask=None, past_key_values: Optional[KVCache] = None,
                    use_cache: bool = False, output_attentions: bool = False, output_hidden_states: bool = False, position_ids=None,
                    cache_position=None, *, chunk_lengths: Optional[Sequence[int]] = None):
        """CustomLlamaModel.llm_forward (llm.py:150-227): inputs_embeds [B, n, hidden] at positions len .. len + n - 1 of
        `past_key_values` (a KVCache; use_cache=True with none creates one of B rows x max_position_embeddings), causal.  Returns an
        object with .last_hidden_state [B, n, hidden], .past_key_values (None unless use_cache) and .hidden_states (None, or the
        n_layers + 1 tensors of output_hidden_states).  A sequence's rows do not depend on the batch it is in.

        chunk_lengths (B ints, 0 .. n; needs a cache): row b feeds only its first chunk_lengths[b] positions, at the row's own position
        in the cache (qa_lm_forward_ragged).  The input behind a row's count is never read and the outputs there are exactly 0; a count
        of 0 leaves the row idle.  None is the plain call; on a cache whose rows differ in length it feeds n positions to every row."""
        self._ready()
        _unsupported(attention_mask=(attention_mask, None), position_ids=(position_ids, None), cache_position=(cache_position, None),
                     output_attentions=(bool(output_attentions), False))
        x = inputs_embeds.to(device=self.device, dtype=torch.float32).contiguous()
        if x.dim() != 3 or x.shape[2] != self.hidden_size:
            raise _lib.QuarkAudioError(-1, f"llm_forward: inputs_embeds must be [B, n, hidden = {self.hidden_size}], got {tuple(x.shape)}")
        B, n, d = x.shape
        cache = past_key_values
        if cache is not None and not isinstance(cache, KVCache):
            raise _lib.QuarkAudioError(-1, "llm_forward: past_key_values must be a unified_audio_amd.KVCache")
        if cache is not None and cache._lm is not self:
            raise _lib.QuarkAudioError(-1, "llm_forward: past_key_values belongs to another model")
        if use_cache and cache is None:
            cache = KVCache(self, B, MAX_POSITION_EMBEDDINGS)  # llm.py:170-171
        # chunk_lengths: zeros, so that a call whose counts are all 0 (which launches nothing) returns what every idle row returns
        new = torch.empty if chunk_lengths is None else torch.zeros
        out = new(x.shape, dtype=torch.float32, device=self.device)
        hs = new((self.num_layers + 1, B, n, d), dtype=torch.float32, device=self.device) if output_hidden_states else None
        hs_ptr = hs.data_ptr() if hs is not None else None
        if chunk_lengths is not None:
            lens = [int(v) for v in (chunk_lengths.tolist() if torch.is_tensor(chunk_lengths) else chunk_lengths)]
            if len(lens) != B:
                raise _lib.QuarkAudioError(-1, f"llm_forward: chunk_lengths has {len(lens)} entries for {B} sequences")
            _lib.check(self._lib.qa_lm_forward_ragged(self._handle, cache._ptr() if cache is not None else None, x.data_ptr(), B, n,
                                                      (C.c_int64 * B)(*lens), out.data_ptr(), hs_ptr, self._stream()))
        else:
            _lib.check(self._lib.qa_lm_forward(self._handle, cache._ptr() if cache is not None else None, x.data_ptr(), B, n, out.data_ptr(),
                                               hs_ptr, self._stream()))
        return SimpleNamespace(last_hidden_state=out, past_key_values=cache if use_cache else None,
                               hidden_states=tuple(hs.unbind(0)) if hs is not None else None, attentions=None)

    @torch.no_grad()
    def test_generate(self, inputs_embeds: torch.Tensor, top_k: int = 50, top_p: float = 0.95, temperature: float = 0.8):
        """llm.py:229-250: inputs_embeds one position at a time over a fresh cache; the concatenated last hidden states."""
        cache = KVCache(self, inputs_embeds.shape[0], max(int(inputs_embeds.shape[1]), 1))
        outs = [self.llm_forward(inputs_embeds[:, i:i + 1], past_key_values=cache, use_cache=True).last_hidden_state
                for i in range(inputs_embeds.shape[1])]
        cache.free()
        return torch.cat(outs, dim=1)

    @torch.no_grad()
    def codec_embedding(self, ids: torch.Tensor) -> torch.Tensor:
        """LLM_SFT.codec_embedding: raw vocabulary ids [...] -> [..., hidden]; IndexError for an id outside the vocabulary."""
        self._ready()
        t = ids.to(device=self.device, dtype=torch.int64).contiguous()
        out = torch.empty(tuple(t.shape) + (self.hidden_size,), dtype=torch.float32, device=self.device)
        if t.numel():
            bad = C.c_int64(0)
            _lib.check(self._lib.qa_codes_check(t.data_ptr(), t.numel(), self.vocab_size, C.byref(bad), self._stream()))
            if bad.value:
                raise IndexError(f"{bad.value} ids out of range [0, {self.vocab_size})")
            _lib.check(self._lib.qa_lm_embed(self._handle, t.data_ptr(), t.numel(), out.data_ptr(), self._stream()))
        return out

    @torch.no_grad()
    def output_head(self, hidden: torch.Tensor, lo: int = 0, width: Optional[int] = None) -> torch.Tensor:
        """LLM_SFT.output_head on last_hidden_state rows [..., hidden] -> logits [..., width] of the vocabulary slice [lo, lo + width)
        (default: the whole vocabulary)."""
        self._ready()
        h = hidden.to(device=self.device, dtype=torch.float32).contiguous()
        if h.shape[-1] != self.hidden_size:
            raise _lib.QuarkAudioError(-1, f"output_head: hidden must be [..., {self.hidden_size}], got {tuple(h.shape)}")
        width = self.vocab_size - int(lo) if width is None else int(width)
        out = torch.empty(tuple(h.shape[:-1]) + (width,), dtype=torch.float32, device=self.device)
        rows = h.numel() // self.hidden_size
        if rows:
            _lib.check(self._lib.qa_lm_head(self._handle, h.data_ptr(), rows, int(lo), width, out.data_ptr(), self._stream()))
        return out

    @staticmethod
    def _lengths(name: str, lengths, B: int):
        """A per-row length argument (None, or B ints as a list / tensor) as (list or None, HOST int64 array or None)."""
        return _lib.host_lengths(name, lengths, B)

    @torch.no_grad()
    def build_prompt(self, task_name: str, enroll_feats: Optional[torch.Tensor], mix_feats: torch.Tensor, *, enroll_lengths=None,
                     mix_lengths=None) -> torch.Tensor:
        """llm_sft.py:110-128: [task, (enroll_sos, adapter(enroll_feats)), mix_sos, adapter(mix_feats)] -> [B, L, hidden].

        enroll_lengths / mix_lengths (keyword only; B frame counts each, None: every row at full width): row b uses
        enroll_feats[b, :enroll_lengths[b]] and mix_feats[b, :mix_lengths[b]].  The result is [B, Lp_max, hidden] with Lp_max the prompt
        at the tensors' widths; row b is left-aligned over its own Lp_b = 1 + (1 + enroll_lengths[b]) + 1 + mix_lengths[b] positions
        (2 + mix_lengths[b] without an enrollment) - build_prompt of the row alone, bit for bit - with exact zeros behind.  Padding frames
        are never copied.  It feeds llm_forward(..., chunk_lengths=Lp) on a KVCache (qa_lm_prompt_ragged)."""
        self._ready()
        task = self.task_map[task_name]  # KeyError like the reference
        mix = mix_feats.to(device=self.device, dtype=torch.float32).contiguous()
        if mix.dim() != 3 or mix.shape[2] != self._spec.feats_dim:
            raise _lib.QuarkAudioError(-1, f"build_prompt: mix_feats must be [B, N, {self._spec.feats_dim}], got {tuple(mix.shape)}")
        B, n_mix, _ = mix.shape
        enr, n_enr = None, 0
        if enroll_feats is not None:
            enr = enroll_feats.to(device=self.device, dtype=torch.float32).contiguous()
            if enr.dim() != 3 or enr.shape[0] != B or enr.shape[2] != self._spec.feats_dim:
                raise _lib.QuarkAudioError(-1, f"build_prompt: enroll_feats must be [{B}, N, {self._spec.feats_dim}], got {tuple(enr.shape)}")
            n_enr = enr.shape[1]
        L = 1 + (1 + n_enr if enr is not None else 0) + 1 + n_mix
        out = torch.empty((B, L, self.hidden_size), dtype=torch.float32, device=self.device)
        if enroll_lengths is not None or mix_lengths is not None:
            _, ne_arr = self._lengths("build_prompt: enroll_lengths", enroll_lengths, B)
            _, nm_arr = self._lengths("build_prompt: mix_lengths", mix_lengths, B)
            _lib.check(self._lib.qa_lm_prompt_ragged(self._handle, task, enr.data_ptr() if enr is not None else None, n_enr, ne_arr,
                                                     mix.data_ptr(), n_mix, nm_arr, B, out.data_ptr(), self._stream()))
            return out
        _lib.check(self._lib.qa_lm_prompt(self._handle, task, enr.data_ptr() if enr is not None else None, n_enr, mix.data_ptr(), n_mix, B,
                                          out.data_ptr(), self._stream()))
        return out

    @torch.no_grad()
    def generate(self, task_name: str, enroll_mel, enroll_feats, mix_mel: torch.Tensor, mix_feats: torch.Tensor,
                 global_length: int = 32, temperature: float = 0.8, top_k: int = 50, top_p: float = 0.95,
                 do_sample: bool = True, *, enroll_lengths=None, mix_lengths=None, semantic_lengths=None):
        """Returns (global_ids [B, global_length], semantic_ids [B, mix_mel.size(1)]) int64, offsets subtracted.
        mix_lengths / semantic_lengths (keyword only; B ints each, None: every row at full width): mix_feats is
        [B, max(mix_lengths), feats_dim] and row b is what the reference returns for that sequence alone on mix_feats[b, :mix_lengths[b]]
        with semantic_lengths[b] semantic steps (0 .. S_max = mix_mel.size(1), checked by the library).  semantic_ids comes back
        [B, S_max] with -1 behind each row's length - what BiCodec.detokenize(..., lengths=semantic_lengths) ignores.  Padding frames
        are never read, and a finished row stops costing key / value traffic (qa_lm_generate_rows).
        enroll_lengths (keyword only; None: the reference's rectangular call): a sequence or tensor of B frame counts for a batch whose
        enrollments differ in length.  enroll_feats is then [B, max(enroll_lengths), feats_dim], row b's frames at or behind
        enroll_lengths[b] are padding that is never read, and row b's tokens are what the reference returns for that sequence alone
        with its own enroll_feats[b:b+1, :enroll_lengths[b]] (qa_lm_generate_ragged).
        Only `mix_mel.size(1)` is consumed from the mel inputs, exactly like the reference (llm_sft.py:108).
        do_sample=True (the reference's signature default, llm_sft.py:106) samples every token on the device with
        CustomLlamaModel.sample_logits' filters (llm.py:253-288); the draws come from a Philox stream seeded from torch's
        global generator (torch.manual_seed controls reproducibility, as in the reference), so the distribution - not
        the individual stream - matches the reference."""
        if not self._handle.value:
            raise _lib.QuarkAudioError(-3, "LLM_SFT has no weights: call load_state_dict first")
        task = self.task_map[task_name]  # KeyError like the reference
        mix = mix_feats.to(device=self.device, dtype=torch.float32).contiguous()
        B, n_mix, _ = mix.shape
        enr, n_enr = None, 0
        if enroll_mel is not None:
            enr = enroll_feats.to(device=self.device, dtype=torch.float32).contiguous()
            n_enr = enr.shape[1]
        S = int(mix_mel.size(1))
        gids = torch.empty((B, global_length), dtype=torch.int64, device=self.device)
        sids = torch.empty((B, S), dtype=torch.int64, device=self.device)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        _, arr = _lib.host_lengths("generate: enroll_lengths", enroll_lengths, B)
        if arr is not None and enr is not None and (enr.dim() != 3 or enr.shape[0] != B):
            raise _lib.QuarkAudioError(-1, f"generate: enroll_feats must be [{B}, max(enroll_lengths), feats_dim], got {tuple(enr.shape)}")
        _, nm_arr = _lib.host_lengths("generate: mix_lengths", mix_lengths, B)
        _, ns_arr = _lib.host_lengths("generate: semantic_lengths", semantic_lengths, B)
        if nm_arr is not None or ns_arr is not None:
            fn = self._lib.qa_lm_generate_rows_sampled if do_sample else self._lib.qa_lm_generate_rows
            seed = _call_seed(do_sample)
            _lib.check(fn(self._handle, task, enr.data_ptr() if enr is not None else None, n_enr, arr, mix.data_ptr(), n_mix, nm_arr, B,
                          global_length, S, ns_arr, temperature, top_k, top_p, *seed, gids.data_ptr(), sids.data_ptr(), stream))
            return gids, sids
        # without them: qa_lm_generate / qa_lm_generate_ragged themselves, so that their messages keep their prefix
        fn, lens, seed = _generate_call(self._lib, "qa_lm_generate", arr, do_sample)
        _lib.check(fn(self._handle, task, enr.data_ptr() if enr is not None else None, n_enr, *lens, mix.data_ptr(), n_mix, B, global_length, S,
                      temperature, top_k, top_p, *seed, gids.data_ptr(), sids.data_ptr(), stream))
        return gids, sids

    def _score(self, task_name: str, enroll_mel, enroll_feats, mix_mel, mix_feats, global_ids, semantic_ids, mix_lengths=None,
               semantic_lengths=None, enroll_lengths=None):
        """qa_lm_score, or qa_lm_score_ragged with any per-row length: (loss_per_seq float [B], correct_per_seq int64 [B], loss, acc 0-dim
        float, Lt) on the device.  Lt is G + T + 2, or with per-row lengths Lt_b = G + semantic_lengths[b] + 2 as an int64 [B] device tensor;
        only the ids inside a row's length are then range-checked."""
        if not self._handle.value:
            raise _lib.QuarkAudioError(-3, "LLM_SFT has no weights: call load_state_dict first")
        task = self.task_map[task_name]  # KeyError like the reference
        B = int(mix_mel.size(0))  # llm_sft.py:63: the task row is repeated mix_mel.size(0) times
        mix = mix_feats.to(device=self.device, dtype=torch.float32).contiguous()
        if mix.dim() != 3 or mix.shape[0] != B:
            raise _lib.QuarkAudioError(-1, f"mix_feats must be [B={B}, N, feats_dim], got {tuple(mix.shape)}")
        enr, n_enr = None, 0
        if enroll_mel is not None:  # llm_sft.py:72: only the None test reads enroll_mel
            enr = enroll_feats.to(device=self.device, dtype=torch.float32).contiguous()
            if enr.dim() != 3 or enr.shape[0] != B:
                raise _lib.QuarkAudioError(-1, f"enroll_feats must be [B={B}, N, feats_dim], got {tuple(enr.shape)}")
            n_enr = enr.shape[1]
        g = global_ids.to(device=self.device, dtype=torch.int64)  # .long() (llm_sft.py:48-49)
        sids = semantic_ids.to(device=self.device, dtype=torch.int64)
        g = g.reshape(B, g.numel() // B).contiguous()  # a width of 0 (no id at all) is a valid shape
        sids = sids.reshape(B, sids.numel() // B).contiguous()
        G, T = g.shape[1], sids.shape[1]
        _, ne_arr = self._lengths("enroll_lengths", enroll_lengths, B)
        _, nm_arr = self._lengths("mix_lengths", mix_lengths, B)
        t_lens, t_arr = self._lengths("semantic_lengths", semantic_lengths, B)
        ragged = ne_arr is not None or nm_arr is not None or t_arr is not None
        stream = torch.cuda.current_stream(self.device).cuda_stream
        # nn.Embedding's range check of the shifted input ids (the targets are the same ids): one count, one host synchronisation.  With
        # per-row lengths over the ids a row really holds: what lies at or behind semantic_lengths[b] is padding
        Lt, live_sids = G + T + 2, sids.reshape(-1)
        if ragged:
            t_dev = torch.tensor(t_lens if t_lens is not None else [T] * B, dtype=torch.int64, device=self.device)
            Lt, live_sids = t_dev + (G + 2), sids[torch.arange(T, device=self.device)[None, :] < t_dev[:, None]]
        shifted = torch.cat([g.reshape(-1) + self.global_offset, live_sids + self.semantic_offset]).contiguous()
        if shifted.numel():
            bad = C.c_int64(0)
            _lib.check(self._lib.qa_codes_check(shifted.data_ptr(), shifted.numel(), self.vocab_size, C.byref(bad), stream))
            if bad.value:
                raise IndexError(f"{bad.value} input ids out of range [0, {self.vocab_size}) after the offsets (global + {self.global_offset}, "
                                 f"semantic + {self.semantic_offset})")
        loss_seq = torch.empty(B, dtype=torch.float32, device=self.device)
        correct = torch.empty(B, dtype=torch.int64, device=self.device)
        out = torch.empty(2, dtype=torch.float32, device=self.device)
        enr_ptr = enr.data_ptr() if enr is not None else None
        outs = (self.label_smoothing, loss_seq.data_ptr(), correct.data_ptr(), out.data_ptr(), out[1:].data_ptr(), stream)
        if ragged:
            _lib.check(self._lib.qa_lm_score_ragged(self._handle, task, enr_ptr, n_enr, ne_arr, mix.data_ptr(), mix.shape[1], nm_arr, B,
                                                    g.data_ptr(), G, sids.data_ptr(), T, t_arr, *outs))
        else:  # qa_lm_score itself, so that its messages keep their prefix
            _lib.check(self._lib.qa_lm_score(self._handle, task, enr_ptr, n_enr, mix.data_ptr(), mix.shape[1], B, g.data_ptr(), G,
                                             sids.data_ptr(), T, *outs))
        return loss_seq, correct, out[0], out[1], Lt

    _score_ragged = _score  # the name tests/test_lm_score_ragged_gpu.py calls it by: the same function, the lengths in the same order

    @torch.no_grad()
    def forward(self, task_name: str, enroll_mel, enroll_feats, mix_mel, mix_feats, global_ids, semantic_ids, *, mix_lengths=None,
                semantic_lengths=None, enroll_lengths=None):
        """llm_sft.py:37-90: teacher-forced (loss, acc), 0-dim float32 device tensors.  loss = F.kl_div(log_softmax(logits), true_dist,
        'batchmean') over the B * (G + T + 2) target rows with label smoothing `label_smoothing` (llm.py:87-104); acc = the fraction of
        rows whose first arg-max over the full vocabulary is the target.  global_ids [B, G] / semantic_ids [B, T], int32 or int64, offsets
        subtracted (what BiCodecTokenizer.tokenize returns; any G).  Forward only: no graph, no gradient.

        mix_lengths / semantic_lengths / enroll_lengths (keyword only; a list or tensor of B ints each, None: every row at full width;
        DESIGN.md section 35): row b is scored as that sequence alone on enroll_feats[b, :enroll_lengths[b]], mix_feats[b, :mix_lengths[b]]
        and semantic_ids[b, :semantic_lengths[b]], with Lt_b = G + semantic_lengths[b] + 2 target rows.  What lies at or behind a row's
        lengths is never read and never range-checked.  loss and acc then pool the rows: the sums over all target rows divided by
        sum_b Lt_b.  With all three None the call is the reference's rectangular one."""
        _, _, loss, acc, _ = self._score(task_name, enroll_mel, enroll_feats, mix_mel, mix_feats, global_ids, semantic_ids, mix_lengths,
                                         semantic_lengths, enroll_lengths)
        return loss, acc

    def __call__(self, *args, **kwargs):
        return self.forward(*args, **kwargs)

    @torch.no_grad()
    def score(self, task_name: str, enroll_mel, enroll_feats, mix_mel, mix_feats, global_ids, semantic_ids, *, mix_lengths=None,
              semantic_lengths=None, enroll_lengths=None):
        """forward per sequence: (loss [B], acc [B]) float32 - each sequence's mean label-smoothed KL and accuracy over its own G + T + 2
        target rows (forward's scalars are their means).  A sequence's values do not depend on the batch it is scored in.
        With per-row lengths (see forward) row b's values are over its own Lt_b = G + semantic_lengths[b] + 2 rows."""
        loss_seq, correct, _, _, Lt = self._score(task_name, enroll_mel, enroll_feats, mix_mel, mix_feats, global_ids, semantic_ids, mix_lengths,
                                                  semantic_lengths, enroll_lengths)
        return loss_seq, correct.to(torch.float32) / (Lt.to(torch.float32) if torch.is_tensor(Lt) else Lt)

    def enable_taps(self, on: bool = True):
        """Test hook: make generate record the slice logits of every decode step (qa_lm_enable_taps)."""
        if not self._handle.value:
            raise _lib.QuarkAudioError(-3, "LLM_SFT has no weights: call load_state_dict first")
        _lib.check(self._lib.qa_lm_enable_taps(self._handle, int(on)))
        return self

    def tap(self, name: str) -> torch.Tensor:
        """Test hook: flat fp32 copy of a snapshot of the last generate: "logits.global" ([B, global_length + 1, global_size]) or
        "logits.semantic" ([B, semantic_length, semantic_size]); of the last forward / score: "logits.forced" ([B, G + T + 2, vocab]; after a call with per-row lengths packed,
        [sum_b Lt_b, vocab], sequences in order)."""
        n = self._lib.qa_lm_tap(self._handle, name.encode(), None, 0, None)
        if n < 0:
            _lib.check(int(n))
        out = torch.empty(int(n), dtype=torch.float32, device=self.device)
        n2 = self._lib.qa_lm_tap(self._handle, name.encode(), out.data_ptr(), n, torch.cuda.current_stream(self.device).cuda_stream)
        if n2 < 0:
            _lib.check(int(n2))
        return out


DEFAULT_CONFORMER_PARAMS = dict(num_layers=2, dim=256, heads=8, dim_head=32, depthwise_conv_kernel_size=31, ff_mult=4, dropout=0.1,
                                qk_norm=None, pe_attn_head=None)  # llm.py:25-35


class CustomLlamaModel:
    """llm.py:13-374: the Llama body with the Conformer condition encoder in front.  `forward` and `generate` take the log-mel
    condition `cond` [B, T, cond_dim] (prompt [mix_sos, cond_output_layer(cond_encoder(cond_input_layer(cond)))]) or None (no prompt).
    The reference's generate is written for one sequence (llm.py:316); here B = cond.size(0), or `batch_size` without a condition, and
    every row equals its one-sequence result under greedy decoding.  `rope_interleaved`: see unified_audio_amd.conformer."""

    def __init__(self, cond_dim: int = 80, global_size: int = 4096, semantic_size: int = 8192, hidden_size: int = 256, num_layers: int = 2,
                 num_attention_heads: int = 8, dropout_p: float = 0.1, max_position_embeddings: int = 4096, label_smoothing: float = 0.1,
                 conformer_params: Optional[dict] = None, *, rope_interleaved: bool = True, device: str | torch.device = "cuda:0"):
        from .conformer import ConditionEncoder

        if max_position_embeddings != 4096:
            raise ValueError("max_position_embeddings is 4096 in this library (conf/config.yaml:146)")
        self.device = torch.device(device)
        self.cond_dim, self.hidden_size = int(cond_dim), int(hidden_size)
        # the LM handle is LLM_SFT's: its task / enrollment / adapter tensors do not exist in this model and are filled with zeros
        self._lm = LLM_SFT(num_tasks=1, feats_dim=32, device=device,
                           llm_base_config=dict(global_size=global_size, semantic_size=semantic_size, hidden_size=hidden_size,
                                                num_layers=num_layers, num_attention_heads=num_attention_heads,
                                                label_smoothing=label_smoothing))
        self._cond = ConditionEncoder(cond_dim, hidden_size, dict(conformer_params or DEFAULT_CONFORMER_PARAMS),
                                      rope_interleaved=rope_interleaved, device=device)
        self._has_cond = False
        self.label_smoothing = float(label_smoothing)
        self.vocab_size, self.global_offset, self.semantic_offset = self._lm.vocab_size, self._lm.global_offset, self._lm.semantic_offset

    def load_state_dict(self, state_dict: Dict[str, torch.Tensor], strict: bool = True):
        """The reference's keys (`dnn.` prefix optional).  Without `cond_*` keys the body still loads (strict=False) and the condition
        path raises when called."""
        sd = {(k[4:] if k.startswith("dnn.") else k): v for k, v in state_dict.items()}
        d = self.hidden_size
        body = {k: v for k, v in sd.items() if not k.startswith("cond_")}
        body.setdefault("task_embedding.weight", torch.zeros(1, d))
        body.setdefault("enroll_sos_embedding.weight", torch.zeros(1, d))
        body.setdefault("adapter.weight", torch.zeros(d, 32))
        body.setdefault("adapter.bias", torch.zeros(d))
        self._lm.load_state_dict(body)
        self._has_cond = any(k.startswith("cond_") for k in sd)
        if self._has_cond:
            self._cond.load_state_dict(sd)
        elif strict:
            raise _lib.QuarkAudioError(-3, "CustomLlamaModel.load_state_dict: no cond_input_layer / cond_encoder / cond_output_layer keys "
                                           "(strict=False loads the body alone)")
        return self

    def eval(self):
        return self

    @property
    def lm(self) -> "LLM_SFT":
        """The LLM_SFT facade of the SAME qa_lm handle (num_tasks = 1, feats_dim = 32 unless the checkpoint carried LLM_SFT's task /
        enrollment / adapter tensors in those shapes): its generate / forward share weights, workspace and captured steps with this model."""
        return self._lm

    def encode_condition(self, cond: torch.Tensor, lengths=None) -> torch.Tensor:
        """cond [B, T, cond_dim] -> the prompt embeddings [B, T, hidden_size] (llm.py:130-132).  lengths (B frame counts, None: every row
        at T): row b is encoded as cond[b:b+1, :lengths[b]] alone would be, with exact zeros behind (ConditionEncoder.forward)."""
        if not self._has_cond:
            raise _lib.QuarkAudioError(-3, "CustomLlamaModel: the checkpoint had no cond_* weights, the condition path cannot run")
        return self._cond(cond, lengths=lengths)

    @torch.no_grad()
    def generate(self, cond: Optional[torch.Tensor] = None, global_length: int = 32, semantic_length: int = 150, temperature: float = 0.8,
                 top_k: int = 50, top_p: float = 0.95, do_sample: bool = True, *, batch_size: int = 1, cond_lengths=None):
        """llm.py:291-374 -> (global_ids [B, global_length], semantic_ids [B, semantic_length]) int64, offsets subtracted.  Sampling as
        LLM_SFT.generate: Philox draws seeded from torch's global generator.

        cond_lengths (keyword only; B frame counts, None: every row at T): row b is generated as generate(cond[b:b+1, :cond_lengths[b]])
        would generate it alone - the condition encoder and the LM both run with the rows' lengths, in one pass each
        (qa_cond_encoder_forward_ragged, qa_lm_generate_cond_ragged).  global_length and semantic_length stay common
        to the batch."""
        lm = self._lm
        if not lm._handle.value:
            raise _lib.QuarkAudioError(-3, "CustomLlamaModel has no weights: call load_state_dict first")
        emb, T, B = None, 0, int(batch_size)
        if cond is not None:
            emb = self.encode_condition(cond, cond_lengths)
            B, T = emb.shape[0], emb.shape[1]
        _, nc_arr = _lib.host_lengths("generate: cond_lengths", cond_lengths, B)
        gids = torch.empty((B, global_length), dtype=torch.int64, device=self.device)
        sids = torch.empty((B, semantic_length), dtype=torch.int64, device=self.device)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        fn, lens, seed = _generate_call(lm._lib, "qa_lm_generate_cond", nc_arr, do_sample)
        _lib.check(fn(lm._handle, emb.data_ptr() if emb is not None else None, T, *lens, B, global_length, semantic_length, temperature, top_k,
                      top_p, *seed, gids.data_ptr(), sids.data_ptr(), stream))
        return gids, sids

    def llm_forward(self, inputs_embeds, attention_mask=None, past_key_values=None, use_cache=False, output_attentions=False,
                    output_hidden_states=False, position_ids=None, cache_position=None, *, chunk_lengths=None):
        """llm.py:150-227 over a KVCache: see LLM_SFT.llm_forward (the same code on the same handle)."""
        return self._lm.llm_forward(inputs_embeds, attention_mask, past_key_values, use_cache, output_attentions, output_hidden_states,
                                    position_ids, cache_position, chunk_lengths=chunk_lengths)

    def test_generate(self, inputs_embeds, top_k: int = 50, top_p: float = 0.95, temperature: float = 0.8):
        """llm.py:229-250"""
        return self._lm.test_generate(inputs_embeds, top_k, top_p, temperature)

    def codec_embedding(self, ids):
        return self._lm.codec_embedding(ids)

    def output_head(self, hidden, lo: int = 0, width: Optional[int] = None):
        return self._lm.output_head(hidden, lo, width)

    def build_prompt(self, task_name, enroll_feats, mix_feats, *, enroll_lengths=None, mix_lengths=None):
        """LLM_SFT.build_prompt on the same handle; with per-row lengths the result is [B, Lp_max, hidden], row b left-aligned over
        Lp_b = 1 + (1 + enroll_lengths[b]) + 1 + mix_lengths[b] positions (2 + mix_lengths[b] without an enrollment), zeros behind."""
        return self._lm.build_prompt(task_name, enroll_feats, mix_feats, enroll_lengths=enroll_lengths, mix_lengths=mix_lengths)

    def _score(self, global_ids, semantic_ids, cond, cond_lengths=None, semantic_lengths=None):
        """The last entry is Lt: G + T + 1, or with per-row lengths Lt_b = G + semantic_lengths[b] + 1 as an int64 [B] device tensor."""
        lm = self._lm
        if not lm._handle.value:
            raise _lib.QuarkAudioError(-3, "CustomLlamaModel has no weights: call load_state_dict first")
        B = int(global_ids.shape[0])
        ragged = cond_lengths is not None or semantic_lengths is not None
        g = global_ids.to(device=self.device, dtype=torch.int64)
        sids = semantic_ids.to(device=self.device, dtype=torch.int64)
        if ragged:  # a width of 0 (no id at all) is a valid shape here
            g, sids = g.reshape(B, g.numel() // B).contiguous(), sids.reshape(B, sids.numel() // B).contiguous()
        else:
            g, sids = g.reshape(B, -1).contiguous(), sids.reshape(B, -1).contiguous()
        G, T = g.shape[1], sids.shape[1]
        emb, Tc = None, 0
        if cond is not None:
            if cond.shape[0] != B:
                raise _lib.QuarkAudioError(-1, f"cond must be [B={B}, T, {self.cond_dim}], got {tuple(cond.shape)}")
            emb = self.encode_condition(cond, cond_lengths)
            Tc = emb.shape[1]
        stream = torch.cuda.current_stream(self.device).cuda_stream
        _, nc_arr = _lib.host_lengths("cond_lengths", cond_lengths, B)
        t_lens, t_arr = _lib.host_lengths("semantic_lengths", semantic_lengths, B)
        shifted = torch.cat([g.reshape(-1) + self.global_offset, sids.reshape(-1) + self.semantic_offset])
        t_dev = None
        if ragged:  # nn.Embedding's range check, over the ids a row really holds: what lies at or behind semantic_lengths[b] is padding
            t_dev = torch.tensor(t_lens if t_lens is not None else [T] * B, dtype=torch.int64, device=self.device)
            live = torch.arange(T, device=self.device)[None, :] < t_dev[:, None]
            shifted = torch.cat([g.reshape(-1) + self.global_offset, sids[live] + self.semantic_offset]).contiguous()
        if shifted.numel():
            bad = C.c_int64(0)
            _lib.check(lm._lib.qa_codes_check(shifted.data_ptr(), shifted.numel(), self.vocab_size, C.byref(bad), stream))
            if bad.value:
                raise IndexError(f"{bad.value} input ids out of range [0, {self.vocab_size}) after the offsets")
        loss_seq = torch.empty(B, dtype=torch.float32, device=self.device)
        correct = torch.empty(B, dtype=torch.int64, device=self.device)
        out = torch.empty(2, dtype=torch.float32, device=self.device)
        if ragged:
            _lib.check(lm._lib.qa_lm_score_cond_ragged(lm._handle, emb.data_ptr() if emb is not None else None, Tc, nc_arr, B, g.data_ptr(), G,
                                                       sids.data_ptr(), T, t_arr, self.label_smoothing, loss_seq.data_ptr(),
                                                       correct.data_ptr(), out.data_ptr(), out[1:].data_ptr(), stream))
            return loss_seq, correct, out[0], out[1], t_dev + (G + 1)
        _lib.check(lm._lib.qa_lm_score_cond(lm._handle, emb.data_ptr() if emb is not None else None, Tc, B, g.data_ptr(), G, sids.data_ptr(), T,
                                            self.label_smoothing, loss_seq.data_ptr(), correct.data_ptr(), out.data_ptr(),
                                            out[1:].data_ptr(), stream))
        return loss_seq, correct, out[0], out[1], G + T + 1

    @torch.no_grad()
    def forward(self, global_ids, semantic_ids, cond: Optional[torch.Tensor] = None, *, cond_lengths=None, semantic_lengths=None):
        """llm.py:107-147 -> (loss, acc), 0-dim float32 device tensors over the B * (G + T + 1) target rows (no semantic_eos target).

        cond_lengths / semantic_lengths (keyword only; B ints each, None: every row at full width): row b is scored
        as forward(global_ids[b:b+1], semantic_ids[b:b+1, :semantic_lengths[b]], cond[b:b+1, :cond_lengths[b]]) scores it alone, with
        Lt_b = G + semantic_lengths[b] + 1 target rows (the last position of its OWN stream is dropped).  loss and acc pool the rows: the
        sums over all target rows divided by sum_b Lt_b.  What lies at or behind a row's lengths is never read and never range-checked."""
        _, _, loss, acc, _ = self._score(global_ids, semantic_ids, cond, cond_lengths, semantic_lengths)
        return loss, acc

    def __call__(self, *args, **kwargs):
        return self.forward(*args, **kwargs)

    @torch.no_grad()
    def score(self, global_ids, semantic_ids, cond: Optional[torch.Tensor] = None, *, cond_lengths=None, semantic_lengths=None):
        """forward per sequence: (loss [B], acc [B]); with per-row lengths (see forward) over each row's own Lt_b target rows"""
        loss_seq, correct, _, _, Lt = self._score(global_ids, semantic_ids, cond, cond_lengths, semantic_lengths)
        return loss_seq, correct.to(torch.float32) / (Lt.to(torch.float32) if torch.is_tensor(Lt) else Lt)

    def enable_taps(self, on: bool = True):
        self._lm.enable_taps(on)
        return self

    def tap(self, name: str) -> torch.Tensor:
        """"logits.global" [B, global_length, global_size], "logits.semantic", "logits.forced" [B, G + T + 1, vocab] (packed
        [sum Lt_b, vocab] after a call with per-row lengths)"""
        return self._lm.tap(name)


def sample_logits(logits: torch.Tensor, temperature: float = 0.8, top_k: int = 50, top_p: float = 0.95,
                  do_sample: bool = True, seed: Optional[int] = None) -> torch.Tensor:
    """CustomLlamaModel.sample_logits (llm.py:253-288) on the device: logits [B, V] float32 cuda -> [B, 1] int64.
    Unlike the reference it does not filter `logits` in place."""
    lib = _lib.load_library()
    x = logits.to(dtype=torch.float32).contiguous()
    if not x.is_cuda:
        raise _lib.QuarkAudioError(-1, "sample_logits: logits must live on the HIP device (there is no CPU path)")
    out = torch.empty((x.shape[0],), dtype=torch.int64, device=x.device)
    if seed is None:
        seed = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())
    _lib.check(lib.qa_sample_logits(x.data_ptr(), x.shape[0], x.shape[1], x.stride(0), top_k, top_p, temperature,
                                    1 if do_sample else 0, seed, out.data_ptr(), torch.cuda.current_stream(x.device).cuda_stream))
    return out[:, None]
