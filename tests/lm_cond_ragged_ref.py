"""TEST INFRASTRUCTURE ONLY - the oracle of the condition path with per-row lengths: every function of
tests/conformer_ref.py called on x[b:b+1, :L_b], one row at a time.  "Row b behaves as the rectangular call would for that clip alone at
its own length" is the definition, so the oracle is the rectangular restatement itself and nothing else.

Outputs are padded to the batch's width with NaN, not 0: a comparison takes the rows a length owns explicitly, and the zero tail of the
library's output is checked on its own."""
from __future__ import annotations

import math
from typing import List, Optional, Sequence

import torch

from tests import conformer_ref as R

NAN = float("nan")


def frames(n: int, hop: int = 320) -> int:
    """qa_logmel_frames"""
    return math.ceil(n / hop)


def _pad_rows(rows: Sequence[torch.Tensor], T: int) -> torch.Tensor:
    out = torch.full((len(rows), T) + tuple(rows[0].shape[1:]), NAN, dtype=rows[0].dtype)
    for b, r in enumerate(rows):
        out[b, :r.shape[0]] = r
    return out


def stft_logmel(wav: torch.Tensor, lengths: Sequence[int], dtype=torch.float32, **kw) -> torch.Tensor:
    """[B, frames(n), n_mels]: row b is R.stft_logmel(wav[b:b+1, :lengths[b]]), NaN behind its frames"""
    hop = kw.get("hop_length", 320)
    rows = [R.stft_logmel(wav[b:b + 1, :n], dtype=dtype, **kw)[0] for b, n in enumerate(lengths)]
    return _pad_rows(rows, frames(wav.shape[1], hop))


def conformer_encoder(sd, params, x: torch.Tensor, lengths: Sequence[int], dtype=torch.float32, taps: Optional[dict] = None, **kw):
    """[B, T, dim]: row b is R.conformer_encoder(x[b:b+1, :lengths[b]]) with no mask; taps likewise"""
    rows, row_taps = [], []
    for b, n in enumerate(lengths):
        t = {}
        rows.append(R.conformer_encoder(sd, params, x[b:b + 1, :n], None, dtype=dtype, taps=t, **kw)[0])
        row_taps.append(t)
    if taps is not None:
        for name in row_taps[0]:
            taps[name] = _pad_rows([t[name][0] for t in row_taps], x.shape[1])
    return _pad_rows(rows, x.shape[1])


def condition(sd, params, cond: torch.Tensor, lengths: Sequence[int], dtype=torch.float32, taps: Optional[dict] = None, **kw):
    rows, row_taps = [], []
    for b, n in enumerate(lengths):
        t = {}
        rows.append(R.condition(sd, params, cond[b:b + 1, :n], dtype=dtype, taps=t, **kw)[0])
        row_taps.append(t)
    if taps is not None:
        for name in row_taps[0]:
            taps[name] = _pad_rows([t[name][0] for t in row_taps], cond.shape[1])
    return _pad_rows(rows, cond.shape[1])


def generate(sd, spec, params, cond: torch.Tensor, lengths: Sequence[int], G: int, S: int, forced: Optional[torch.Tensor] = None,
             dtype=torch.float32):
    """R.generate on every row's own slice: (global_ids [B, G], semantic_ids [B, S], tokens [B, G + S], gaps [B, G + S])"""
    outs = [R.generate(sd, spec, params, cond[b:b + 1, :n], G, S, 1, forced=None if forced is None else forced[b:b + 1], dtype=dtype)
            for b, n in enumerate(lengths)]
    return tuple(torch.cat([o[i] for o in outs], dim=0) for i in range(4))


def score(sd, spec, params, global_ids, semantic_ids, cond: Optional[torch.Tensor], cond_lengths: Optional[Sequence[int]],
          semantic_lengths: Optional[Sequence[int]], eps: float, dtype=torch.float32) -> List[dict]:
    """R.score on every row's own slices (a list of its dicts, B = 1 each): cond[b:b+1, :cond_lengths[b]] and
    semantic_ids[b:b+1, :semantic_lengths[b]]; a vector that is None leaves that tensor at full width."""
    B = global_ids.shape[0]
    out = []
    for b in range(B):
        c = None if cond is None else cond[b:b + 1, :(cond.shape[1] if cond_lengths is None else cond_lengths[b])]
        s = semantic_ids[b:b + 1, :(semantic_ids.shape[1] if semantic_lengths is None else semantic_lengths[b])]
        out.append(R.score(sd, spec, params, global_ids[b:b + 1], s, c, eps, dtype=dtype))
    return out
