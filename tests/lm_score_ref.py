"""TEST INFRASTRUCTURE ONLY - CPU restatement of LLM_SFT.forward (QuarkAudio-UniSE/model/llm/llm_sft.py:37-90) and its loss
(model/llm/llm.py:87-104), built on oracle/llm_ref.py's prompt and Llama body.  Pinned to the reference's own forward by
tests/test_lm_score_oracle_cpu.py; the GPU tests (tests/test_lm_score_gpu.py) use it in float64 as the truth and in float32 as the
yardstick of what fp32 arithmetic costs.

The loss is evaluated in closed form per row, in float64 whatever the logits' precision:
    kl = c log c + (V - 1) s log s - c (z_y - lse) - s (sum z - z_y - (V - 1) lse),   0 log 0 = 0
with c = 1 - eps and s = eps / (V - 1) rounded to float32, as the reference's float32 true_dist holds them."""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import llm_ref as L


def token_ids(global_ids: torch.Tensor, semantic_ids: torch.Tensor, spec: L.LMSpec):
    """llm_sft.py:48-58: (input_ids, target_ids), both int64 [B, G + T + 2]."""
    g = global_ids.long() + spec.global_offset
    s = semantic_ids.long() + spec.semantic_offset
    B = g.shape[0]
    col = lambda v: torch.full((B, 1), v, dtype=torch.long)  # noqa: E731
    return torch.cat([col(0), g, col(1), s], dim=1), torch.cat([g, col(1), s, col(2)], dim=1)


def smoothing(eps: float, V: int):
    """(confidence, smoothing value) as float32 values, the entries of the reference's true_dist."""
    return float(np.float32(1.0 - eps)), float(np.float32(eps / (V - 1)))


@torch.no_grad()
def forced_logits(sd, spec: L.LMSpec, task: str, enroll_feats, mix_feats, global_ids, semantic_ids, dtype=torch.float32):
    """The teacher-forced full-vocabulary logits [B, Lt, V] and the targets [B, Lt] (llm_sft.py:60-84)."""
    if dtype != torch.float32:
        sd = {k: v.to(dtype) for k, v in sd.items()}
        enroll_feats = None if enroll_feats is None else enroll_feats.to(dtype)
        mix_feats = mix_feats.to(dtype)
    inp, tgt = token_ids(global_ids, semantic_ids, spec)
    x = torch.cat([L.build_prompt(sd, L.TASK_MAP[task], enroll_feats, mix_feats), sd["codec_embedding.weight"][inp]], dim=1)
    hs = L.llm_forward(sd, x, L.KVCache(spec.n_layers), spec, dtype)[:, -tgt.shape[1]:]
    return F.linear(hs, sd["output_head.weight"]), tgt


def row_kl(logits: torch.Tensor, tgt: torch.Tensor, eps: float) -> torch.Tensor:
    """Closed-form label-smoothed KL per row, float64 [B, Lt]."""
    z = logits.double()
    V = z.shape[-1]
    c, s = smoothing(eps, V)
    lse = torch.logsumexp(z, dim=-1)
    zy = z.gather(-1, tgt[..., None])[..., 0]
    kl = (c * math.log(c) if c > 0 else 0.0) - c * (zy - lse)
    if s > 0:
        kl = kl + (V - 1) * s * math.log(s) - s * (z.sum(-1) - zy - (V - 1) * lse)
    return kl


def first_argmax(x: torch.Tensor) -> torch.Tensor:
    """Index of the FIRST maximum along the last axis, independent of torch.argmax's tie behaviour."""
    m = x.amax(-1, keepdim=True)
    idx = torch.arange(x.shape[-1]).expand_as(x)
    return torch.where(x == m, idx, x.shape[-1]).amin(-1)


def score(sd, spec: L.LMSpec, task: str, enroll_feats, mix_feats, global_ids, semantic_ids, eps: float = 0.1, dtype=torch.float32) -> dict:
    """forward in closed form: logits, targets, row_kl, argmax, loss_seq [B], correct [B], loss, acc (float64 scalars)."""
    z, tgt = forced_logits(sd, spec, task, enroll_feats, mix_feats, global_ids, semantic_ids, dtype)
    kl = row_kl(z, tgt, eps)
    am = first_argmax(z)
    ok = (am == tgt)
    return dict(logits=z, targets=tgt, row_kl=kl, argmax=am, loss_seq=kl.mean(-1), correct=ok.sum(-1), loss=float(kl.mean()),
                acc=float(ok.double().mean()))


def reference_loss(logits: torch.Tensor, tgt: torch.Tensor, eps: float):
    """llm.py:87-104 and llm_sft.py:87 verbatim in the logits' precision: (F.kl_div 'batchmean' loss, accuracy)."""
    size = logits.shape[-1]
    z = logits.reshape(-1, size)
    t = tgt.reshape(-1)
    true_dist = z.clone()
    true_dist.fill_(eps / (size - 1))
    true_dist.scatter_(1, t.unsqueeze(1), 1.0 - eps)
    loss = F.kl_div(F.log_softmax(z, dim=-1), true_dist, reduction="batchmean")
    return loss, (logits.argmax(-1) == tgt).float().mean()


# ------------------------------------------------------------------------------- golden cases (tools/gen_golden_lm_score.py)

# a spec the HIP decode step accepts (hidden % 256 == 0, vocabulary slices multiples of 4), V = 259
SMALL = L.LMSpec(hidden=256, n_layers=2, n_heads=4, global_size=96, semantic_size=160, feats_dim=64, num_tasks=3)
# name -> (weight seed, task, B, n_mix, n_enroll, G, T, eps, targets): targets "random" = seeded ids over the whole slices,
# "greedy" = the reference's own greedy generate stream (accuracy neither 0 nor 1)
CASES = {
    "lm_score_small_se": (61, "se", 3, 9, 0, 4, 10, 0.1, "random"),
    "lm_score_small_tse": (62, "tse", 2, 7, 5, 6, 8, 0.1, "random"),
    "lm_score_small_rtse_eps0": (63, "rtse", 2, 6, 4, 5, 9, 0.0, "random"),
    "lm_score_small_greedy_se": (64, "se", 4, 8, 0, 6, 12, 0.1, "greedy"),
}


def case_tensors(name: str):
    """(spec, sd, task, mix, enr, global_ids, semantic_ids, eps) of a golden case, regenerated from its seeds."""
    seed, task, B, Nm, Ne, G, T, eps, kind = CASES[name]
    spec = SMALL
    sd = L.lm_state_dict(seed, spec)
    mix = L.synth_feats(seed + 100, B, Nm, spec.feats_dim)
    enr = L.synth_feats(seed + 101, B, Ne, spec.feats_dim) if Ne else None
    if kind == "greedy":
        g, s, _, _ = L.generate(sd, task, enr, mix, T, G, spec)
    else:
        gen = torch.Generator().manual_seed(seed + 102)
        g = torch.randint(0, spec.global_size, (B, G), generator=gen, dtype=torch.int32)  # tokenize's dtypes: int32 global, int64 semantic
        s = torch.randint(0, spec.semantic_size, (B, T), generator=gen, dtype=torch.int64)
    return spec, sd, task, mix, enr, g, s, eps


def reference_forward(spec, sd, task, mix, enr, global_ids, semantic_ids, eps):
    """The reference's OWN LLM_SFT.forward (oracle/ref_llm_shim.py): (loss, acc, logits [B, Lt, V]) - the logits are caught at
    output_head's output."""
    from oracle import ref_llm_shim as S

    model = S.load_state(S.load_reference_llm(spec), sd)
    model.label_smoothing = eps
    caught = []
    model.output_head.register_forward_hook(lambda m, i, o: caught.append(o.detach().clone()))
    mel = torch.zeros(mix.shape[0], 1, 80)  # only mix_mel.size(0) and `enroll_mel is None` are read (llm_sft.py:63,72)
    with torch.no_grad():
        loss, acc = model(task, None if enr is None else mel, enr, mel, mix, global_ids, semantic_ids)
    return loss, acc, caught[0]
