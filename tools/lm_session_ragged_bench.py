#!/usr/bin/env python
"""UniSE LM sessions with per-row lengths: a TSE batch whose enrollments differ in length (the lengths
tools/lm_ragged_bench.py draws: seeded, 2 - 5 s = 100 - 250 feature frames), mix prompt 250 frames, 33 + 250 greedy steps, written with
the primitives a user's own decode loop would call.

  ragged   (a) ONE cache: one llm_forward(chunk_lengths=) prefill of the left-aligned prompts, then the 283-step host-driven greedy loop
  grouped  (b) the same work as one session per distinct prompt length - the only way without per-row lengths
  join     (c) 16 rows only: 15 rows take one step while the 16th row's prompt is prefilled in the same call; beside it the two calls
               it replaces (a step of the 15 rows, a prefill of one row in a cache of its own)

Each figure is the median (and min - max) of REPS runs after one warm-up run, wall clock around a device synchronisation, as
tools/lm_session_bench.py.  One JSON line per figure is appended to profiles/lm_session_ragged_bench.jsonl (argument 3: another path)."""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import unified_audio_amd as qa  # noqa: E402
from unified_audio_amd import synth as L  # noqa: E402  (seeded weights / features: data generation only)

SIZES = [int(v) for v in sys.argv[1].split(",")] if len(sys.argv) > 1 else [16, 64]
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
OUT = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "lm_session_ragged_bench.jsonl")
N_MIX, G, S = 250, 32, 250
STEPS = G + 1 + S
FRAMES = (100, 250)  # 2 s .. 5 s of enrollment at 50 frames per second
dev = torch.device("cuda:0")
lm = qa.LLM_SFT(device=dev).load_state_dict(L.lm_state_dict(4321))
rows = []


def timed(fn, setup=None):
    ts, out = [], None
    for _ in range(REPS + 1):
        if setup:
            setup()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return (statistics.median(ts[1:]), min(ts[1:]), max(ts[1:])), out


def report(name, n, ms, **kw):
    row = dict(bench="lm_session_ragged", name=name, segments=n, ms_median=round(ms[0], 3), ms_min=round(ms[1], 3), ms_max=round(ms[2], 3),
               reps=REPS, **kw)
    rows.append(row)
    print(json.dumps(row), flush=True)


def greedy_loop(cache, B):
    """LLM_SFT.generate's two phases (llm_sft.py:137-193) on the primitives; the ids stay on the device."""
    out = []
    for first_id, steps, lo, width in ((0, G + 1, lm.global_offset, 4096), (1, S, lm.semantic_offset, 8192)):
        ids = torch.full((B,), first_id, dtype=torch.int64, device=dev)
        for _ in range(steps):
            h = lm.llm_forward(lm.codec_embedding(ids)[:, None], past_key_values=cache, use_cache=True).last_hidden_state[:, 0]
            ids = lm.output_head(h, lo, width).argmax(-1) + lo
            out.append(ids)
    return torch.stack(out, dim=1)


for n in SIZES:
    gen = torch.Generator().manual_seed(1000 + n)
    lens = torch.randint(FRAMES[0], FRAMES[1] + 1, (n,), generator=gen).tolist()
    distinct = sorted(set(lens))
    mix = L.synth_feats(50, n, N_MIX).to(dev)
    enr = L.synth_feats(51, n, max(lens)).to(dev)
    groups = {v: [b for b, x in enumerate(lens) if x == v] for v in distinct}
    # the prompts, per distinct length (set-up, not timed), and the same rows left-aligned in one [n, P_max, hidden] tensor
    group_prompt = {v: lm.build_prompt("tse", enr[idx, :v].contiguous(), mix[idx].contiguous()) for v, idx in groups.items()}
    plen = [int(group_prompt[v].shape[1]) for v in lens]
    P = max(plen)
    prompt = torch.zeros((n, P, lm.hidden_size), device=dev)
    for v, idx in groups.items():
        prompt[idx, :group_prompt[v].shape[1]] = group_prompt[v]
    cap = 64 * ((P + STEPS + 63) // 64)
    cache = qa.KVCache(lm, n, cap)
    group_cache = {v: qa.KVCache(lm, len(idx), cap) for v, idx in groups.items()}
    split = {}

    def ragged():
        t0 = time.perf_counter()
        lm.llm_forward(prompt, past_key_values=cache, use_cache=True, chunk_lengths=plen)
        torch.cuda.synchronize()
        split["ragged_prefill"] = (time.perf_counter() - t0) * 1e3
        return greedy_loop(cache, n)

    def grouped():
        toks = torch.empty((n, STEPS), dtype=torch.int64, device=dev)
        pre = 0.0
        for v, idx in groups.items():
            t0 = time.perf_counter()
            lm.llm_forward(group_prompt[v], past_key_values=group_cache[v], use_cache=True)
            torch.cuda.synchronize()
            pre += (time.perf_counter() - t0) * 1e3
            toks[idx] = greedy_loop(group_cache[v], len(idx))
        split["grouped_prefill"] = pre
        return toks

    def reset_groups():
        for c in group_cache.values():
            c.reset()

    ms_r, tok_r = timed(ragged, cache.reset)
    pre_r = split["ragged_prefill"]
    ms_g, tok_g = timed(grouped, reset_groups)
    pre_g = split["grouped_prefill"]
    total = n * STEPS
    report("ragged", n, ms_r, distinct_lengths=len(distinct), prompt_min=min(plen), prompt_max=P, steps=STEPS,
           prefill_ms_last_run=round(pre_r, 3), tok_per_s=round(total / ms_r[0] * 1e3))
    report("grouped", n, ms_g, distinct_lengths=len(distinct), sessions=len(distinct), steps=STEPS, prefill_ms_last_run=round(pre_g, 3),
           tok_per_s=round(total / ms_g[0] * 1e3))
    row = dict(bench="lm_session_ragged", name="grouped_over_ragged", segments=n, ratio_of_medians=round(ms_g[0] / ms_r[0], 2),
               decode_ratio_last_run=round((ms_g[0] - pre_g) / max(ms_r[0] - pre_r, 1e-9), 2), distinct_lengths=len(distinct),
               tokens_equal=bool(torch.equal(tok_r, tok_g)),
               note="a launch-bound decode step (DESIGN.md section 11) predicts a decode ratio near the number of distinct lengths")
    rows.append(row)
    print(json.dumps(row), flush=True)

    if n == 16:  # (c) the join: rows 0 .. 14 hold their prompts and step; row 15 is empty and takes its whole prompt in the same call
        base = plen[:15] + [0]
        x = prompt.clone()
        x[:15, 0] = lm.codec_embedding(torch.zeros(15, dtype=torch.int64, device=dev))
        counts = [1] * 15 + [plen[15]]

        def join_setup():
            cache.reset()
            lm.llm_forward(prompt, past_key_values=cache, use_cache=True, chunk_lengths=plen)
            cache.crop_rows(base)

        ms_j, _ = timed(lambda: lm.llm_forward(x, past_key_values=cache, use_cache=True, chunk_lengths=counts), join_setup)
        report("join_15_step_1_prefill", n, ms_j, n_max=P, prefill_positions=plen[15])
        ms_s, _ = timed(lambda: lm.llm_forward(x[:, :1].contiguous(), past_key_values=cache, use_cache=True, chunk_lengths=[1] * 15 + [0]), join_setup)
        report("step_15_of_16_rows", n, ms_s)
        one = qa.KVCache(lm, 1, cap)
        p15 = prompt[15:16, :plen[15]].contiguous()
        ms_p, _ = timed(lambda: lm.llm_forward(p15, past_key_values=one, use_cache=True), one.reset)
        report("prefill_1_row_alone", 1, ms_p, positions=plen[15])
    del cache, group_cache
os.makedirs(os.path.dirname(OUT), exist_ok=True)
with open(OUT, "a") as f:
    for row in rows:
        f.write(json.dumps(row) + "\n")
