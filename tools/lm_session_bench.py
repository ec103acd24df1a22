#!/usr/bin/env python
"""UniSE LM sessions micro-benchmark: llm_forward over a KVCache at the shapes of tools/lm_bench.py (B segments, SE prompt 252,
33 + 250 steps), written with the primitives a user's own decode loop would call.

  prefill        one llm_forward call of the 252-position prompt
  step           283 x [codec_embedding, llm_forward(n = 1), output_head, argmax]: a host-driven greedy loop
  chunk n        one llm_forward call of n = 4 / 16 / 64 positions over ~535 cached keys
  select 1 -> B  batch_repeat_interleave of a 252-position prefix run at B = 1

Each figure is the median of REPS runs after one warm-up run, wall clock around a device synchronisation.  One JSON line per figure is
appended to profiles/lm_session_bench.jsonl (argument 3: another path)."""
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

B = int(sys.argv[1]) if len(sys.argv) > 1 else 16
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
OUT = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "lm_session_bench.jsonl")
N_MIX, G, S = 250, 32, 250
dev = torch.device("cuda:0")
lm = qa.LLM_SFT(device=dev).load_state_dict(L.lm_state_dict(4321))
mix = L.synth_feats(50, B, N_MIX).to(dev)
prompt = lm.build_prompt("se", None, mix)
P = prompt.shape[1]
KV = P + G + 1 + S  # 535
cache = qa.KVCache(lm, B, 64 * ((KV + 64 + 63) // 64))  # room for the largest chunk behind 535 keys
rows = []


def timed(fn, setup=None):
    ts = []
    for i in range(REPS + 1):
        if setup:
            setup()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts[1:]), min(ts[1:]), max(ts[1:])


def report(name, ms, **kw):
    row = dict(bench="lm_session", name=name, B=B, ms_median=round(ms[0], 4), ms_min=round(ms[1], 4), ms_max=round(ms[2], 4), reps=REPS, **kw)
    rows.append(row)
    print(json.dumps(row), flush=True)


def prefill():
    lm.llm_forward(prompt, past_key_values=cache, use_cache=True)


def greedy_loop():
    """LLM_SFT.generate's two phases (llm_sft.py:137-193) on the primitives; the ids stay on the device."""
    out = []
    for first_id, steps, lo, width in ((0, G + 1, lm.global_offset, 4096), (1, S, lm.semantic_offset, 8192)):
        ids = torch.full((B,), first_id, dtype=torch.int64, device=dev)
        for _ in range(steps):
            h = lm.llm_forward(lm.codec_embedding(ids)[:, None], past_key_values=cache, use_cache=True).last_hidden_state[:, 0]
            ids = lm.output_head(h, lo, width).argmax(-1) + lo
            out.append(ids)
    return out


def body_only():
    """the same 283 positions through llm_forward(n = 1) alone: what the library's part of a step costs"""
    x = prompt[:, :1]
    for _ in range(G + 1 + S):
        lm.llm_forward(x, past_key_values=cache, use_cache=True)


report("prefill", timed(prefill, cache.reset), n=P)
ms = timed(greedy_loop, lambda: cache.crop(P))
report("greedy_loop", ms, steps=G + 1 + S, ms_per_step=round(ms[0] / (G + 1 + S), 4))
ms = timed(body_only, lambda: cache.crop(P))
report("forward_n1_only", ms, steps=G + 1 + S, ms_per_step=round(ms[0] / (G + 1 + S), 4))
for n in (4, 16, 64):
    x = prompt[:, :n].contiguous()
    report(f"chunk_n{n}", timed(lambda: lm.llm_forward(x, past_key_values=cache, use_cache=True), lambda: cache.crop(KV)), n=n, kv=KV)
one = qa.KVCache(lm, B, 256)


def prefix():
    one.reset()
    lm.llm_forward(prompt[:1], past_key_values=one, use_cache=True)


report(f"select_1_to_{B}", timed(lambda: one.batch_repeat_interleave(B), prefix), prefix=P)
# the closed loop on the same shapes, for the ratio (tools/lm_bench.py measures the same call)
mel = torch.zeros(B, S, 80)
ms = timed(lambda: lm.generate("se", None, None, mel, mix, do_sample=False))
report("generate", ms, steps=G + 1 + S, note="prefill + 283 fused steps with head and pick, graph replay off by default")
os.makedirs(os.path.dirname(OUT), exist_ok=True)
with open(OUT, "a") as f:
    for row in rows:
        f.write(json.dumps(row) + "\n")
