"""Golden values of `LLM_SFT.forward` (QuarkAudio-UniSE/model/llm/llm_sft.py:37-90), produced by the reference's OWN module on seeded
weights, features and token ids (unified_audio_amd/synth.py: the GPU machine regenerates the same inputs from the seeds of
tests/lm_score_ref.CASES, so only outputs are stored): the loss and accuracy, the per-row KL of the reference's float32 true_dist
(F.kl_div reduction='none' summed over the vocabulary), the per-row arg-max and the top-1 minus top-2 logit gap for the near-tie audit.

Run where the reference tree is present:  python tools/gen_golden_lm_score.py
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import lm_score_ref as R  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def main(names=None):
    for name in names or R.CASES:
        spec, sd, task, mix, enr, g, s, eps = R.case_tensors(name)
        loss, acc, z = R.reference_forward(spec, sd, task, mix, enr, g, s, eps)
        _, tgt = R.token_ids(g, s, spec)
        V = z.shape[-1]
        true_dist = torch.full_like(z, eps / (V - 1)).scatter_(-1, tgt[..., None], 1.0 - eps)
        kl = F.kl_div(F.log_softmax(z, dim=-1), true_dist, reduction="none").sum(-1)
        top2 = z.topk(2, dim=-1).values
        ours = R.score(sd, spec, task, enr, mix, g, s, eps)
        assert abs(ours["loss"] - float(loss)) <= 1e-5 * abs(float(loss)), (name, ours["loss"], float(loss))  # the pin itself
        np.savez_compressed(os.path.join(GOLDEN, name + ".npz"), loss=np.float32(loss), acc=np.float32(acc), row_kl=kl.numpy().astype(np.float32),
                            argmax=z.argmax(-1).numpy().astype(np.int16), gap=(top2[..., 0] - top2[..., 1]).numpy().astype(np.float32),
                            targets=tgt.numpy().astype(np.int16))
        print(f"{name}: loss {float(loss):.6f} acc {float(acc):.4f} rows {tuple(kl.shape)}")


if __name__ == "__main__":
    main(sys.argv[1:] or None)
