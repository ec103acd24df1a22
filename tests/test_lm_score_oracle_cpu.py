"""Pins tests/lm_score_ref.py (the restatement of LLM_SFT.forward and its closed-form loss) to the reference's OWN forward
(QuarkAudio-UniSE/model/llm/llm_sft.py:37-90, llm.py:87-104): live through oracle/ref_llm_shim.py where the reference tree is present,
and everywhere through the values that reference run produced (tools/gen_golden_lm_score.py -> tests/golden/lm_score_*.npz)."""
import os

import numpy as np
import pytest
import torch

from oracle import llm_ref as L
from oracle import ref_llm_shim as S
from tests import lm_score_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
live = pytest.mark.skipif(not S.reference_available(), reason="the reference tree is not present")
TINY = L.LMSpec(hidden=64, n_layers=2, n_heads=2, global_size=40, semantic_size=50, feats_dim=32, num_tasks=3)


def test_token_ids_follow_the_reference_layout():
    spec = TINY
    inp, tgt = R.token_ids(torch.tensor([[0, 39]], dtype=torch.int32), torch.tensor([[5, 49, 0]]), spec)
    so = spec.semantic_offset
    assert inp.tolist() == [[0, 3, 42, 1, so + 5, so + 49, so]]
    assert tgt.tolist() == [[3, 42, 1, so + 5, so + 49, so, 2]]


@pytest.mark.parametrize("eps", [0.1, 0.0, 0.3])
def test_closed_form_kl_equals_kl_div_in_float64(eps):
    """The per-row closed form is F.kl_div(log_softmax, true_dist) summed over the vocabulary, ε = 0 included (xlogy: 0 log 0 = 0)."""
    g = torch.Generator().manual_seed(1)
    z = torch.randn(3, 7, 301, generator=g, dtype=torch.float64) * 4
    tgt = torch.randint(0, 301, (3, 7), generator=g)
    c, s = R.smoothing(eps, 301)
    true_dist = torch.full_like(z, s).scatter_(-1, tgt[..., None], c)
    want = torch.nn.functional.kl_div(torch.log_softmax(z, -1), true_dist, reduction="none").sum(-1)
    torch.testing.assert_close(R.row_kl(z, tgt, eps), want, rtol=1e-12, atol=1e-12)


def test_first_argmax_takes_the_lowest_index_of_exact_ties():
    x = torch.tensor([[1.0, 3.0, 3.0, 2.0], [5.0, 5.0, 5.0, 5.0]])
    assert R.first_argmax(x).tolist() == [1, 0]


@pytest.mark.parametrize("name", list(R.CASES))
def test_restatement_reproduces_reference_goldens(name):
    g = np.load(os.path.join(HERE, "golden", name + ".npz"))
    spec, sd, task, mix, enr, gi, si, eps = R.case_tensors(name)
    out = R.score(sd, spec, task, enr, mix, gi, si, eps)
    assert np.array_equal(out["targets"].numpy(), g["targets"].astype(np.int64))
    np.testing.assert_allclose(out["loss"], float(g["loss"]), rtol=2e-6)
    np.testing.assert_allclose(out["row_kl"].numpy(), g["row_kl"], rtol=1e-5, atol=1e-5)
    clear = g["gap"] > 1e-4  # away from near-ties the arg-max is the reference's
    assert np.array_equal(out["argmax"].numpy()[clear], g["argmax"].astype(np.int64)[clear])
    assert out["acc"] == pytest.approx(float(g["acc"]), abs=1e-6)
    if name.endswith("greedy_se"):
        assert 0.0 < float(g["acc"]) < 1.0


@live
@pytest.mark.parametrize("task,n_enr", [("se", 0), ("tse", 5), ("rtse", 3)])
@pytest.mark.parametrize("eps", [0.1, 0.0])
def test_restatement_equals_reference_forward(task, n_enr, eps):
    sd = L.lm_state_dict(7, TINY)
    mix = L.synth_feats(8, 3, 6, TINY.feats_dim)
    enr = L.synth_feats(9, 3, n_enr, TINY.feats_dim) if n_enr else None
    gen = torch.Generator().manual_seed(10)
    gi = torch.randint(0, TINY.global_size, (3, 5), generator=gen, dtype=torch.int32)
    si = torch.randint(0, TINY.semantic_size, (3, 7), generator=gen)
    loss_r, acc_r, z_r = R.reference_forward(TINY, sd, task, mix, enr, gi, si, eps)
    z, tgt = R.forced_logits(sd, TINY, task, enr, mix, gi, si)
    torch.testing.assert_close(z, z_r, rtol=1e-5, atol=1e-5)
    loss, acc = R.reference_loss(z, tgt, eps)  # the reference's own loss arithmetic on the restated logits
    torch.testing.assert_close(loss, loss_r, rtol=2e-6, atol=0)
    assert float(acc) == float(acc_r)
    closed = R.score(sd, TINY, task, enr, mix, gi, si, eps)  # the closed form in float64 on the same fp32 logits
    assert closed["loss"] == pytest.approx(float(loss_r), rel=2e-6)
    assert closed["acc"] == pytest.approx(float(acc_r), abs=1e-7)
