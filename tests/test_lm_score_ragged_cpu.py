"""CPU side of teacher-forced scoring with per-row lengths: the oracle's two formulations against one another in
float64, the host logic of csrc/lm_score_rows.h as a stand-alone program under the host sanitizers, and the two new ABI symbols."""
import os
import re
import shutil
import subprocess

import pytest
import torch

from oracle import llm_ref as L
from tests import lm_score_ragged_ref as RR
from tests import lm_score_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_case_is_what_it_claims():
    lp, lt, pos = RR.positions(RR.CASE_NE, RR.CASE_NM, RR.CASE_T, RR.CASE_G)
    assert pos == RR.CASE_POSITIONS
    assert 0 in RR.CASE_T and 1 in RR.CASE_NM and 1 in RR.CASE_NE
    assert any(128 < p <= 256 for p in pos) and any(p > 256 for p in pos)  # one and two 128-query block boundaries crossed
    assert any(0 < p % 128 <= 32 for p in pos)                            # a row that ends inside a block's first 32-key tile


def test_rows_scored_alone_equal_one_zero_padded_causal_batch_in_fp64():
    """No mask is needed: a left-aligned row followed by zero rows gives, through the causal body, the logits of the row alone."""
    sd, (enr, mix, g, s), o64, _ = RR.case_oracle("tse")
    padded = RR.padded_logits(sd, R.SMALL, "tse", enr, mix, g, s, RR.CASE_NE, RR.CASE_NM, RR.CASE_T, torch.float64)
    worst = 0.0
    for b, z in enumerate(padded):
        alone = o64["rows"][b]["logits"][0]
        assert z.shape == alone.shape == (RR.CASE_G + RR.CASE_T[b] + 2, 3 + R.SMALL.global_size + R.SMALL.semantic_size)
        worst = max(worst, float((z - alone).abs().max()))
        assert torch.equal(R.first_argmax(z), o64["rows"][b]["argmax"][0]), b
    print(f"padded batch vs rows alone, fp64: max |dz| = {worst:.3e}")
    assert worst <= 1e-12


def test_pooled_scalars_and_se_variant():
    sd, (enr, mix, g, s), o64, o32 = RR.case_oracle("tse")
    assert o64["Lt"] == [RR.CASE_G + t + 2 for t in RR.CASE_T]
    kl = torch.cat([o["row_kl"].reshape(-1) for o in o64["rows"]])
    assert o64["loss"] == pytest.approx(float(kl.mean()), rel=1e-12)
    assert o64["acc"] == pytest.approx(float(o64["correct"].sum()) / kl.numel(), abs=1e-12)
    for b, o in enumerate(o64["rows"]):
        assert float(o64["loss_seq"][b]) == pytest.approx(float(o["row_kl"].mean()), rel=1e-12)
    # equal lengths: the pooled scalars are the rectangular call's
    full = R.score(sd, R.SMALL, "se", None, mix[:, :7], g, s[:, :5], RR.CASE_EPS, torch.float64)
    rag = RR.score_ragged(sd, R.SMALL, "se", None, mix[:, :7], g, s[:, :5], None, [7] * 6, [5] * 6, RR.CASE_EPS, torch.float64)
    assert rag["loss"] == pytest.approx(full["loss"], rel=1e-12) and rag["acc"] == pytest.approx(full["acc"], abs=1e-12)
    for b in range(6):
        assert torch.equal(rag["rows"][b]["logits"][0], full["logits"][b])


def test_lm_score_rows_selftest_is_clean_under_the_host_sanitizers(tmp_path):
    """tools/lm_score_rows_selftest.cpp: every refusal with its row, offsets / maxima / groups against a naive recount (B = 1 .. 129),
    the uniform decision - compiled with -fsanitize=address,undefined and run as a program of its own."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler: the self-test of csrc/lm_score_rows.h cannot be built")
    exe = str(tmp_path / "lm_score_rows_selftest")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
           os.path.join(ROOT, "unified_audio_amd", "csrc"), os.path.join(ROOT, "tools", "lm_score_rows_selftest.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "lm_score_rows_selftest: ok" in r.stdout


def test_abi_declares_and_exports_the_ragged_entries(qa_lib):
    with open(os.path.join(ROOT, "include", "quarkaudio.h")) as f:
        header = f.read()
    for name in ("qa_lm_score_ragged", "qa_lm_prompt_ragged"):
        assert re.search(r"\bint " + name + r"\(qa_lm\* lm,", header), name
        assert hasattr(qa_lib, name), name
    assert "const int64_t* n_semantic" in header and "const int64_t* n_mix" in header
