"""The reduced conv_gemm arithmetics (unified_audio_amd.gemm_math: "split3", "bf16") through whole models, at the mini specs.

(a) H-Codec 1.0 mini, encode + decode of 2 short clips under split-6, split-3 and bf16: finite outputs; the decode waveform of the ORACLE's
    codes is closer to the oracle's waveform under split-3 than under bf16 (all three errors printed); each clip alone equals its row of
    the batch bit for bit in the reduced modes; and after the context manager exits a default call gives the bits it gave before.
(b) the UniSE LM keeps the fp32 chain (ConvParams::math_fp32): generate and its logits taps are bit-identical under modes 0, 1, 2, 3.
(c) H-Codec 1.5 mini and an SSL mini model: one split-3 call each runs, is finite and has the default call's shapes.

End-to-end accuracy of the reduced modes is a property of the arithmetic, measured by tools/gemm_math_bench.py, not a bound asserted here.
"""
import pytest
import torch

from oracle import hcodec_ref as R
from oracle import llm_ref as L
from oracle import synth
from tests.test_conv_gemm_presplit_gpu import _hcodec15, _ssl
from tests.test_llm_gpu import SMALL as LM_SMALL
from tests.test_llm_gpu import _model as _lm_model
from tests.util import MINI, rel_err

pytestmark = pytest.mark.gpu


# (a)
def test_hcodec10_under_each_arithmetic(qa_lib, gpu_device):
    import unified_audio_amd as qa

    assert qa.gemm_math_name() == "split6"
    ospec = R.HCodecSpec(**MINI)
    sd = synth.hcodec10_state_dict(5, ospec)
    codec = qa.Codec(None, None, None, spec=qa.HCodecSpec(**MINI), device=gpu_device).load_state_dict(sd)
    T = 16 * 64
    wav, feat = synth.synth_wav(6, 2, T), synth.synth_feat(7, 2, T // 8, 64)
    ac_o, sc_o = R.encode(sd, wav.unsqueeze(1), feat, ospec)
    wav_o = R.decode(sd, ac_o, sc_o, ospec)
    wd, fd, ac_d, sc_d = wav.to(gpu_device).unsqueeze(1), feat.to(gpu_device), ac_o.to(gpu_device), sc_o.to(gpu_device)

    def run(rows=slice(None)):
        ac, sc = codec.encode(wd[rows], fd[rows])
        return ac.clone(), sc.clone(), codec.decode(ac_d[rows], sc_d[rows]).clone()

    before = run()
    err = {}
    for mode in ("split6", "split3", "bf16"):
        with qa.gemm_math(mode):
            assert qa.gemm_math_name() == mode
            ac, sc, w = run()
            assert ac.shape == before[0].shape and sc.shape == before[1].shape and w.shape == before[2].shape
            assert torch.isfinite(w).all() and int(ac.min()) >= 0 and int(sc.min()) >= 0
            err[mode] = rel_err(w, wav_o)
            if mode == "split6":
                assert all(torch.equal(u, v) for u, v in zip((ac, sc, w), before))
            else:
                assert not torch.equal(w, before[2]), f"{mode} decoded the bits of split-6"
                for b in range(2):
                    alone = run(slice(b, b + 1))
                    for name, u, v in zip(("acoustic codes", "semantic codes", "waveform"), alone, (ac, sc, w)):
                        assert torch.equal(u, v[b:b + 1]), f"{mode}: {name} of clip {b} alone differ from its row of the batch"
        assert qa.gemm_math_name() == "split6"
    print("decode rel. RMS error against the oracle on its own codes: " + ", ".join(f"{m} {e:.3e}" for m, e in err.items()))
    assert err["split3"] < err["bf16"], err
    after = run()
    assert all(torch.equal(u, v) for u, v in zip(after, before)), "a default call after the reduced modes differs from the one before"


# (b)
def test_unise_lm_keeps_the_fp32_chain_in_every_mode(qa_lib, gpu_device):
    import unified_audio_amd as qa

    _, lm = _lm_model(LM_SMALL, 21, gpu_device)
    lm.enable_taps()
    B, Nm, S, G = 3, 9, 12, 5
    mix = L.synth_feats(1, B, Nm, LM_SMALL.feats_dim).to(gpu_device)
    mel = torch.zeros(B, S, 80)
    out = {}
    for mode in (1, 0, 2, 3):
        with qa.gemm_math(mode):
            gids, sids = lm.generate("se", None, None, mel, mix, global_length=G, do_sample=False)
            out[mode] = (gids.clone(), sids.clone(), lm.tap("logits.global").clone(), lm.tap("logits.semantic").clone())
    for mode in (0, 2, 3):
        for name, u, v in zip(("global ids", "semantic ids", "logits.global", "logits.semantic"), out[mode], out[1]):
            assert torch.equal(u, v), f"QA_GEMM_MATH = {mode}: {name} differ from the default's"


# (c)
@pytest.mark.parametrize("model", ["hcodec15", "ssl"])
def test_other_models_run_under_split3(qa_lib, gpu_device, model):
    import unified_audio_amd as qa

    run = {"hcodec15": _hcodec15, "ssl": _ssl}[model](qa_lib, gpu_device)
    default = [t.clone() for t in run()]
    with qa.gemm_math("split3"):
        out = [t.clone() for t in run()]
    assert [t.shape for t in out] == [t.shape for t in default]
    assert all(torch.isfinite(t).all() for t in out if t.is_floating_point())
    assert any(not torch.equal(u, v) for u, v in zip(out, default)), "split-3 gave the default's bits"
