"""Golden values of the UniSE condition path, produced by the reference's OWN classes (QuarkAudio-UniSE/model/llm/conformer.py
ConformerEncoder, model/model.py Model.stft_logmel, model/llm/llm.py CustomLlamaModel) on seeded weights and inputs
(tests/conformer_ref.py regenerates the inputs from their seeds, so only outputs are stored):

    lm_cond_conformer.npz   ConformerEncoder outputs for pe_attn_head None / 1 and with a ragged mask
    lm_cond_logmel.npz      Model.stft_logmel of seeded noise with an all-zero stretch, length not a multiple of the hop
    lm_cond_generate.npz    greedy generate(cond) and generate(None) token streams, with the top-2 logit gap of every step
    lm_cond_forward.npz     forward loss / accuracy with and without cond, label smoothing 0.1 and 0

The reference imports RotaryEmbedding / apply_rotary_pos_emb from x_transformers and melscale_fbanks from torchaudio; neither package
is available offline: tests/conformer_ref.py's restatement [upstream-memory] and oracle/stubs/torchaudio stand in for them.
Conditions checked here (and again by tests/test_lm_cond_oracle_cpu.py): every step's top-2 gap is above the 2e-4 near-tie bar, and the
conditional stream differs from the unconditional one.

Run where the reference tree is present:  python tools/gen_golden_lm_cond.py
"""
from __future__ import annotations

import importlib
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_llm_shim as S  # noqa: E402
from tests import conformer_ref as R  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
TIE = 2e-4


def reference_modules():
    R.install_x_transformers()
    S._import_llm_sft()
    conf = importlib.import_module("model.llm.conformer")
    conf.RotaryEmbedding, conf.apply_rotary_pos_emb = R.RotaryEmbedding, R.apply_rotary_pos_emb
    return conf, importlib.import_module("model.llm.llm")


def reference_custom_llama(llm, spec, params, sd, eps):
    model = llm.CustomLlamaModel(cond_dim=80, global_size=spec.global_size, semantic_size=spec.semantic_size, hidden_size=spec.hidden,
                                 num_layers=spec.n_layers, num_attention_heads=spec.n_heads, label_smoothing=eps, conformer_params=params)
    for layer in model.layers:
        S._patch_layer(layer)
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.startswith("rotary_emb.") or "rotary_embedding" in k for k in missing), (missing, unexpected)
    return model.eval()


def reference_logmel(wav):
    from oracle import ref_unise_shim as U

    mod = U._import_model_module()
    me = types.SimpleNamespace(stft_conf=dict(hop_length=320, win_length=640, n_fft=640, n_mels=80))  # conf/config.yaml:124-128
    return mod.Model.stft_logmel(me, wav)


@torch.no_grad()
def main():
    conf, llm = reference_modules()
    out = {}
    for name in R.CONFORMER_CASES:
        params, sd, x, mask = R.golden_conformer_case(name)
        enc = conf.ConformerEncoder(**params).eval()
        missing, unexpected = enc.load_state_dict(sd, strict=False)
        assert not unexpected and all(k.startswith("rotary_embedding") for k in missing)
        out[name] = enc(x.clone(), mask=mask).numpy()
    np.savez_compressed(os.path.join(GOLDEN, "lm_cond_conformer.npz"), **out)
    print("conformer:", {k: v.shape for k, v in out.items()})

    mel = reference_logmel(R.golden_logmel_wav())
    np.savez_compressed(os.path.join(GOLDEN, "lm_cond_logmel.npz"), logmel=mel.numpy().astype(np.float32))
    print("logmel:", tuple(mel.shape))

    spec, params, sd = R.GOLDEN_SPEC, R.GOLDEN_CF, R.golden_lm_weights()
    cond, g, s = R.golden_lm_inputs()
    G, Sn, B = R.GOLDEN_G, R.GOLDEN_S, R.GOLDEN_B
    model = reference_custom_llama(llm, spec, params, sd, 0.1)
    gen = {}
    for key, cd in (("cond", cond), ("nocond", None)):
        rows_g, rows_s = [], []
        for b in range(B if cd is not None else 1):  # the reference generates one sequence per call (llm.py:316)
            gi, si = model.generate(None if cd is None else cd[b:b + 1], global_length=G, semantic_length=Sn, do_sample=False)
            rows_g.append(gi[0])
            rows_s.append(si[0])
        gi, si = torch.stack(rows_g), torch.stack(rows_s)
        forced = torch.cat([gi + spec.global_offset, si + spec.semantic_offset], dim=1)
        cdr = None if cd is None else cd[:gi.shape[0]]
        _, _, toks, gaps = R.generate(sd, spec, params, cdr, G, Sn, gi.shape[0], forced=forced)
        assert torch.equal(toks, forced), key  # the restatement decides as the reference did, step by step
        assert float(gaps.min()) > TIE, (key, float(gaps.min()))
        gen[key + "_global"], gen[key + "_semantic"], gen[key + "_gap"] = gi.numpy().astype(np.int16), si.numpy().astype(np.int16), gaps.numpy().astype(np.float32)
        print(f"generate {key}: smallest top-2 gap {float(gaps.min()):.3e}")
    for b in range(B):
        assert not (np.array_equal(gen["cond_global"][b], gen["nocond_global"][0]) and np.array_equal(gen["cond_semantic"][b], gen["nocond_semantic"][0])), \
            "the conditional stream equals the unconditional one: scale the synthetic weights"
    np.savez_compressed(os.path.join(GOLDEN, "lm_cond_generate.npz"), **gen)

    fwd = {}
    for name, (with_cond, eps) in R.FORWARD_CASES.items():
        model.label_smoothing = eps
        loss, acc = model(g, s, cond if with_cond else None)
        fwd[name + "_loss"], fwd[name + "_acc"] = np.float32(loss), np.float32(acc)
        ours = R.score(sd, spec, params, g, s, cond if with_cond else None, eps)
        assert abs(ours["loss"] - float(loss)) <= 1e-5 * abs(float(loss)), (name, ours["loss"], float(loss))
        print(f"forward {name}: loss {float(loss):.6f} acc {float(acc):.4f}")
    np.savez_compressed(os.path.join(GOLDEN, "lm_cond_forward.npz"), **fwd)


if __name__ == "__main__":
    main()
