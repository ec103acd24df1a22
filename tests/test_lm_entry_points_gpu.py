"""The argument checks of the fourteen generate / score / prompt entry points of csrc/lm.cpp (qa_lm_generate and its _sampled, _ragged,
_cond variants, qa_lm_score / _ragged / _cond / _cond_ragged, qa_lm_prompt / _ragged), through ctypes on sentinel-filled outputs: every
refusal comes with its status and its exact message - the name the library has always printed for that entry point, the offending row,
value and bound - before any output is written and without touching the handle; of two simultaneous faults the one checked first is
reported; and full-width length vectors are the rectangular call, bit for bit.

Every expected string below is written out from the messages the library printed before the entry points were given one front per
family: the file passes unedited on the commit before that one.

Models: SMALL of tests/test_llm_gpu.py as an LLM_SFT (speech prompt) and as a CustomLlamaModel with SMALL_CF of tests/test_lm_cond_gpu.py
(condition prompt).  B = 3, n_mix = 4, n_enroll = 5, G = 2, S = T = 3, condition T = 4."""
import ctypes as C
import types

import pytest
import torch

from tests.test_llm_gpu import SMALL, _model
from tests.test_lm_cond_gpu import SMALL_CF, _custom, _weights

pytestmark = pytest.mark.gpu

B, NM, NE, G, S, TC = 3, 4, 5, 2, 3, 4
INVALID = -1  # QA_ERR_INVALID
SENTINEL = -(7 ** 20)  # no token, no count
SPEECH_GEN = ("qa_lm_generate", "qa_lm_generate_sampled", "qa_lm_generate_ragged", "qa_lm_generate_ragged_sampled")
COND_GEN = ("qa_lm_generate_cond", "qa_lm_generate_cond_sampled", "qa_lm_generate_cond_ragged", "qa_lm_generate_cond_ragged_sampled")
SCORE = ("qa_lm_score", "qa_lm_score_ragged", "qa_lm_score_cond", "qa_lm_score_cond_ragged")
PROMPT = ("qa_lm_prompt", "qa_lm_prompt_ragged")
ALL = SPEECH_GEN + COND_GEN + SCORE + PROMPT
SPEECH = SPEECH_GEN + ("qa_lm_score", "qa_lm_score_ragged") + PROMPT


def printed(name):
    """The name an entry point's messages carry: the _sampled functions report as their unsuffixed siblings."""
    return name[:-len("_sampled")] if name.endswith("_sampled") else name


class _Raw:
    """The fourteen entry points through ctypes on two handles; every call returns (status, qa_last_error())."""

    def __init__(self, lm, cm, dev):
        gen = torch.Generator().manual_seed(1234)
        self.lib, self.dev = lm._lib, dev
        self.models = (lm, cm)  # the handles below live as long as their models
        self.h_speech, self.h_cond = lm._handle, cm.lm._handle
        self.stream = torch.cuda.current_stream(dev).cuda_stream
        self.mix = torch.randn(B, NM, SMALL.feats_dim, generator=gen).to(dev)
        self.enr = torch.randn(B, NE, SMALL.feats_dim, generator=gen).to(dev)
        self.cond = torch.randn(B, TC, SMALL.hidden, generator=gen).to(dev)
        self.gin = torch.randint(0, SMALL.global_size, (B, G), generator=gen).to(dev)
        self.sin = torch.randint(0, SMALL.semantic_size, (B, S), generator=gen).to(dev)
        self.long_enr = torch.zeros(B, 4096, SMALL.feats_dim, device=dev)
        self.long_cond = torch.zeros(B, 4095, SMALL.hidden, device=dev)
        self.reset()

    def reset(self):
        d = self.dev
        self.gids = torch.full((B, G), SENTINEL, dtype=torch.int64, device=d)
        self.sids = torch.full((B, S), SENTINEL, dtype=torch.int64, device=d)
        self.loss_seq = torch.full((B,), float("inf"), device=d)
        self.correct = torch.full((B,), SENTINEL, dtype=torch.int64, device=d)
        self.out2 = torch.full((2,), float("inf"), device=d)
        self.prompt = torch.full((B, 1 + 1 + NE + 1 + NM, SMALL.hidden), float("inf"), device=d)

    def untouched(self):
        torch.cuda.synchronize()
        return (bool((self.gids == SENTINEL).all()) and bool((self.sids == SENTINEL).all()) and bool(torch.isinf(self.loss_seq).all())
                and bool((self.correct == SENTINEL).all()) and bool(torch.isinf(self.out2).all()) and bool(torch.isinf(self.prompt).all()))

    def outputs(self):
        torch.cuda.synchronize()
        return [t.clone() for t in (self.gids, self.sids, self.loss_seq, self.correct, self.out2, self.prompt)]

    def call(self, name, **kw):
        """`name` with valid arguments at the module's shapes, except what `kw` replaces.  The ragged entry points get non-uniform
        vectors unless told otherwise (n_enroll / n_mix / n_semantic / n_cond: a list, or None for a NULL vector)."""
        rag, cond = "_ragged" in name, "_cond" in name
        a = types.SimpleNamespace(task=0, enr=self.enr.data_ptr(), ne=NE, mix=self.mix.data_ptr(), nm=NM, cond=self.cond.data_ptr(), Tc=TC, B=B,
                                  G=G, S=S, temperature=0.8, top_k=50, top_p=0.95, seed=7, ls=0.1, gin=self.gin.data_ptr(),
                                  sin=self.sin.data_ptr(), gids=self.gids.data_ptr(), sids=self.sids.data_ptr(),
                                  loss_seq=self.loss_seq.data_ptr(), correct=self.correct.data_ptr(), loss=self.out2.data_ptr(),
                                  acc=self.out2[1:].data_ptr(), prompt=self.prompt.data_ptr(), n_enroll=[5, 3, 1], n_mix=[4, 2, 1],
                                  n_semantic=[3, 0, 2], n_cond=[4, 1, 3])
        vars(a).update(kw)
        vec = lambda v: None if v is None else (C.c_int64 * len(v))(*v)
        h = self.h_cond if cond else self.h_speech
        if "generate" in name:
            head = [a.cond, a.Tc] + ([vec(a.n_cond)] if rag else []) if cond else \
                [a.task, a.enr, a.ne] + ([vec(a.n_enroll)] if rag else []) + [a.mix, a.nm]
            args = head + [a.B, a.G, a.S, a.temperature, a.top_k, a.top_p] + ([a.seed] if name.endswith("_sampled") else []) + [a.gids, a.sids]
        elif "score" in name:
            head = [a.cond, a.Tc] + ([vec(a.n_cond)] if rag else []) if cond else \
                [a.task, a.enr, a.ne] + ([vec(a.n_enroll)] if rag else []) + [a.mix, a.nm] + ([vec(a.n_mix)] if rag else [])
            args = head + [a.B, a.gin, a.G, a.sin, a.S] + ([vec(a.n_semantic)] if rag else []) + [a.ls, a.loss_seq, a.correct, a.loss, a.acc]
        else:
            args = [a.task, a.enr, a.ne] + ([vec(a.n_enroll)] if rag else []) + [a.mix, a.nm] + ([vec(a.n_mix)] if rag else []) + [a.B, a.prompt]
        st = getattr(self.lib, name)(h, *args, self.stream)
        return st, self.lib.qa_last_error().decode("utf-8", "replace")


@pytest.fixture(scope="module")
def raw(qa_lib, gpu_device):
    _, lm = _model(SMALL, 91, gpu_device)
    sd = _weights(SMALL, SMALL_CF, 92)
    cm = _custom(SMALL, SMALL_CF, gpu_device).load_state_dict({"dnn." + k: v for k, v in sd.items()})
    return _Raw(lm, cm, gpu_device)


def null_arguments():
    """1. A required pointer null: the mixture features of the speech-prompt functions, an output of the others."""
    for name in ALL:
        kw = dict(mix=None) if name in SPEECH else dict(gids=None) if name in COND_GEN else dict(loss=None)
        yield name, kw, f"{printed(name)}: null argument"


def scalar_refusals():
    """2. One scalar out of range."""
    for name in SPEECH:
        yield name, dict(task=3), f"{printed(name)}: task 3 out of range (KeyError in the reference)"
        yield name, dict(ne=0), f"{printed(name)}: enrollment given with no frames"
    for name in SPEECH_GEN + COND_GEN:
        yield name, dict(temperature=0.0), f"{printed(name)}: temperature must be in (0, 1] (llm.py:278)"
        yield name, dict(top_p=0.0), f"{printed(name)}: bad top_k / top_p"
    for name in SCORE:
        yield name, dict(ls=1.5), f"{name}: label_smoothing 1.5 outside [0, 1]"
    for kw, T in ((dict(cond=None), 4), (dict(Tc=0), 0)):
        for name in COND_GEN:
            yield name, kw, f"{printed(name)}: cond_embeds [B, T, hidden] with T > 0, or NULL with T = 0 (got T = {T}); at least one step"
        yield "qa_lm_score_cond", kw, f"qa_lm_score_cond: cond_embeds [B, T, hidden] with T > 0, or NULL with T = 0 (got T = {T})"
        yield "qa_lm_score_cond_ragged", kw, (f"qa_lm_score_cond_ragged: cond_embeds [B, T_max, hidden] with T_max > 0, or NULL with T_max = 0 "
                                              f"(got T_max = {T}); bad shape otherwise")


def order_of_checks():
    """3. Two faults at once: the task is checked before the label smoothing and before the temperature."""
    yield "qa_lm_score", dict(task=3, ls=1.5), "qa_lm_score: task 3 out of range (KeyError in the reference)"
    yield "qa_lm_score_ragged", dict(task=3, ls=1.5), "qa_lm_score_ragged: task 3 out of range (KeyError in the reference)"
    yield "qa_lm_generate_ragged", dict(task=3, temperature=0.0), "qa_lm_generate_ragged: task 3 out of range (KeyError in the reference)"


def per_row_vectors(r):
    """4. One row below and one above range per vector, the vectors given without their tensor, the prompts that cannot fit."""
    for name in ("qa_lm_generate_ragged", "qa_lm_generate_ragged_sampled", "qa_lm_score_ragged", "qa_lm_prompt_ragged"):
        fn = printed(name)
        yield name, dict(n_enroll=[5, 0, 5]), f"{fn}: n_enroll[1] = 0 is outside 1 .. n_enroll_max = 5"
        yield name, dict(n_enroll=[5, 5, 6]), f"{fn}: n_enroll[2] = 6 is outside 1 .. n_enroll_max = 5"
    for name in ("qa_lm_score_ragged", "qa_lm_prompt_ragged"):
        yield name, dict(n_mix=[4, 0, 4]), f"{name}: n_mix[1] = 0 is outside 1 .. n_mix_max = 4"
        yield name, dict(n_mix=[4, 4, 5]), f"{name}: n_mix[2] = 5 is outside 1 .. n_mix_max = 4"
        yield name, dict(enr=None, ne=0), f"{name}: n_enroll given (n_enroll[0] = 5) without an enrollment (enroll_feats is NULL)"
    for name in ("qa_lm_generate_cond_ragged", "qa_lm_generate_cond_ragged_sampled", "qa_lm_score_cond_ragged"):
        fn = printed(name)
        yield name, dict(n_cond=[4, 0, 4]), f"{fn}: n_cond[1] = 0 is outside 1 .. T_max = 4"
        yield name, dict(n_cond=[4, 4, 5]), f"{fn}: n_cond[2] = 5 is outside 1 .. T_max = 4"
        yield name, dict(cond=None, Tc=0, n_cond=[1, 1, 1]), \
            f"{fn}: n_cond given (n_cond[0] = 1) without a condition (cond_embeds is NULL or T_max = 0)"
    for name in ("qa_lm_score_ragged", "qa_lm_score_cond_ragged"):
        yield name, dict(n_semantic=[3, -1, 3]), f"{name}: n_semantic[1] = -1 is outside 0 .. semantic_length_max = 3"
        yield name, dict(n_semantic=[3, 3, 4]), f"{name}: n_semantic[2] = 4 is outside 0 .. semantic_length_max = 3"
    for name in ("qa_lm_generate_ragged", "qa_lm_generate_ragged_sampled"):
        yield name, dict(enr=None, ne=0), \
            "qa_lm_generate_ragged: per-row enrollment lengths need enroll_feats [B, n_enroll_max, feats_dim] and n_enroll [B]"
        yield name, dict(enr=None, ne=0, n_enroll=None), \
            "qa_lm_generate_ragged: per-row enrollment lengths need enroll_feats [B, n_enroll_max, feats_dim] and n_enroll [B]"
        yield name, dict(enr=r.long_enr.data_ptr(), ne=4096, n_enroll=[4096, 1, 1]), \
            ("qa_lm_generate_ragged: 4109 positions (prompt 4103 with n_enroll_max 4096 and n_mix 4, + 2 + 1 + 3) exceed "
             "max_position_embeddings 4096")
    yield "qa_lm_generate_cond_ragged", dict(cond=r.long_cond.data_ptr(), Tc=4095, n_cond=[4095, 1, 1]), \
        "qa_lm_generate_cond_ragged: 4102 positions (prompt 1 + T_max 4095, + 2 + 1 + 3) exceed max_position_embeddings 4096"


def _refused(r, cases):
    r.reset()
    n = 0
    for name, kw, want in cases:
        st, msg = r.call(name, **kw)
        assert st == INVALID and msg == want, (name, kw, st, msg, want)
        assert r.untouched(), (name, kw)
        n += 1
    return n


def test_a_null_argument(raw):
    assert _refused(raw, null_arguments()) == 14


def test_a_scalar_out_of_range(raw):
    assert _refused(raw, scalar_refusals()) == 2 * 8 + 2 * 8 + 4 + 2 * 6


def test_of_two_faults_the_one_checked_first_is_reported(raw):
    assert _refused(raw, order_of_checks()) == 3


def test_a_per_row_vector_out_of_range(raw):
    assert _refused(raw, per_row_vectors(raw)) == 8 + 6 + 9 + 4 + 6 + 1


FULL = dict(n_enroll=[NE] * B, n_mix=[NM] * B, n_semantic=[S] * B, n_cond=[TC] * B)


def test_full_width_vectors_are_the_rectangular_call(raw):
    """5. Bit for bit, on every output; qa_lm_generate_ragged with full rows still runs as a ragged call and gives the same tokens.  NULL
    vectors are the rectangular call too."""
    for rect, ragged in (("qa_lm_score", "qa_lm_score_ragged"), ("qa_lm_score_cond", "qa_lm_score_cond_ragged"),
                         ("qa_lm_prompt", "qa_lm_prompt_ragged"), ("qa_lm_generate_cond", "qa_lm_generate_cond_ragged"),
                         ("qa_lm_generate", "qa_lm_generate_ragged")):
        raw.reset()
        st, msg = raw.call(rect)
        assert st == 0, (rect, msg)
        want = raw.outputs()
        assert not raw.untouched()
        variants = [FULL] if ragged == "qa_lm_generate_ragged" else [FULL, dict(n_enroll=None, n_mix=None, n_semantic=None, n_cond=None)]
        for kw in variants:
            raw.reset()
            st, msg = raw.call(ragged, **kw)
            assert st == 0, (ragged, msg)
            assert all(torch.equal(x, y) for x, y in zip(want, raw.outputs())), (ragged, kw)


def test_the_refusals_leave_the_handles_as_they_were(raw):
    """6. A valid greedy qa_lm_generate, qa_lm_score, qa_lm_score_ragged and qa_lm_generate_cond_ragged (the last two with rows of unequal
    lengths) give the same bits after the whole table of refusals as before it."""
    valid = ("qa_lm_generate", "qa_lm_score", "qa_lm_score_ragged", "qa_lm_generate_cond_ragged")

    def run():
        got = []
        for name in valid:
            raw.reset()
            st, msg = raw.call(name)
            assert st == 0, (name, msg)
            got.append(raw.outputs())
        return got

    before = run()
    for cases in (null_arguments(), scalar_refusals(), order_of_checks(), per_row_vectors(raw)):
        _refused(raw, cases)
    after = run()
    for name, x, y in zip(valid, before, after):
        assert all(torch.equal(p, q) for p, q in zip(x, y)), name
    assert int(before[0][0].min()) >= 0 and bool(torch.isfinite(before[1][2]).all()) and bool(torch.isfinite(before[2][2]).all())
