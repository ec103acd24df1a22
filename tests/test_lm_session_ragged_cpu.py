"""tests/lm_session_ragged_ref.py, the yardstick of the ragged session tests, against the batched oracle (no GPU).

On a schedule whose rows all have one length the per-row B = 1 runs of RowOracle and oracle.llm_ref.llm_forward over ONE cache of B rows
compute the same thing: a sequence's rows never mix with its neighbours'.  The two differ only in how the CPU's matrix products block a
batch of 1 and a batch of B, so they agree to a few roundings of their format: 64 eps relative to a row's rms (eps = 2^-52 / 2^-23; the
longest sum of these specs has 1024 terms, whose rounding error grows like sqrt(1024) = 32 eps).  Then the ragged bookkeeping: padding is
zero in the output and untouched in the input, idle rows do not advance, select copies."""
import torch

from oracle import llm_ref as L
from tests.lm_session_ragged_ref import DTYPES, RowOracle, row_err, valid_rows

SPEC = L.LMSpec(hidden=64, n_layers=2, n_heads=2, global_size=40, semantic_size=50, feats_dim=32, num_tasks=3)
EPS = {torch.float64: 2.0 ** -52, torch.float32: 2.0 ** -23}


def _embeds(sd, seed, B, n):
    gen = torch.Generator().manual_seed(seed)
    return sd["codec_embedding.weight"][torch.randint(0, SPEC.vocab, (B, n), generator=gen)].clone()


def test_row_oracle_equals_the_batched_oracle_on_an_equal_length_schedule():
    sd = L.lm_state_dict(3, SPEC)
    B, schedule = 3, [7, 1, 4, 1, 1]
    x = _embeds(sd, 4, B, sum(schedule))
    rows = RowOracle(sd, SPEC, B)
    batched = {t: L.KVCache(SPEC.n_layers) for t in DTYPES}
    pos = 0
    for n in schedule:
        chunk = x[:, pos:pos + n]
        got = rows(chunk)
        for t, h in zip(DTYPES, got):
            want = L.llm_forward(rows.sd[t], chunk.to(t), batched[t], SPEC, t)
            e = row_err(h, want)
            print(f"row oracle vs batched oracle, {t}, pos {pos} n {n}: {e:.3e} (bound {64 * EPS[t]:.3e})")
            assert h.dtype == t and e <= 64 * EPS[t], (t, pos, n, e)
        pos += n
    assert rows.lengths == [sum(schedule)] * B


def test_row_oracle_ragged_bookkeeping():
    sd = L.lm_state_dict(3, SPEC)
    x = _embeds(sd, 5, 3, 6)
    x_nan = x.clone()
    n = [2, 0, 6]
    for b, v in enumerate(n):
        x_nan[b, v:] = float("nan")
    a, b_ = RowOracle(sd, SPEC, 3), RowOracle(sd, SPEC, 3)
    h = a(x, n)
    h_nan = b_(x_nan, n)
    for u, w in zip(h, h_nan):
        assert torch.equal(u, w), "the input behind a row's count is never read"
        assert all(bool((u[r, v:] == 0).all()) for r, v in enumerate(n)) and torch.isfinite(u).all()
    assert a.lengths == [2, 0, 6]
    # a row fed in two ragged calls equals the row fed alone in one rectangular call per chunk
    solo = RowOracle(sd, SPEC, 1)
    first = solo(x[0:1, :2])
    more = _embeds(sd, 6, 3, 3)
    second = a(more, [3, 1, 0])
    second_solo = solo(more[0:1])
    for u, w in zip(second, second_solo):
        assert torch.equal(u[0], w[0])
    assert torch.equal(valid_rows(h[0], n)[:2], first[0][0])
    # select copies: continuing a selected row leaves its source as it was
    a.select([2, 2, 0])
    assert a.lengths == [6, 6, 5] and a.B == 3
    step = _embeds(sd, 7, 3, 1)
    step[1] = step[0]
    out = a(step, [1, 0, 1])
    assert a.lengths == [7, 6, 6]
    again = a(step, [0, 1, 0])
    assert torch.equal(out[0][0], again[0][1]) and torch.equal(out[1][0], again[1][1]), "rows 0 and 1 were the same sequence"
