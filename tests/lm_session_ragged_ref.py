"""The truth of a ragged session (qa_lm_forward_ragged): row b is oracle.llm_ref.llm_forward over a B = 1 oracle
cache OF ITS OWN, fed that row's valid positions call by call, idle calls skipped - in float64 (the truth) and in float32 (the yardstick),
as _Oracle in tests/test_lm_session_gpu.py does for a rectangular batch.  Shared by tests/test_lm_session_ragged_cpu.py (which pins it
against the batched oracle) and tests/test_lm_session_ragged_gpu.py."""
import torch

from oracle import llm_ref as L

DTYPES = (torch.float64, torch.float32)


class RowOracle:
    def __init__(self, sd, spec, B):
        self.spec, self.B = spec, B
        self.sd = {torch.float32: sd, torch.float64: {k: v.double() for k, v in sd.items()}}
        self.cache = {t: [L.KVCache(spec.n_layers) for _ in range(B)] for t in DTYPES}
        self.lengths = [0] * B

    def select(self, idx):
        """Row j becomes a COPY of old row idx[j] (KVCache.batch_select_indices)."""
        for t in DTYPES:
            old = self.cache[t]
            new = []
            for i in idx:
                c = L.KVCache(self.spec.n_layers)
                c.k = [None if k is None else k.clone() for k in old[i].k]
                c.v = [None if v is None else v.clone() for v in old[i].v]
                new.append(c)
            self.cache[t] = new
        self.lengths = [self.lengths[i] for i in idx]
        self.B = len(idx)

    def __call__(self, x, n=None):
        """x [B, n_max, hidden] (fp32, host), n: the rows' counts (None: every row takes all n_max).  -> (h64, h32), each [B, n_max,
        hidden] in its dtype with exact zeros behind a row's count - what the ragged call must write there.  The input behind a row's
        count is never touched."""
        B, n_max, _ = x.shape
        assert B == self.B
        n = [n_max] * B if n is None else [int(v) for v in n]
        out = []
        for t in DTYPES:
            h = torch.zeros(x.shape, dtype=t)
            for b in range(B):
                if n[b] > 0:
                    h[b, :n[b]] = L.llm_forward(self.sd[t], x[b:b + 1, :n[b]].to(t), self.cache[t][b], self.spec, t)[0]
            out.append(h)
        self.lengths = [l + v for l, v in zip(self.lengths, n)]
        return out


def row_err(h, truth):
    """max over rows of max |h - truth| / rms(truth): _row_err of tests/test_lm_session_gpu.py on rows that exist."""
    truth = truth.double()
    rms = truth.pow(2).mean(-1).sqrt()
    return float(((h.double() - truth).abs().amax(-1) / rms).max())


def valid_rows(t, n):
    """The rows a ragged call computed, concatenated: [sum(n), hidden] of t [B, n_max, hidden]."""
    return torch.cat([t[b, :int(v)] for b, v in enumerate(n)], dim=0)
