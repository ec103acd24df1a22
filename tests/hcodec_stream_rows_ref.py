"""Per-row lengths, offsets and resets of the H-Codec 1.0 stream, restated on the CPU: a schedule driver over
tests/hcodec_stream_ref.step in which every row of a batch owns a streaming state, steps only when the schedule gives it frames, and
starts over when it is reset.  A row between two of its resets is a SEGMENT; the definition of correct is that a segment's concatenated
outputs equal one offline causal encode of the segment's own waveform.

Also here: the schedule, seeds and waveforms that tests/test_hcodec_stream_rows_cpu.py and tests/test_hcodec_stream_rows_gpu.py share, so
that the near-tie condition the CPU test asserts is the condition of the very inputs the GPU test compares codes on.
"""
import torch

from oracle import hcodec_ref as R
from oracle import synth
from tests import hcodec_stream_ref as S
from tests import transformer_stream_ref as TR

# code frames per step for rows 0 .. 3; RESETS[s]: the rows reset in front of step s
SCHEDULE = ((2, 0, 3, 0), (2, 0, 1, 2), (2, 0, 0, 1), (2, 2, 2, 1), (2, 2, 2, 1), (2, 2, 1, 0), (1, 2, 1, 3), (1, 2, 1, 1))
RESETS = {4: (2,)}
DELAY = 3  # row 1 carries row 0's waveform, three steps late
GPU_ROWS_CASE = dict(seed=11, wav_seed=61)


def segments(schedule=SCHEDULE, resets=RESETS):
    """[(row, [(step, frames), ...]), ...]: every row's segments in order, the idle steps left out."""
    B = len(schedule[0])
    out = []
    for b in range(B):
        cur = []
        for s, fr in enumerate(schedule):
            if b in resets.get(s, ()) and cur:
                out.append((b, cur))
                cur = []
            if fr[b] > 0:
                cur.append((s, fr[b]))
        if cur:
            out.append((b, cur))
    return out


def segment_waves(case, spec, schedule=SCHEDULE, resets=RESETS):
    """One waveform [1, 1, frames * hop] per segment; row 1's is the head of row 0's (the delayed duplicate)."""
    segs = segments(schedule, resets)
    longest = max(sum(f for _, f in steps) for _, steps in segs)
    pool = synth.synth_wav(case["wav_seed"], len(segs), longest * spec.enc_hop).unsqueeze(1)
    waves = []
    for i, (b, steps) in enumerate(segs):
        src = 0 if b == 1 else i
        waves.append(pool[src:src + 1, :, :sum(f for _, f in steps) * spec.enc_hop].clone())
    return segs, waves


def case_inputs(case, spec_kwargs):
    ospec = R.HCodecSpec(**spec_kwargs)
    sd = synth.hcodec10_state_dict(case["seed"], ospec)
    segs, waves = segment_waves(case, ospec)
    return ospec, sd, segs, waves


def run_schedule(sd, spec, segs, waves, dtype):
    """Every segment through a streaming state of its own, in the chunks the schedule gives it: [emb [1, D, frames], ...]."""
    sd = TR.cast(sd, dtype)
    out = []
    for (b, steps), wav in zip(segs, waves):
        state, t, parts = S.State(spec), 0, []
        for _, n in steps:
            parts.append(S.step(sd, wav[..., t * spec.enc_hop:(t + n) * spec.enc_hop].to(dtype), spec, state))
            t += n
        assert t * spec.enc_hop == wav.shape[-1]
        out.append(torch.cat(parts, -1))
    return out


def rectangles(spec, segs, waves, schedule=SCHEDULE, fill=float("nan")):
    """The batch's view of the schedule: per step (x [B, 1, n * hop], lengths), every sample behind a row's frames set to `fill`.  n is
    the longest entry of the whole schedule in EVERY step: rows 0 and 1 are to consume the same chunks in rectangles of the same width."""
    B, hop = len(schedule[0]), spec.enc_hop
    width = max(max(fr) for fr in schedule)
    steps_x = [torch.full((B, 1, width * hop), fill) for fr in schedule]
    for (b, steps), wav in zip(segs, waves):
        t = 0
        for s, n in steps:
            steps_x[s][b, 0, :n * hop] = wav[0, 0, t * hop:(t + n) * hop]
            t += n
    return [(x, list(fr)) for x, fr in zip(steps_x, schedule)]
