"""Segmenting / batching driver of the UniSE inference step, in front of the HIP paths of this package.

    UniSE.enhance_tokens(mode, src, enroll)  <->  Model.test_step, 'se' and 'tse' branches
                                                  (QuarkAudio-UniSE/model/model.py:170-222): wrap-pad to a multiple of 5 s,
                                                  cut into 5 s segments, (se: divide by the utterance peak), WavLM
                                                  features, LLM_SFT.generate -> (global_ids, semantic_ids)

The reference handles ONE utterance per call (`batch_size == 1`, dataloader/data_module.py:340); here any number of
utterances is accepted: their segments are concatenated into one batch for the front-end and the LM (segments are
independent), and the results are handed back per utterance.  The last stage of `test_step` - BiCodec `detokenize` - is
`unified_audio_amd.BiCodecTokenizer`: with it `UniSE.enhance` returns waveforms for 'se', 'tse' and the three-pass
'ss' mode (model.py:223-290); without it `enhance_tokens` returns the tokens.
"""
from __future__ import annotations

import inspect
import math
from typing import Callable, List, Optional, Sequence, Tuple

import torch

SEG_LEN = 5 * 16000        # model.py:176
HOP_LENGTH = 320           # conf/config.yaml:124-128 (stft_config)
WIN_LENGTH = 640
MIN_TAIL = 16000           # UniSE(tail="trim"): the shortest last segment, in samples


def wrap_pad(src: torch.Tensor, multiple: int = SEG_LEN) -> torch.Tensor:
    """np.pad(src, [(0,0),(0,pad_len)], 'wrap') of model.py:177-178: the utterance repeats itself to the next multiple."""
    T = src.size(-1)
    pad_len = math.ceil(T / multiple) * multiple - T
    if pad_len == 0:
        return src
    reps = math.ceil(pad_len / T)
    return torch.cat([src] + [src] * reps, dim=-1)[..., : T + pad_len]


def segment(src: torch.Tensor, normalise: bool) -> torch.Tensor:
    """src [1, T] -> seg_src [ceil(T / 80000), 80000] (model.py:176-182).  normalise = the 'se' branch: every segment is divided
    by the peak of the WHOLE utterance (`src.abs().max(dim=-1)`), the 'tse' branch does not normalise (model.py:199-203)."""
    if src.dim() != 2 or src.size(0) != 1:
        raise ValueError(f"src must be [1, T] like the reference's batch, got {tuple(src.shape)}")
    seg = wrap_pad(src).reshape(-1, SEG_LEN)
    if normalise:
        seg = seg / src.abs().max(dim=-1, keepdim=True)[0]
    return seg


def trim_samples(T: int, min_tail: int = MIN_TAIL) -> List[int]:
    """The sample counts of the segments UniSE(tail="trim") cuts an utterance of T samples into: its full 5 s segments, then one last
    segment of T mod 80000 samples - at least `min_tail`, an utterance that ends sooner wraps around as far."""
    full, rem = divmod(int(T), SEG_LEN)
    return [SEG_LEN] * full + ([max(rem, min_tail)] if rem or not full else [])


def segment_trim(src: torch.Tensor, normalise: bool, min_tail: int = MIN_TAIL) -> Tuple[torch.Tensor, List[int]]:
    """`segment` without the wrap-padding to a multiple of 5 s: src [1, T] -> (seg_src [n, 80000], the n rows' sample counts
    `trim_samples(T)`).  The last row holds its samples in front and zeros behind them.  A last segment shorter than `min_tail` is
    wrap-padded up to it the way the reference wraps to 80000: the utterance repeats itself.  normalise as in `segment`: the peak of the
    WHOLE utterance."""
    if src.dim() != 2 or src.size(0) != 1:
        raise ValueError(f"src must be [1, T] like the reference's batch, got {tuple(src.shape)}")
    samples = trim_samples(src.size(-1), min_tail)
    total = sum(samples)
    x = torch.cat([src] * math.ceil(total / src.size(-1)), dim=-1)[..., :total]
    seg = x.new_zeros((len(samples), SEG_LEN))
    seg.reshape(-1)[:total] = x[0]
    if normalise:
        seg = seg / src.abs().max(dim=-1, keepdim=True)[0]
    return seg, samples


def mel_frames(n_samples: int) -> int:
    """Number of frames `stft_logmel` (model.py:53-79) yields - the only property of the mel the LM consumes
    (llm_sft.py:108): the signal is padded to a multiple of the hop plus (win - hop) in total, center=False."""
    padded = math.ceil(n_samples / HOP_LENGTH) * HOP_LENGTH + (WIN_LENGTH - HOP_LENGTH)
    return (padded - WIN_LENGTH) // HOP_LENGTH + 1


def mel_frames_for(n_samples: int, hop_length: int, win_length: int) -> int:
    """`mel_frames` for any hop / window"""
    padded = math.ceil(n_samples / hop_length) * hop_length + (win_length - hop_length)
    return (padded - win_length) // hop_length + 1


class _Frames:
    """Stand-in for a mel tensor: LLM_SFT.generate only calls `.size(1)` on it, LLM_SFT.forward only `.size(0)`."""

    def __init__(self, batch: int, frames: int):
        self._shape = (batch, frames, 80)

    def size(self, dim: int) -> int:
        return self._shape[dim]


def stft_logmel(x: torch.Tensor, hop_length: int = HOP_LENGTH, win_length: int = WIN_LENGTH, n_fft: int = 640, n_mels: int = 80,
                lengths=None) -> torch.Tensor:
    """Model.stft_logmel (model.py:53-79), restated with the filter bank of torchaudio.functional.melscale_fbanks (HTK scale, no
    normalisation, 0-8000 Hz).  LLM_SFT.generate consumes only `mel.size(1)` (llm_sft.py:108), which `mel_frames()` gives without
    computing anything; CustomLlamaModel's condition encoder consumes the values.  A CUDA input runs on the device (qa_logmel: the
    framed-signal DFT GEMM); a CPU input keeps this torch restatement.

    lengths (B sample counts in 1 .. x.size(1), None: every row is full): out[b, :F_b], F_b = mel_frames_for(lengths[b], ...), is the
    log-mel of x[b:b+1, :lengths[b]] alone and out[b, F_b:] is exactly 0; samples behind a row's length are never used.  Device inputs in
    the configuration qa_logmel serves only (qa_logmel_ragged)."""
    assert x.ndim == 2
    # the condition encoder's input (CustomLlamaModel): computed on the device by qa_logmel where its framed-signal DFT serves the
    # configuration (win = 2 hop, hop a multiple of 16, n_mels a multiple of 4); any other configuration keeps the torch path below
    if x.is_cuda and win_length == 2 * hop_length and hop_length % 16 == 0 and n_fft >= win_length and (n_fft - win_length) % 2 == 0 \
            and n_mels % 4 == 0:
        from . import _lib

        lib = _lib.load_library()
        xc = x.to(torch.float32).contiguous()
        out = torch.empty((xc.shape[0], mel_frames_for(xc.shape[1], hop_length, win_length), n_mels), dtype=torch.float32, device=x.device)
        _, lens = _lib.host_lengths("stft_logmel: lengths", lengths, xc.shape[0])
        with torch.cuda.device(x.device):
            if lens is not None:
                _lib.check(lib.qa_logmel_ragged(xc.data_ptr(), lens, xc.shape[0], xc.shape[1], n_fft, win_length, hop_length, n_mels, 16000,
                                                0.0, 8000.0, out.data_ptr(), torch.cuda.current_stream(x.device).cuda_stream))
                return out
            _lib.check(lib.qa_logmel(xc.data_ptr(), xc.shape[0], xc.shape[1], n_fft, win_length, hop_length, n_mels, 16000, 0.0, 8000.0,
                                     out.data_ptr(), torch.cuda.current_stream(x.device).cuda_stream))
        return out
    if lengths is not None:
        raise ValueError("stft_logmel: lengths need a device input in the configuration qa_logmel serves (win = 2 hop, hop % 16 == 0)")
    pad_length = math.ceil(x.size(-1) / hop_length) * hop_length - x.size(-1)
    x = torch.nn.functional.pad(x, ((win_length - hop_length) // 2, pad_length + (win_length - hop_length) // 2))
    spec = torch.stft(x, n_fft, hop_length, win_length=win_length, window=torch.hann_window(win_length, device=x.device), onesided=True,
                      center=False, return_complex=True).transpose(1, 2)
    n_freqs = n_fft // 2 + 1
    all_freqs = torch.linspace(0, 16000 // 2, n_freqs)
    hz2mel = lambda f: 2595.0 * math.log10(1.0 + f / 700.0)  # noqa: E731
    m_pts = torch.linspace(hz2mel(0.0), hz2mel(8000.0), n_mels + 2)
    f_pts = 700.0 * (10.0 ** (m_pts / 2595.0) - 1.0)
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts.unsqueeze(0) - all_freqs.unsqueeze(1)
    down, up = -slopes[:, :-2] / f_diff[:-1], slopes[:, 2:] / f_diff[1:]
    fb = torch.clamp(torch.minimum(down, up), min=0.0).to(x.device)
    return torch.log(spec.abs() @ fb + 1e-10)


class UniSE:
    def __init__(self, dnn, semantic_model, tokenizer=None, detokenize: Optional[Callable] = None, max_segments: int = 64,
                 tail: str = "wrap", min_tail: int = MIN_TAIL):
        """dnn: unified_audio_amd.LLM_SFT; semantic_model: unified_audio_amd.SSLFeatureExtractor(SPEC_WAVLM_BASE_PLUS);
        tokenizer: unified_audio_amd.BiCodecTokenizer (or any object / callable with the reference's
        `detokenize(global_tokens [B, 1, 32], semantic_tokens [B, N]) -> wav [B, 1, t]`, model.py:193).
        max_segments: 5 s segments per pass through the three stages (the micro-batch).  The reference feeds one utterance per step
        (data_module.py:340); here all segments of a call are batched, 64 at a time: the LM's decode step costs about the same for 16
        and for 64 sequences (one chain, two row groups per launch: 92 k tok/s against 41 k at 16), memory stays
        bounded for long file lists, and - every stage being batch-invariant - the result does not depend on the value.
        tail: "wrap" (the default) is the reference's behaviour: every utterance is wrap-padded to a multiple of 5 s (model.py:177-178), so
        a 2 s utterance pays for a 5 s prompt and 250 semantic steps.  "trim" is opt-in and DEVIATES from the reference: an utterance of
        T samples gives its full 5 s segments plus one last segment of T mod 80000 samples that runs at its own length through all three
        stages - semantic_model(seg, lengths=), generate(mix_lengths=, semantic_lengths=), detokenize(lengths=) -
        so the last segment is modelled WITHOUT the repeated start of the utterance behind it and its tokens differ from the
        reference's.  A last segment shorter than `min_tail` samples is wrap-padded up to `min_tail`; 'se' still divides by the whole
        utterance's peak; the 'ss' mode keeps "wrap".  It needs an LM, a front-end and a detokenizer that take per-row lengths."""
        self.dnn = dnn
        self.semantic_model = semantic_model
        self.detokenize = detokenize if detokenize is not None else (tokenizer.detokenize if tokenizer is not None else None)
        self.max_segments = max(1, int(max_segments))
        # per-row enrollment lengths (LLM_SFT.generate's `enroll_lengths`) are this package's extension: an LM with
        # the reference's own signature (the reference's LLM_SFT module behind the same driver, tests/test_file_boundary_cpu.py) cannot
        # take them and keeps one pass per enrollment length
        try:
            params = inspect.signature(dnn.generate).parameters.values()
            self._ragged_ok = any(p.name == "enroll_lengths" or p.kind is inspect.Parameter.VAR_KEYWORD for p in params)
        except (AttributeError, TypeError, ValueError):
            self._ragged_ok = False
        # the same for the front-end: SSLFeatureExtractor.__call__(wavs, lengths=...) runs enrollments of different
        # lengths in one call, every row as the clip alone; it also needs `frames(samples)` for the rows' frame counts.  Any other
        # front-end keeps one pass per distinct length
        try:
            params = inspect.signature(semantic_model.__call__).parameters.values()
            self._ssl_ragged_ok = any(p.name == "lengths" for p in params) and callable(getattr(semantic_model, "frames", None))
        except (AttributeError, TypeError, ValueError):
            self._ssl_ragged_ok = False
        if tail not in ("wrap", "trim"):
            raise ValueError(f"tail must be 'wrap' or 'trim', got {tail!r}")
        self.tail, self.min_tail = tail, int(min_tail)
        if tail == "trim":
            if not 1 <= self.min_tail <= SEG_LEN:
                raise ValueError(f"min_tail must be 1 .. {SEG_LEN} samples, got {min_tail}")

            def takes(fn, *names):
                try:
                    params = list(inspect.signature(fn).parameters.values())
                except (AttributeError, TypeError, ValueError):
                    return False
                return any(p.kind is inspect.Parameter.VAR_KEYWORD for p in params) or all(any(p.name == n for p in params) for n in names)

            missing = []
            if not (self._ragged_ok and takes(getattr(dnn, "generate", None), "mix_lengths", "semantic_lengths")):
                missing.append("dnn.generate(..., enroll_lengths=, mix_lengths=, semantic_lengths=)")
            if not self._ssl_ragged_ok:
                missing.append("semantic_model(wavs, lengths=) with frames(n_samples)")
            if self.detokenize is not None and not takes(self.detokenize, "lengths"):
                missing.append("detokenize(global_tokens, semantic_tokens, lengths=)")
            if missing:
                raise TypeError("UniSE(tail='trim') runs the last segment at its own length and needs " + "; ".join(missing))

    def _generate(self, mode: str, seg_src: torch.Tensor, counts: Sequence[int], enroll_feats_per_utt: Optional[torch.Tensor],
                  enroll_samples: int, enroll_frames: Optional[Sequence[int]] = None, samples: Optional[Sequence[int]] = None):
        """enroll_frames (enrollments of different lengths): the valid feature frames of every row of enroll_feats_per_utt, which is
        then zero-padded to the longest; None: every row is valid throughout.
        samples (tail="trim"): every segment's own sample count; the semantic ids then come back [n, 250] with -1 behind a row's
        mel_frames(samples) tokens."""
        m = self.max_segments
        if seg_src.size(0) > m:  # micro-batches of <= max_segments segments; a segment's utterance is looked up through `owner`
            owner = torch.repeat_interleave(torch.arange(len(counts)), torch.tensor(list(counts)))
            gs, ss = [], []
            for a in range(0, seg_src.size(0), m):
                own = owner[a:a + m]
                utts, sub_counts = torch.unique_consecutive(own, return_counts=True)
                ef = enroll_feats_per_utt[utts.to(enroll_feats_per_utt.device)] if enroll_feats_per_utt is not None else None
                frames = [enroll_frames[i] for i in utts.tolist()] if enroll_frames is not None else None
                g, sids = self._generate(mode, seg_src[a:a + m], sub_counts.tolist(), ef, enroll_samples, frames,
                                         samples[a:a + m] if samples is not None else None)
                gs.append(g)
                ss.append(sids)
            return torch.cat(gs, dim=0), torch.cat(ss, dim=0)
        ragged = {}
        if samples is not None and any(n != SEG_LEN for n in samples):
            # a micro-batch with a trimmed last segment: every stage at the rows' own lengths, the tensors at the longest row's
            seg_src, mix_feats, mix_mel, ragged = self._trimmed_inputs(seg_src, samples)
        else:
            mix_feats = self.semantic_model(seg_src)                               # extract_semantic_features, model.py:38-51
            mix_mel = _Frames(seg_src.size(0), mel_frames(SEG_LEN))
        enroll_mel = enroll_feats = None
        if enroll_feats_per_utt is not None:
            if enroll_frames is not None:  # this micro-batch's longest enrollment bounds its prompt, not the call's
                enroll_feats_per_utt = enroll_feats_per_utt[:, :max(enroll_frames)]
                if len(set(enroll_frames)) > 1:
                    # one generate call over rows of different prompt lengths (LLM_SFT.generate enroll_lengths):
                    # every segment carries its utterance's frame count, and the padding behind it is never read
                    ragged["enroll_lengths"] = [n for n, c in zip(enroll_frames, counts) for _ in range(c)]
            # model.py:207-210: the utterance's enrollment is tiled over its segments
            enroll_feats = torch.cat([enroll_feats_per_utt[i:i + 1].expand(c, -1, -1) for i, c in enumerate(counts)], dim=0).contiguous()
            enroll_mel = _Frames(seg_src.size(0), mel_frames(enroll_samples))
        g, sids = self.dnn.generate(task_name=mode, enroll_mel=enroll_mel, enroll_feats=enroll_feats, mix_mel=mix_mel, mix_feats=mix_feats,
                                    do_sample=False, **ragged)
        return g, (self._full_width(sids) if samples is not None else sids)

    def _trimmed_inputs(self, seg_src: torch.Tensor, samples: Sequence[int]):
        """The front-end and the LM's length arguments for segments of `samples` samples each (tail="trim"): (the segments cut to the
        longest row, its features [B, frames(longest), d], the mel stand-in at the longest row's step count, generate's keywords)."""
        samples = [int(n) for n in samples]
        seg_src = seg_src[:, :max(samples)].contiguous()
        mix_feats = self.semantic_model(seg_src, lengths=samples)
        steps = [mel_frames(n) for n in samples]
        lens = dict(mix_lengths=[int(self.semantic_model.frames(n)) for n in samples], semantic_lengths=steps)
        return seg_src, mix_feats, _Frames(seg_src.size(0), max(steps)), lens

    @staticmethod
    def _full_width(sids: torch.Tensor) -> torch.Tensor:
        """semantic ids [B, S] of a micro-batch whose longest row is shorter than 5 s -> [B, 250], -1 behind"""
        full = mel_frames(SEG_LEN)
        return sids if sids.size(1) == full else torch.nn.functional.pad(sids, (0, full - sids.size(1)), value=-1)

    def _enroll_features(self, enrolls: Sequence[torch.Tensor]):
        """The SSL features of one enrollment per utterance -> ([U, N_e, d], samples, frames).  Equal lengths: one front-end pass, frames
        None.  Different lengths: the front-end is not causal, so zero-padding a waveform would change its features.  A front-end that
        takes per-clip `lengths` runs them in ONE call, every row as the enrollment alone (bit for bit, tests/test_ssl_ragged_gpu.py) with
        zeros behind its frames.  Any other runs once per DISTINCT length (every utterance keeps its own enrollment length, as in the
        reference's one-file-per-step loop, model.py:197-219) and the features are zero-padded to the longest.  Either way `frames` holds
        every utterance's own count for the LM's ragged call."""
        lens = [int(e.size(-1)) for e in enrolls]
        if len(set(lens)) == 1:
            return self.semantic_model(torch.cat(list(enrolls), dim=0)), lens[0], None
        if self._ssl_ragged_ok:
            wav = enrolls[0].new_zeros((len(enrolls), max(lens)))
            for i, e in enumerate(enrolls):
                wav[i, :lens[i]] = e[0]
            return self.semantic_model(wav, lengths=lens), max(lens), [int(self.semantic_model.frames(n)) for n in lens]
        feats: List[Optional[torch.Tensor]] = [None] * len(enrolls)
        for n in sorted(set(lens)):
            idx = [i for i, v in enumerate(lens) if v == n]
            f = self.semantic_model(torch.cat([enrolls[i] for i in idx], dim=0))
            for j, i in enumerate(idx):
                feats[i] = f[j]
        frames = [int(f.size(0)) for f in feats]
        ef = feats[0].new_zeros((len(feats), max(frames), feats[0].size(-1)))
        for i, f in enumerate(feats):
            ef[i, :frames[i]] = f
        return ef, max(lens), frames

    @staticmethod
    def _split(counts, *tensors):
        out, at = [], 0
        for c in counts:
            out.append(tuple(t[at:at + c] for t in tensors))
            at += c
        return out

    @torch.no_grad()
    def enhance_tokens(self, mode: str, srcs: Sequence[torch.Tensor], enrolls: Optional[Sequence[torch.Tensor]] = None
                       ) -> List[Tuple[torch.Tensor, torch.Tensor]]:
        """srcs: utterances [1, T_i] (device tensors); enrolls (tse / rtse): one [1, T_e_i] per utterance (any lengths).
        Returns per utterance (global_ids [n_seg_i, 32], semantic_ids [n_seg_i, 250]); with tail="trim" the last row of an utterance
        holds mel_frames(its samples) ids and -1 behind them."""
        if mode not in ("se", "tse", "rtse"):
            raise KeyError(mode)
        if mode != "se":
            if enrolls is None or len(enrolls) != len(srcs):
                raise ValueError(f"{mode} needs one enrollment per utterance")
            lens = [int(e.size(-1)) for e in enrolls]
            if len(set(lens)) > 1 and not self._ragged_ok:
                # an LM without `enroll_lengths`: the prompt length of its generate call is common to the batch, so utterances are grouped
                # by enrollment length (each keeps ITS length, model.py:197-219), one pass per group, handed back in the caller's order
                out: List[Optional[Tuple[torch.Tensor, torch.Tensor]]] = [None] * len(srcs)
                for n in sorted(set(lens)):
                    idx = [i for i, v in enumerate(lens) if v == n]
                    for i, r in zip(idx, self.enhance_tokens(mode, [srcs[i] for i in idx], [enrolls[i] for i in idx])):
                        out[i] = r
                return out  # type: ignore[return-value]
        segs, counts, samples = self._segments(mode, srcs)
        seg_src = torch.cat(segs, dim=0)
        ef, n_enr, frames = None, 0, None
        if mode != "se":
            # enrollments of different lengths no longer split the LM pass into one group per length: the features are padded to the
            # longest and the segments of ALL utterances go through one ragged generate per micro-batch
            ef, n_enr, frames = self._enroll_features(enrolls)                    # [U, N_e, d]
        global_ids, semantic_ids = self._generate(mode, seg_src, counts, ef, n_enr, frames, samples)
        return self._split(counts, global_ids, semantic_ids)

    def _segments(self, mode: str, srcs: Sequence[torch.Tensor]):
        """The utterances' segments, their counts and - tail="trim" only, else None - every segment's own sample count"""
        if self.tail == "trim":
            cut = [segment_trim(s, normalise=(mode == "se"), min_tail=self.min_tail) for s in srcs]
            return [c[0] for c in cut], [len(c[1]) for c in cut], [n for c in cut for n in c[1]]
        segs = [segment(s, normalise=(mode == "se")) for s in srcs]
        return segs, [s.size(0) for s in segs], None

    def _wave(self, src: torch.Tensor, gids: torch.Tensor, sids: torch.Tensor) -> torch.Tensor:
        est = self.detokenize(gids.unsqueeze(1), sids).squeeze(1)                 # model.py:192
        return est.reshape(-1)[: src.size(-1)]

    def _detokenize_rows(self, g: torch.Tensor, s: torch.Tensor, samples: Sequence[int]) -> List[torch.Tensor]:
        """One detokenize call over a micro-batch of tail="trim": row i's waveform over its own samples[i] samples"""
        steps = [mel_frames(int(n)) for n in samples]
        if all(n == SEG_LEN for n in samples):
            est = self.detokenize(g.unsqueeze(1), s).squeeze(1)
        else:
            est = self.detokenize(g.unsqueeze(1), s[:, :max(steps)].contiguous(), lengths=steps).squeeze(1)
        return [est[i, :int(n)] for i, n in enumerate(samples)]

    @torch.no_grad()
    def enhance(self, mode: str, srcs: Sequence[torch.Tensor], enrolls: Optional[Sequence[torch.Tensor]] = None):
        """Model.test_step up to the waveform (model.py:170-290).  'se' / 'tse': one tensor [T_i] per utterance
        (`est.reshape(-1)[:src.size(-1)]`); 'ss': a pair (s1, s2) per utterance - SE on the first 5 s gives the enrollment, then TSE
        (speaker 1) and rTSE (speaker 2) over all segments (model.py:223-290)."""
        if self.detokenize is None:
            raise RuntimeError("UniSE.enhance needs a tokenizer (unified_audio_amd.BiCodecTokenizer) or a detokenize callable; "
                               "enhance_tokens returns the tokens")
        if mode == "ss":
            return self._separate(srcs)
        toks = self.enhance_tokens(mode, srcs, enrolls)
        return self._waves(srcs, toks, trim=self.tail == "trim")

    def _waves(self, srcs, toks, trim: bool = False):
        """model.py:192 for every utterance, with ONE detokenize call over all segments (segments are independent and the detokenizer
        is batch-invariant, so this equals the reference's per-utterance calls bit for bit).  trim (tail="trim"): every row over its own
        samples, an utterance's rows concatenated and cut to its length."""
        g = torch.cat([t[0] for t in toks], dim=0)
        s = torch.cat([t[1] for t in toks], dim=0)
        m = self.max_segments
        if trim:
            samples = [n for src in srcs for n in trim_samples(src.size(-1), self.min_tail)]
            rows = [w for a in range(0, g.size(0), m) for w in self._detokenize_rows(g[a:a + m], s[a:a + m], samples[a:a + m])]
            return self._join_rows(srcs, [t[0].size(0) for t in toks], rows)
        est = torch.cat([self.detokenize(g[a:a + m].unsqueeze(1), s[a:a + m]).squeeze(1) for a in range(0, g.size(0), m)], dim=0)
        out, at = [], 0
        for src, (gi, _) in zip(srcs, toks):
            out.append(est[at:at + gi.size(0)].reshape(-1)[: src.size(-1)])
            at += gi.size(0)
        return out

    @staticmethod
    def _join_rows(srcs, counts, rows: List[torch.Tensor]):
        out, at = [], 0
        for src, c in zip(srcs, counts):
            out.append(torch.cat(rows[at:at + c])[: src.size(-1)])
            at += c
        return out

    @torch.no_grad()
    def enhance_pipelined(self, mode: str, srcs: Sequence[torch.Tensor], enrolls: Optional[Sequence[torch.Tensor]] = None,
                          segments_per_batch: int = 16, lm_graph: bool = False):
        """The same results as `enhance` ('se' / 'tse' / 'rtse'), produced by a THREE-STAGE PIPELINE over micro-batches of
        `segments_per_batch` 5 s segments on three streams: WavLM features of batch k + 1, LLM_SFT.generate of batch k and
        BiCodec.detokenize of batch k - 1 run concurrently.  The decode loop of the LM is bound by the latency of its dependent
        launches and leaves the matrix cores idle; the two GEMM-bound stages fill them.  Every stage owns its
        handle (workspace), so the three streams never share library state; tensors that cross streams are recorded on the consuming
        stream.  `lm_graph`: the LM replays one captured hipGraph per token (QA_LM_GRAPH) instead of issuing its ~17 000 launches.
        Segments are independent and every stage is batch-invariant, so the output is bit-identical to `enhance`
        (tests/test_unise_driver_gpu.py).
        MEASURED (profiles/r03_unise_pipeline_ab.txt, 6 x 16 segments): 176.8 ms per batch against 181.2 ms for `enhance` batch by
        batch - the overlap is almost nil: the workgroups of the GEMM stages (30 - 300 us each) hold the wave slots of every CU, so
        the 5 us launches of the LM queue behind them exactly as the LSTM step launches do, and the work adds
        up instead of overlapping; with replayed LM graphs 194.8 ms.  Throughput comes from the batch size instead: 64 segments per
        call run at 775 audio-s/s end to end against 463 at 16."""
        from . import _lib

        if self.detokenize is None:
            raise RuntimeError("UniSE.enhance_pipelined needs a tokenizer (unified_audio_amd.BiCodecTokenizer) or a detokenize callable")
        if mode not in ("se", "tse", "rtse"):
            raise KeyError(mode)
        segs, counts, samples = self._segments(mode, srcs)
        seg_src = torch.cat(segs, dim=0)
        dev = seg_src.device
        n_seg, m = seg_src.size(0), max(1, int(segments_per_batch))
        owner = torch.repeat_interleave(torch.arange(len(srcs)), torch.tensor(counts)).tolist()  # utterance of every segment
        cur = torch.cuda.current_stream(dev)
        s_feat, s_lm, s_dec = (torch.cuda.Stream(dev) for _ in range(3))
        for st in (s_feat, s_lm, s_dec):
            st.wait_stream(cur)
        ef, n_enr, frames = None, 0, None
        if mode != "se":
            if enrolls is None or len(enrolls) != len(srcs):
                raise ValueError(f"{mode} needs one enrollment per utterance")
            if len({e.size(-1) for e in enrolls}) != 1 and not self._ragged_ok:
                raise ValueError("enrollments of one call must have the same length (the LM's generate takes no enroll_lengths)")
            with torch.cuda.stream(s_feat):
                ef, n_enr, frames = self._enroll_features(enrolls)  # different lengths: padded features + per-utterance frame counts
        nb = (n_seg + m - 1) // m
        feats, toks, wavs = [None] * nb, [None] * nb, [None] * nb  # alive until the final join: nothing is freed under a stream
        ev_f = [torch.cuda.Event() for _ in range(nb)]
        ev_l = [torch.cuda.Event() for _ in range(nb)]
        old_graph = _lib.set_knob("QA_LM_GRAPH", 1) if lm_graph else None
        # the detokenizer's range check of its inputs is a host synchronisation per call: the tokens here are the LM's own (offsets
        # subtracted inside the active vocabulary slices, in range by construction), so the check is switched off inside the pipeline
        bic = getattr(getattr(self.detokenize, "__self__", None), "model", None)
        old_check = getattr(bic, "check_tokens", None)
        if old_check:
            bic.check_tokens = False
        try:
            for k in range(nb + 2):
                if k < nb:  # stage 1: features of micro-batch k
                    with torch.cuda.stream(s_feat):
                        x = seg_src[k * m:(k + 1) * m]
                        sm = samples[k * m:(k + 1) * m] if samples is not None else None
                        rag, steps = {}, mel_frames(SEG_LEN)
                        if sm is not None and any(n != SEG_LEN for n in sm):  # as _generate: the rows' own lengths through every stage
                            x, f, mel, rag = self._trimmed_inputs(x, sm)
                            steps = mel.size(1)
                        else:
                            f = self.semantic_model(x)
                        e = None
                        if ef is not None:
                            own = owner[k * m:(k + 1) * m]
                            e = ef[torch.tensor(own, device=dev)]
                            if frames is not None:  # as _generate: trimmed to the micro-batch's longest, ragged only if the lengths differ
                                fr = [frames[u] for u in own]
                                e = e[:, :max(fr)]
                                if len(set(fr)) > 1:
                                    rag["enroll_lengths"] = fr
                            e = e.contiguous()
                            e.record_stream(s_lm)
                        f.record_stream(s_lm)
                        feats[k] = (f, e, x.size(0), rag, steps)
                        ev_f[k].record(s_feat)
                j = k - 2
                if 0 <= j < nb:  # stage 3: waveform of micro-batch k - 2 (enqueued BEFORE the long LM enqueue of this turn)
                    with torch.cuda.stream(s_dec):
                        s_dec.wait_event(ev_l[j])
                        g, s = toks[j]
                        if samples is not None:
                            w = self._detokenize_rows(g, s, samples[j * m:(j + 1) * m])
                            for row in w:
                                row.record_stream(cur)
                        else:
                            w = self.detokenize(g.unsqueeze(1), s).squeeze(1)
                            w.record_stream(cur)
                        wavs[j] = w
                j = k - 1
                if 0 <= j < nb:  # stage 2: tokens of micro-batch k - 1
                    with torch.cuda.stream(s_lm):
                        s_lm.wait_event(ev_f[j])
                        f, e, b, rag, steps = feats[j]
                        g, s = self.dnn.generate(task_name=mode, enroll_mel=None if e is None else _Frames(b, mel_frames(n_enr)), enroll_feats=e,
                                                 mix_mel=_Frames(b, steps), mix_feats=f, do_sample=False, **rag)
                        g.record_stream(s_dec)
                        s.record_stream(s_dec)
                        toks[j] = (g, s)
                        ev_l[j].record(s_lm)
        finally:
            if old_graph is not None:
                _lib.set_knob("QA_LM_GRAPH", old_graph)
            if old_check:
                bic.check_tokens = old_check
        cur.wait_stream(s_dec)
        cur.wait_stream(s_lm)
        cur.wait_stream(s_feat)
        if samples is not None:
            return self._join_rows(srcs, counts, [row for w in wavs for row in w])
        est = torch.cat(wavs, dim=0)
        out, at = [], 0
        for src, c in zip(srcs, counts):
            out.append(est[at:at + c].reshape(-1)[: src.size(-1)])
            at += c
        return out

    def _separate(self, srcs: Sequence[torch.Tensor]):
        # pass 1 (model.py:224-242): SE on the first 5 s of every mixture (wrap-padded if shorter; no peak normalisation in this mode)
        heads = []
        for s in srcs:
            if s.dim() != 2 or s.size(0) != 1:
                raise ValueError(f"src must be [1, T] like the reference's batch, got {tuple(s.shape)}")
            heads.append(s[:, :SEG_LEN] if s.size(-1) > SEG_LEN else wrap_pad(s))
        head = torch.cat(heads, dim=0)
        g0, s0 = self._generate("se", head, [1] * len(srcs), None, 0)
        enroll = self.detokenize(g0.unsqueeze(1), s0).squeeze(1)[:, :SEG_LEN]                      # (U, t)
        enroll = enroll / (enroll.abs().amax(dim=-1, keepdim=True) + 1e-5) * 0.99                  # model.py:243 (per mixture)
        ef = self.semantic_model(enroll)
        # passes 2 and 3 (model.py:249-288): TSE then rTSE over all (un-normalised) segments with the tiled enrollment
        segs = [segment(s, normalise=False) for s in srcs]
        counts = [s.size(0) for s in segs]
        seg_src = torch.cat(segs, dim=0)
        out = []
        tse = self._split(counts, *self._generate("tse", seg_src, counts, ef, SEG_LEN))
        rtse = self._split(counts, *self._generate("rtse", seg_src, counts, ef, SEG_LEN))
        w1, w2 = self._waves(srcs, tse), self._waves(srcs, rtse)
        return list(zip(w1, w2))


class TestDataset:
    """The reference's inference data iterator (QuarkAudio-UniSE/dataloader/data_module.py:296-410, built from
    `config['dataset_config']['test_kwargs']`): every `*.flac` / `*.wav` of `data_src_dir` gives one batch tuple
    `(mode, enroll, src, tgt, fs, lengths, names)` with `batch_size == 1` (:340), first channel only, 16 kHz; the enrollment is wrapped /
    cut to `enroll_duration` seconds and scaled to a peak of 0.99 (:346-352).  Differences, both stated in INTEGRATION.md: wav files only
    (soundfile / FLAC are not available offline - a FLAC file raises), and a file at another rate is resampled on the device with
    qa_resample (torchaudio's sinc kernel) where the reference uses librosa's soxr_hq.  Sharding over ranks follows :364 (rank-strided)."""

    __test__ = False  # not a pytest class

    def __init__(self, data_enroll_dir, data_src_dir, data_tgt_dir, mode: str, enroll_duration: float = 5.0, batch_size: int = 1,
                 num_workers: int = 1, prefetch: int = 0, *, device="cuda:0", rank: int = 0, world_size: int = 1):
        import pathlib

        if batch_size != 1:
            raise AssertionError("batch_size == 1 (data_module.py:340); UniSE.enhance batches utterances itself")
        self.mode, self.enroll_duration = mode, float(enroll_duration)
        self.data_enroll_dir = pathlib.Path(data_enroll_dir) if data_enroll_dir is not None else None
        self.data_src_dir, self.data_tgt_dir = pathlib.Path(data_src_dir), pathlib.Path(data_tgt_dir)
        self.wav_names = [p.name for p in self.data_src_dir.glob("*.flac")] + [p.name for p in self.data_src_dir.glob("*.wav")]
        self.device, self.rank, self.world_size = torch.device(device), rank, world_size

    def load_wav(self, path):
        from . import audio_io

        if str(path).lower().endswith(".flac"):
            raise ValueError(f"{path}: FLAC needs soundfile, which is not available here - convert to wav")
        return audio_io.load_audio(str(path), 16000, self.device)

    def process_one_sample(self, name):
        import pathlib

        src = self.load_wav(self.data_src_dir / name)
        tgt = self.load_wav(self.data_tgt_dir / name)
        enroll = None
        if self.data_enroll_dir is not None:
            enroll = self.load_wav(self.data_enroll_dir / name)
            length = int(self.enroll_duration * 16000)
            enroll = wrap_pad(enroll, length)[..., :length] if enroll.shape[-1] < length else enroll[..., :length]
            enroll = enroll / (enroll.abs().max() + 1e-5) * 0.99
        return enroll, src, tgt, 16000, src.shape[-1], pathlib.Path(name).stem

    def __len__(self):
        return len(range(self.rank, len(self.wav_names), self.world_size))

    def __iter__(self):
        for i in range(self.rank, len(self.wav_names), self.world_size):
            enroll, src, tgt, fs, length, name = self.process_one_sample(self.wav_names[i])
            yield (self.mode, enroll, src, tgt, torch.tensor([fs], dtype=torch.int64), torch.tensor([length], dtype=torch.int64), [name])


class Model:
    """The test path of the reference's `Model` (QuarkAudio-UniSE/model/model.py:20-36 constructor, :82-91 state-dict rules, :170-290
    `test_step`), as `test.py:11-30` drives it: `Model(config)`, the Lightning checkpoint `config['ckpt_path']`, then one
    `test_step(batch, batch_idx)` per file with `batch = (mode, enroll, src, tgt, fs, lengths, names)`, writing
    `config['save_enhanced']/{name}.wav` ('se', 'tse') or `{name}_s1.wav` / `{name}_s2.wav` ('ss').

    config keys read, as in the reference: `codec_ckpt_dir` (-> BiCodecTokenizer(model_dir=...): `BiCodec/config.yaml` +
    `BiCodec/model.safetensors`), `llm_config` (-> LLM_SFT(**...)), `stft_config`, `save_enhanced`, `ckpt_path`.  One key is added:
    `semantic_model_path` - a local snapshot of microsoft/wavlm-base-plus (the reference downloads it, model.py:30; there is no
    network here); `semantic_model=` passes a loaded SSLFeatureExtractor instead.
    `test_steps(batches)` is the batched form: any number of the same tuples in one pass (segments of all files share the launches).
    """

    def __init__(self, config, *, device: str | torch.device = "cuda:0", semantic_model=None, tokenizer=None, dnn=None, max_segments: int = 64,
                 tail: str = "wrap"):
        from .bicodec import BiCodecTokenizer
        from .llm import LLM_SFT
        from .ssl import SPEC_WAVLM_BASE_PLUS, SSLFeatureExtractor

        self.config = config
        self.stft_conf = dict(config.get("stft_config") or dict(hop_length=HOP_LENGTH, win_length=WIN_LENGTH, n_fft=640, n_mels=80))
        if (self.stft_conf["hop_length"], self.stft_conf["win_length"]) != (HOP_LENGTH, WIN_LENGTH):
            raise ValueError(f"stft_config {self.stft_conf}: the LM's step count follows hop 320 / win 640 (conf/config.yaml:124-128)")
        self.device = torch.device(device)
        self.tokenizer = tokenizer if tokenizer is not None else BiCodecTokenizer(model_dir=config["codec_ckpt_dir"], device=self.device)
        self.dnn = dnn if dnn is not None else LLM_SFT(**config["llm_config"], device=self.device)
        if semantic_model is None:
            path = config.get("semantic_model_path")
            if path is None:
                raise ValueError("Model needs config['semantic_model_path'] (a local microsoft/wavlm-base-plus snapshot) or semantic_model=: "
                                 "the reference downloads the model (model.py:30), this machine has no network")
            import os

            # the snapshot's config.json carries the architecture, as it does for AutoModel.from_pretrained (for the published
            # snapshot it reads back as SPEC_WAVLM_BASE_PLUS); a snapshot without one is taken to be the published model
            has_config = os.path.isdir(str(path)) and os.path.isfile(os.path.join(str(path), "config.json"))
            semantic_model = SSLFeatureExtractor.from_pretrained(path, None if has_config else SPEC_WAVLM_BASE_PLUS, device=self.device)
        self.semantic_model = semantic_model
        # tail="trim" (not the reference's behaviour, see UniSE): the last segment of every file at its own length
        self.driver = UniSE(self.dnn, self.semantic_model, tokenizer=self.tokenizer, max_segments=max_segments, tail=tail)
        if config.get("ckpt_path") and dnn is None:
            import os

            if os.path.isfile(str(config["ckpt_path"])):  # test.py:30 hands it to trainer.test(..., ckpt_path=)
                self.load_checkpoint(config["ckpt_path"])

    def load_state_dict(self, state_dict, strict: bool = True):
        """model.py:82-91: the checkpoint holds `dnn.*` only (tokenizer / semantic_model are excluded on save and loading is non-strict)."""
        sd = {k: v for k, v in state_dict.items() if k.startswith("dnn.")}
        if not sd:
            raise KeyError("no 'dnn.*' entries: not a UniSE checkpoint (model.py:82-91)")
        self.dnn.load_state_dict(sd)
        return self

    def load_checkpoint(self, ckpt_path):
        """A Lightning checkpoint `{'state_dict': {'dnn.*': ...}, ...}` (what `trainer.test(model, dm, ckpt_path=...)` restores, test.py:30)."""
        ck = torch.load(ckpt_path, map_location="cpu", weights_only=False)
        return self.load_state_dict(ck["state_dict"] if isinstance(ck, dict) and "state_dict" in ck else ck)

    def eval(self):
        return self

    def to(self, *args, **kwargs):
        return self

    def extract_semantic_features(self, wavs: torch.Tensor) -> torch.Tensor:  # model.py:38-51
        return self.semantic_model(wavs.to(self.device))

    def stft_logmel(self, x: torch.Tensor, lengths=None) -> torch.Tensor:  # model.py:53-79; lengths: see stft_logmel
        c = self.stft_conf
        return stft_logmel(x, c["hop_length"], c["win_length"], c["n_fft"], c["n_mels"], lengths=lengths)

    def _save(self, name: str, est: torch.Tensor, fs: int):
        import os

        from . import audio_io

        out = self.config.get("save_enhanced") if hasattr(self.config, "get") else None
        if out is not None:  # model.py:195-196 (the directory is made by test.py:17)
            audio_io.write_wav(os.path.join(str(out), f"{name}.wav"), est, int(fs))

    @staticmethod
    def _unpack(batch):
        mode, enroll, src, tgt, fs, lengths, names = batch
        if src.dim() != 2 or src.size(0) != 1:
            raise ValueError(f"src must be [1, T]: the reference's test batches hold one file (data_module.py:340), got {tuple(src.shape)}")
        return mode, enroll, src, int(fs[0]), names[0]

    @torch.no_grad()
    def validation_step(self, batch, batch_idx: int = 0, *, use_lengths: bool = False):
        """model.py:134-160: score the checkpoint on one held-out batch `(mode, enroll, mix, speech, interf, fs, lengths, names)` (B >= 1).
        The LM's targets are the BiCodec tokens of the interferer for 'rtse' and of the clean speech otherwise (tokenize needs the
        tokenizer's encoder weights); the prompt is the SSL features of the mixture (and of the enrollment when there is one).  There is
        no Lightning here, so the values are returned instead of logged: {'valid_loss', 'valid_acc'}, 0-dim float32 device tensors.

        use_lengths (keyword only; False: the reference's behaviour, which ignores `lengths` and scores the padding of a short clip like
        any other frame): every clip is tokenized, featurised and scored over its own `lengths[b]` samples - tokenize(..., lengths=) with
        token_frames(lengths) semantic tokens, semantic_model(mix, lengths=) with frames(lengths[b]) feature frames, the enrollment at
        its one fixed duration as the loader gives it, then the LM's forward with per-row lengths.  The values pool
        the clips' own target rows."""
        mode, enroll, mix, speech, interf, fs, lengths, names = batch
        if use_lengths:
            return self._validation_step_lengths(mode, enroll, mix, speech, interf, lengths)
        global_tokens, semantic_tokens = self.tokenizer.tokenize(interf if mode == "rtse" else speech)  # (B, 1, G) int32, (B, T) int64
        mix = mix.to(self.device, torch.float32)
        # the LM reads only mix_mel.size(0) and whether enroll_mel is None (llm_sft.py:63,72): the frame-count stand-in replaces the mel
        mix_mel = _Frames(mix.size(0), mel_frames(mix.size(-1)))
        mix_feats = self.extract_semantic_features(mix)
        enroll_mel = enroll_feats = None
        if enroll is not None:
            enroll = enroll.to(self.device, torch.float32)
            enroll_mel = _Frames(enroll.size(0), mel_frames(enroll.size(-1)))
            enroll_feats = self.extract_semantic_features(enroll)
        loss, acc = self.dnn(task_name=mode, enroll_mel=enroll_mel, enroll_feats=enroll_feats, mix_mel=mix_mel, mix_feats=mix_feats,
                             global_ids=global_tokens.squeeze(1), semantic_ids=semantic_tokens)
        return {"valid_loss": loss, "valid_acc": acc}

    def _validation_step_lengths(self, mode, enroll, mix, speech, interf, lengths):
        """validation_step(use_lengths=True): the batch's `lengths` (samples) through the tokenizer, the semantic model and the LM."""
        import inspect

        def takes_lengths(fn):
            try:
                return "lengths" in inspect.signature(fn).parameters
            except (TypeError, ValueError):
                return False

        if lengths is None:
            raise ValueError("validation_step(use_lengths=True): the batch carries no `lengths`")
        if not takes_lengths(self.tokenizer.tokenize) or not hasattr(self.tokenizer, "token_frames"):
            raise TypeError("validation_step(use_lengths=True): the tokenizer needs tokenize(wav, lengths=) and token_frames(lengths)")
        if not takes_lengths(self.semantic_model.__call__) or not hasattr(self.semantic_model, "frames"):
            raise TypeError("validation_step(use_lengths=True): the semantic model needs __call__(wavs, lengths=) and frames(n_samples)")
        lens = [int(v) for v in (lengths.tolist() if torch.is_tensor(lengths) else lengths)]
        global_tokens, semantic_tokens = self.tokenizer.tokenize(interf if mode == "rtse" else speech, lengths=lens)
        semantic_lengths = self.tokenizer.token_frames(lens)
        mix = mix.to(self.device, torch.float32)
        mix_mel = _Frames(mix.size(0), mel_frames(mix.size(-1)))
        mix_feats = self.semantic_model(mix, lengths=lens)
        mix_lengths = [self.semantic_model.frames(n) for n in lens]
        enroll_mel = enroll_feats = None
        if enroll is not None:  # one fixed duration for the whole batch (data_module.py: enroll_duration)
            enroll = enroll.to(self.device, torch.float32)
            enroll_mel = _Frames(enroll.size(0), mel_frames(enroll.size(-1)))
            enroll_feats = self.extract_semantic_features(enroll)
        loss, acc = self.dnn(task_name=mode, enroll_mel=enroll_mel, enroll_feats=enroll_feats, mix_mel=mix_mel, mix_feats=mix_feats,
                             global_ids=global_tokens.squeeze(1), semantic_ids=semantic_tokens, mix_lengths=mix_lengths,
                             semantic_lengths=semantic_lengths)
        return {"valid_loss": loss, "valid_acc": acc}

    @torch.no_grad()
    def test_step(self, batch, batch_idx: int = 0):
        """model.py:170-290.  Returns what it wrote: the estimate [T] ('se' / 'tse'), the pair ('ss'), None for any other mode (the
        reference's if / elif chain falls through silently)."""
        res = self.test_steps([batch])
        return res[0] if res else None

    @torch.no_grad()
    def test_steps(self, batches):
        """Any number of test batches in ONE pass per mode: all 5 s segments of all files go through WavLM, the LM and BiCodec together
        (every stage is batch-invariant, so each file's result equals its own test_step bit for bit)."""
        items = [self._unpack(b) for b in batches]
        out = [None] * len(items)
        for mode in ("se", "tse", "ss"):
            idx = [i for i, it in enumerate(items) if it[0] == mode]
            if not idx:
                continue
            srcs = [items[i][2].to(self.device, torch.float32) for i in idx]
            enrolls = None
            if mode == "tse":
                if any(items[i][1] is None for i in idx):
                    raise ValueError("'tse' needs an enrollment in every batch (data_enroll_dir)")
                enrolls = [items[i][1].to(self.device, torch.float32) for i in idx]
            for i, est in zip(idx, self.driver.enhance(mode, srcs, enrolls)):
                _, _, _, fs, name = items[i]
                if mode == "ss":
                    self._save(f"{name}_s1", est[0], fs)
                    self._save(f"{name}_s2", est[1], fs)
                else:
                    self._save(name, est, fs)
                out[i] = est
        return out
