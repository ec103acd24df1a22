"""The chunked causal H-Codec 1.0 encoder on the GPU (Codec.streaming / encode_stream -> qa_hcodec_stream_*): the
concatenated steps against the oracle's and the library's own offline causal encode, bit-for-bit properties of the state, the refusals,
and stream_window_kernel alone against a torch restatement."""
import ctypes as C

import pytest
import torch

from oracle import hcodec_ref as R
from oracle import synth
from tests import hcodec_stream_ref as S
from tests.util import MINI, audit_codes_bnq, check_guarded_out, guarded_out, rel_err

pytestmark = pytest.mark.gpu

STAGE_TOL = 5e-5  # relative RMS: the bound the offline graph's stages are held to against the same oracle (tests/test_hcodec_gpu.py)
CAUSAL_MINI = dict(MINI, causal=True)


def _codec(spec_kwargs, sd, device):
    import unified_audio_amd as qa

    codec = qa.Codec(None, None, None, spec=qa.HCodecSpec(**spec_kwargs), device=device).load_state_dict(sd)
    codec.enable_taps()
    return codec


def _offline_emb(codec, ospec, wav, device):
    """The library's own offline causal encode: tap enc.emb as [B, N, D] and the acoustic codes."""
    B, N = wav.shape[0], wav.shape[-1] // ospec.enc_hop
    feat = synth.synth_feat(5, B, 2 * N, ospec.sem_in)
    ac, _ = codec.encode(wav.to(device), feat.to(device))
    return codec.tap("enc.emb").view(B, N, ospec.code_dim).clone(), ac.clone()


def _stream(codec, ospec, wav, chunks, device):
    """wav [B, 1, T] through the codec's CURRENT stream, chunk by chunk (code frames): (codes [B, nq, N], emb [B, N, D])."""
    hop, t, acs, embs = ospec.enc_hop, 0, [], []
    for n in chunks:
        ac, emb = codec.encode_stream(wav[..., t * hop:(t + n) * hop].to(device), return_emb=True)
        acs.append(ac)
        embs.append(emb)
        t += n
    return torch.cat(acs, 2), torch.cat(embs, 1)


@pytest.fixture(scope="module")
def mini(gpu_device):
    """One causal MINI codec, the shared case's waveform and its references, computed once and left unchanged."""
    ospec, sd, wav = S.case_inputs(S.GPU_MINI_CASE, CAUSAL_MINI)
    codec = _codec(CAUSAL_MINI, sd, gpu_device)
    emb_o, ac_o = S.oracle_emb_and_codes(sd, wav, ospec)
    emb_lib, ac_lib = _offline_emb(codec, ospec, wav, gpu_device)
    return dict(ospec=ospec, sd=sd, wav=wav, codec=codec, emb_o=emb_o, ac_o=ac_o, emb_lib=emb_lib, ac_lib=ac_lib,
                cb=R.rvq_codebooks(sd, "quantizer", ospec.num_quantizers))


@pytest.mark.parametrize("name", list(S.CHUNKINGS))
def test_stream_equals_the_offline_causal_encode(qa_lib, gpu_device, mini, name):
    codec, ospec, wav = mini["codec"], mini["ospec"], mini["wav"]
    with codec.streaming(wav.shape[0], max_frames=S.FRAMES):
        assert codec.is_streaming and codec.streaming_offset == 0
        ac, emb = _stream(codec, ospec, wav, S.CHUNKINGS[name], gpu_device)
        assert codec.streaming_offset == S.FRAMES
    assert not codec.is_streaming and codec.streaming_offset == -1
    e_or, e_lib = rel_err(emb, mini["emb_o"].transpose(1, 2)), rel_err(emb, mini["emb_lib"])
    print(f"{name}: emb against the oracle {e_or:.2e}, against the library's offline encode {e_lib:.2e} "
          f"(offline against the oracle {rel_err(mini['emb_lib'], mini['emb_o'].transpose(1, 2)):.2e})")
    assert ac.shape == mini["ac_o"].shape and ac.dtype == torch.int64
    assert e_or < STAGE_TOL and e_lib < STAGE_TOL
    audit_codes_bnq(mini["emb_o"], mini["cb"], ac, mini["ac_o"])
    # no decision of the oracle is a near-tie for these seeds (tests/test_hcodec_stream_cpu.py), so the codes are EQUAL
    assert torch.equal(ac.cpu(), mini["ac_o"])


def test_outputs_do_not_depend_on_which_are_asked_for(qa_lib, gpu_device, mini):
    codec, ospec, wav = mini["codec"], mini["ospec"], mini["wav"]
    B, hop, chunks = wav.shape[0], ospec.enc_hop, S.CHUNKINGS["2-1-5-16"]
    stream = torch.cuda.current_stream(gpu_device).cuda_stream
    with codec.streaming(B, max_frames=S.FRAMES):
        ac_both, emb_both = _stream(codec, ospec, wav, chunks, gpu_device)
    with codec.streaming(B, max_frames=S.FRAMES):
        t, acs = 0, []
        for n in chunks:
            acs.append(codec.encode_stream(wav[..., t * hop:(t + n) * hop].to(gpu_device)))  # codes alone
            t += n
    with codec.streaming(B, max_frames=S.FRAMES):
        t, embs = 0, []
        for n in chunks:  # emb alone: the C-ABI (the Python method always returns the codes)
            x = wav[:, 0, t * hop:(t + n) * hop].to(gpu_device).contiguous()
            emb = torch.empty(B, n, ospec.code_dim, device=gpu_device)
            assert qa_lib.qa_hcodec_stream_encode(codec._handle, x.data_ptr(), n * hop, None, emb.data_ptr(), stream) == 0, qa_lib.qa_last_error()
            embs.append(emb)
            t += n
        x = wav[:, 0, :hop].to(gpu_device).contiguous()
        assert qa_lib.qa_hcodec_stream_encode(codec._handle, x.data_ptr(), hop, None, None, stream) != 0  # neither output
    assert torch.equal(torch.cat(acs, 2), ac_both) and torch.equal(torch.cat(embs, 1), emb_both)


def test_state_properties_bit_for_bit(qa_lib, gpu_device, mini):
    codec, ospec, wav = mini["codec"], mini["ospec"], mini["wav"]
    B, hop, chunks = wav.shape[0], ospec.enc_hop, (3, 4, 3, 4, 3, 4, 3)
    twin = wav.clone()
    twin[1] = twin[0]  # two equal rows of a batch
    with codec.streaming(B, max_frames=S.FRAMES):
        ac0, emb0 = _stream(codec, ospec, twin, chunks, gpu_device)
        # reset, then the same chunks: the first run again (reflect fill, zeroed LSTM state, stale K / V rows invisible)
        codec.reset_streaming()
        assert codec.streaming_offset == 0
        ac1, emb1 = _stream(codec, ospec, twin, chunks, gpu_device)
        # an offline encode + decode on the same handle between two steps leaves the following steps unchanged
        codec.reset_streaming()
        head = _stream(codec, ospec, twin[..., :7 * hop], (3, 4), gpu_device)
        feat = synth.synth_feat(6, B, 2 * S.FRAMES, ospec.sem_in).to(gpu_device)
        ac_off, sc_off = codec.encode(wav.to(gpu_device), feat)
        codec.decode(ac_off, sc_off)
        assert codec.streaming_offset == 7
        tail = _stream(codec, ospec, twin[..., 7 * hop:], (3, 4, 3, 4, 3), gpu_device)
    with codec.streaming(B, max_frames=S.FRAMES):  # a fresh stream behind end
        ac3, emb3 = _stream(codec, ospec, twin, chunks, gpu_device)
    assert torch.equal(emb0[0], emb0[1]) and torch.equal(ac0[0], ac0[1]) and not torch.equal(emb0[0], emb0[2])
    assert torch.equal(emb1, emb0) and torch.equal(ac1, ac0)
    assert torch.equal(torch.cat((head[1], tail[1]), 1), emb0) and torch.equal(torch.cat((head[0], tail[0]), 2), ac0)
    assert torch.equal(emb3, emb0) and torch.equal(ac3, ac0)
    assert torch.equal(ac_off, mini["ac_lib"])  # and the offline call between the steps was not disturbed either


def test_long_run_of_single_frame_steps(qa_lib, gpu_device):
    """2 + 300 single-frame steps at B = 1 against ONE offline encode of the 302 frames: nothing drifts over a long history."""
    ospec, sd, wav = S.case_inputs(S.GPU_LONG_CASE, CAUSAL_MINI)
    codec = _codec(CAUSAL_MINI, sd, gpu_device)
    emb_lib, ac_lib = _offline_emb(codec, ospec, wav, gpu_device)
    N = S.GPU_LONG_CASE["frames"]
    with codec.streaming(1, max_frames=N):
        ac, emb = _stream(codec, ospec, wav, (2,) + (1,) * (N - 2), gpu_device)
        assert codec.streaming_offset == N
    e, e_tail = rel_err(emb, emb_lib), rel_err(emb[:, -50:], emb_lib[:, -50:])
    print(f"{N} frames in {N - 1} steps against the offline encode: {e:.2e} (last 50 frames {e_tail:.2e}); "
          f"{int((ac != ac_lib).sum())} of {ac.numel()} codes differ")
    assert e < STAGE_TOL and e_tail < STAGE_TOL


def test_refusals_leave_the_stream_as_it_was(qa_lib, gpu_device, mini):
    import unified_audio_amd as qa

    codec, ospec, wav = mini["codec"], mini["ospec"], mini["wav"].to(gpu_device)
    B, hop = wav.shape[0], ospec.enc_hop
    assert codec.stream_first_min_frames == 2
    with codec.streaming(B, max_frames=5):
        with pytest.raises(qa.QuarkAudioError, match="first chunk"):  # a first chunk of 1 frame
            codec.encode_stream(wav[..., :hop])
        with pytest.raises(qa.QuarkAudioError, match="multiple"):  # not a whole number of code frames
            codec.encode_stream(wav[..., :2 * hop + 1])
        with pytest.raises(qa.QuarkAudioError, match="batch"):
            codec.encode_stream(wav[:1, :, :2 * hop])
        assert codec.streaming_offset == 0
        ac_a, emb_a = codec.encode_stream(wav[..., :2 * hop], return_emb=True)
        with pytest.raises(qa.QuarkAudioError, match="capacity"):  # 2 + 4 > max_frames = 5
            codec.encode_stream(wav[..., 2 * hop:6 * hop])
        with pytest.raises(qa.QuarkAudioError, match="multiple"):
            codec.encode_stream(wav[..., 2 * hop:3 * hop - 3])
        assert codec.streaming_offset == 2
        ac_b, emb_b = codec.encode_stream(wav[..., 2 * hop:5 * hop], return_emb=True)
        assert codec.streaming_offset == 5
        with pytest.raises(qa.QuarkAudioError, match="capacity"):
            codec.encode_stream(wav[..., 5 * hop:6 * hop])
    emb, ac = torch.cat((emb_a, emb_b), 1), torch.cat((ac_a, ac_b), 2)
    assert rel_err(emb, mini["emb_lib"][:, :5]) < STAGE_TOL and torch.equal(ac.cpu(), mini["ac_o"][..., :5])
    # a non-causal handle has no stream, and says what to call instead
    nc = _codec(dict(MINI), mini["sd"], gpu_device)
    with pytest.raises(qa.QuarkAudioError, match="causal"):
        nc.streaming_forever(B)
    assert not nc.is_streaming and nc.streaming_offset == -1
    with pytest.raises(qa.QuarkAudioError, match="not streaming"):
        nc.encode_stream(wav[..., :2 * hop])
    with pytest.raises(qa.QuarkAudioError):  # max_frames beyond the Transformer's 8192 positions / below the first chunk
        codec.streaming_forever(B, max_frames=4097)
    with pytest.raises(qa.QuarkAudioError):
        codec.streaming_forever(B, max_frames=1)
    assert not codec.is_streaming
    # ... and the causal codec still streams exactly
    with codec.streaming(B, max_frames=S.FRAMES):
        ac, emb = _stream(codec, ospec, mini["wav"], (2, 1, 5, 16), gpu_device)
    assert rel_err(emb, mini["emb_lib"]) < STAGE_TOL and torch.equal(ac.cpu(), mini["ac_o"])


def _window_ref(state, chunk, ctx, first):
    head = chunk[:, 1:ctx + 1].flip(1) if first else state
    win = torch.cat((head, chunk), 1)
    return win, win[:, -ctx:]


@pytest.mark.parametrize("Cc", [1, 32, 132])
def test_stream_window_kernel_is_an_exact_copy(qa_lib, gpu_device, Cc):
    """qa_debug_stream_window against a torch restatement, by equality (pure copies), outputs between sentinels.  n < ctx is where the next
    state takes rows of the current one - the rows that a kernel updating the state in place gets wrong.  A first step needs n > ctx (the
    reflection reads frames 1 .. ctx): shorter ones are refused before the launch."""
    B = 3
    g = torch.Generator().manual_seed(100 + Cc)
    stream = torch.cuda.current_stream(gpu_device).cuda_stream
    for ctx in (2, 6, 8):
        for n in sorted({1, ctx - 1, ctx, ctx + 1, 40}):
            for first in (0, 1):
                for head in ((0, 1) if Cc == 132 and n == ctx - 1 else (0,)):  # head 1: unaligned buffers take the scalar path
                    state = torch.randn(B, ctx, Cc, generator=g).to(gpu_device)
                    chunk = torch.randn(B, n, Cc, generator=g).to(gpu_device)
                    wbuf, win = guarded_out(B * (ctx + n), Cc, Cc, head, gpu_device)
                    sbuf, sout = guarded_out(B * ctx, Cc, Cc, head, gpu_device)
                    st = qa_lib.qa_debug_stream_window(state.data_ptr(), chunk.data_ptr(), win.data_ptr(), sout.data_ptr(), B, ctx, n, Cc,
                                                       first, stream)
                    if first and n <= ctx:
                        assert st != 0 and torch.isnan(win).all() and torch.isnan(sout).all(), (ctx, n)
                        continue
                    assert st == 0, (ctx, n, first, qa_lib.qa_last_error())
                    check_guarded_out(wbuf, win, head)
                    check_guarded_out(sbuf, sout, head)
                    want_win, want_state = _window_ref(state, chunk, ctx, first)
                    assert torch.equal(win.view(B, ctx + n, Cc), want_win), (ctx, n, first, head)
                    assert torch.equal(sout.view(B, ctx, Cc), want_state), (ctx, n, first, head)
    # updating the state in place is refused, not raced
    state = torch.randn(B, 6, Cc).to(gpu_device)
    chunk = torch.randn(B, 2, Cc).to(gpu_device)
    win = torch.empty(B, 8, Cc, device=gpu_device)
    assert qa_lib.qa_debug_stream_window(state.data_ptr(), chunk.data_ptr(), win.data_ptr(), state.data_ptr(), B, 6, 2, Cc, 0, stream) != 0


def test_real_encoder_widths(qa_lib, gpu_device):
    """The H-Codec 1.0 encoder as shipped (ratios 2, 4, 5, 8, 32 -> 512 channels, two d = 512 layers, 1024 codes x 4; the decoder cut to one
    layer each to keep the upload short): B = 2, 8 code frames in chunks (2, 1, 1, 4)."""
    case = S.GPU_REAL_CASE
    kw = {f: getattr(R.SPEC_10, f) for f in R.SPEC_10.__dataclass_fields__}
    kw.update(dec_layers=1, convnext_layers=1, causal=True)
    ospec, sd, wav = S.case_inputs(case, kw)
    codec = _codec(kw, sd, gpu_device)
    emb_o, ac_o = S.oracle_emb_and_codes(sd, wav, ospec)
    with codec.streaming(case["B"], max_frames=case["frames"]):
        ac, emb = _stream(codec, ospec, wav, case["chunks"], gpu_device)
    e = rel_err(emb, emb_o.transpose(1, 2))
    print(f"real widths: emb against the oracle {e:.2e}; {int((ac.cpu() != ac_o).sum())} of {ac.numel()} codes differ")
    assert e < STAGE_TOL
    audit_codes_bnq(emb_o, R.rvq_codebooks(sd, "quantizer", ospec.num_quantizers), ac, ac_o)
