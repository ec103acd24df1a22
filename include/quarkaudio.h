/*
 * quarkaudio.h - C-ABI of libquarkaudio_hip.so: the MI355X (gfx950) hot path of alibaba/unified-audio
 * (QuarkAudio): H-Codec encode -> RVQ -> decode, and the UniSE decoder-only AR-LM generate loop.
 *
 * The reference is 100 % Python and has no FFI of its own; the drop-in boundary is the tensor-in /
 * tensor-out method pair a maintainer would rebind (see INTEGRATION.md for the ctypes stub):
 *
 *   qa_hcodec_encode   <-> Codec.encode(x, feat)            QuarkAudio-HCodec/HCodec-1.0/vq/codec.py:166-175
 *   qa_hcodec_decode   <-> Codec.decode(ac, sc)             QuarkAudio-HCodec/HCodec-1.0/vq/codec.py:178-187
 *   qa_hcodec_create   <-> Codec(...) + load_state_dict     QuarkAudio-HCodec/HCodec-1.0/audio_tokenizer.py:23-26
 *   qa_rvq_search      <-> ResidualVQ.forward (eval)        call sites vq/codec.py:171-172 (algorithm: vq/core_vq.py:223-231,394-404)
 *   qa_rvq_lookup      <-> ResidualVQ.get_output_from_indices  call sites vq/codec.py:183-184 (vq/core_vq.py:406-412)
 *   qa_lm_create       <-> LLM_SFT(...) + load_state_dict   QuarkAudio-UniSE/model/llm/llm_sft.py:13-33, model/model.py:82-91
 *   qa_lm_generate     <-> LLM_SFT.generate(...)            QuarkAudio-UniSE/model/llm/llm_sft.py:93-195
 *   qa_bicodec_detokenize <-> BiCodec.detokenize(...)       QuarkAudio-UniSE/model/bicodec/bicodec.py:182-199
 *   qa_bicodec_tokenize   <-> BiCodec.tokenize(batch)       QuarkAudio-UniSE/model/bicodec/bicodec.py:151-180
 *   qa_bicodec_forward    <-> BiCodec.forward(batch)        QuarkAudio-UniSE/model/bicodec/bicodec.py:113-149
 *
 * Conventions
 *   - every function returns 0 on success or a negative qa_status; nothing throws across the ABI;
 *     qa_last_error() returns a thread-local, NUL-terminated description of the last failure.
 *   - all data pointers are DEVICE pointers owned by the caller (e.g. torch tensor.data_ptr()),
 *     contiguous unless strides are passed, except the weight table of *_create which is HOST memory
 *     in the reference's own state_dict layout (the library folds weight-norm, re-lays filters out for
 *     its kernels and keeps its own device copy).
 *   - work is enqueued on `stream` (a hipStream_t; NULL = the default stream) and is asynchronous;
 *     a handle owns its workspaces and must not be used from two streams / threads at once.
 *     EXCEPTION (qa_hcodec_encode / _decode and their adaptive forms): a call that launched one of the in-launch
 *     LSTM recurrences (knobs QA_LSTM_XCD - the default for d = 512 / 768 -, QA_LSTM_TEAM, QA_LSTM_PERSISTENT) waits
 *     for `stream` on the host before it returns, because it must read that launch's own error word and, if a bounded
 *     barrier spin ran out (device shared with another persistent kernel), re-run itself on the per-step kernels: such
 *     a call is host-synchronous and cannot be issued under a caller's stream capture.  QA_LSTM_XCD=0 QA_LSTM_TEAM=0
 *     QA_LSTM_PERSISTENT=0 restores fully asynchronous calls (launch-per-step recurrence).  The error word and the
 *     launch count are per CALL (a ticket taken by the calling thread), so handles that share a device from
 *     different threads never collect each other's failure.
 *   - there is no CPU fallback: on a machine without a gfx950 device every compute entry point fails.
 */
#ifndef QUARKAUDIO_H_
#define QUARKAUDIO_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QA_VERSION 103 /* 0.1.2 */

typedef enum qa_status {
    QA_OK = 0,
    QA_ERR_INVALID = -1,   /* bad argument / shape (the reference raises AssertionError / RuntimeError) */
    QA_ERR_HIP = -2,       /* a HIP runtime call failed (no device, launch failure, out of memory) */
    QA_ERR_MISSING = -3,   /* a tensor the architecture needs is not in the weight table (KeyError) */
    QA_ERR_UNSUPPORTED = -4
} qa_status;

/* One named fp32 tensor of a state_dict.  `data` is HOST memory, row-major, `numel` elements. */
typedef struct qa_tensor {
    const char* name;
    const float* data;
    int64_t numel;
} qa_tensor;

/* Architecture constants of an H-Codec model (hard-coded in the reference: vq/codec.py:30-136). */
typedef struct qa_hcodec_spec {
    int32_t n_filters;        /* 32            codec.py:33  */
    int32_t n_ratios;         /* 4 */
    int32_t ratios[8];        /* encoder order 2,4,5,8  (codec.py:33 reversed by seanet.py:114) */
    int32_t dimension;        /* 512 */
    int32_t enc_heads;        /* 8   seanet.py:166 */
    int32_t enc_layers;       /* 2   seanet.py:167 */
    int32_t sem_in;           /* 768 codec.py:122 */
    int32_t sem_ch;           /* 768 codec.py:123 */
    int32_t n_sem_strides;    /* 2 */
    int32_t sem_strides[4];   /* 2,1 codec.py:126 */
    int32_t code_dim;         /* 512 */
    int32_t codebook_size;    /* 1024 */
    int32_t num_quantizers;   /* 4 */
    int32_t dec_dim;          /* 768 codec.py:44 */
    int32_t dec_inter;        /* 2304 */
    int32_t dec_heads;        /* 8 */
    int32_t dec_layers;       /* 2 */
    int32_t convnext_layers;  /* 12 */
    int32_t n_fft;            /* 1280 */
    int32_t hop;              /* 320 */
    int32_t gn_groups;        /* 32 */
    /* H-Codec 1.5 adaptive frame rate (QuarkAudio-HCodec/HCodec-1.5/conf/config_adaptive_v3.yaml:65-111); 0 = H-Codec 1.0 */
    int32_t adaptive;
    int32_t agg_layers;       /* 32  aggregators.*.num_layers (d_model = code_dim) */
    int32_t agg_heads;        /* 8 */
    int32_t agg_ff;           /* 2048 */
    int32_t bt_layers;        /* 32  transformer_kwargs.num_layers (bottleneck, d_model = 2*code_dim) */
    int32_t bt_heads;         /* 8 */
    int32_t bt_ff;            /* 2048 */
    int32_t max_tokens_per_group; /* 8 */
    float threshold;          /* 0.6 manual_threshold */
    /* H-Codec 2.0 (QuarkAudio-HCodec/HCodec-2.0/conf/large_12.5hz_config.yaml); version 0 / 10 = SEANet family (1.0, 1.5) */
    int32_t version;          /* 20 = STFT-domain ConvNeXt encoder, repeat-interleave decoder embed */
    int32_t enc_dim;          /* 1536 */
    int32_t enc_inter;        /* 4608 */
    int32_t enc_convnext_layers; /* 24 */
    int32_t frame_stride;     /* 4 = int(50 / target_frame_rate) */
    int32_t tr_inter_cap;     /* 4096: transformer MLP width = min(4*d, cap); 0 = 4*d */
    /* causal variant (all versions; 2.0: `causal` of encoder_config / decoder_config, codec_encoder.py:23, codec_decoder.py:25):
     * every SConv1d pads
     * (k_eff - stride, extra) instead of splitting it (encoder_modules/conv.py:203-206), vq/conv.py's Conv1d /
     * ConvTranspose1d pad (k - 1, 0) (vq/conv.py:44-47,76-79) and both Transformers apply the tril mask
     * (encoder_modules/transformer.py:470-475).  vq/codec.py:31 ships causal=False. */
    int32_t causal;
    /* H-Codec 1.5: `causal` / `context_frames` of the two aggregators and `causal` / `context` of the bottleneck transformer
     * (config_adaptive_v3.yaml:84,87,93,96,103,105; the YAML ships causal: false, where the context is ignored,
     * mimi/transformer.py:403-413).  causal = 1: key j visible to query i iff 0 <= i - j < context (context 0 = unbounded). */
    int32_t agg_causal, agg_context, bt_causal, bt_context;
} qa_hcodec_spec;

typedef struct qa_hcodec qa_hcodec;

int qa_version(void);
const char* qa_last_error(void);
/* number of visible HIP devices (0 if none / runtime unavailable); never fails */
int qa_device_count(void);

/* ---- H-Codec ------------------------------------------------------------------------------------ */

int qa_hcodec_create(qa_hcodec** out, const qa_hcodec_spec* spec, const qa_tensor* tensors, int64_t n_tensors,
                     int device);
void qa_hcodec_destroy(qa_hcodec* h);

/* Codec.encode.  wav: [B, T] fp32, T a multiple of the encoder hop (2*prod(ratios); HCodecTokenizer.pad_wav
 * guarantees it, audio_tokenizer.py:50-53).  feat: fp32 [B, sem_in, N50] addressed through element strides
 * (so the [B, N50, sem_in] tensor the SSL model returns can be passed without the transpose copy the reference
 * makes at audio_tokenizer.py:59).  Outputs: int64 [B, num_quantizers, N25] each, contiguous. */
int qa_hcodec_encode(qa_hcodec* h, const float* wav, int64_t B, int64_t T,
                     const float* feat, int64_t feat_stride_b, int64_t feat_stride_c, int64_t feat_stride_t,
                     int64_t n_feat_frames, int64_t* acoustic_codes, int64_t* semantic_codes, void* stream);

/* Codec.decode.  codes: int64 [B, num_quantizers, N]; wav_out: fp32 [B, 2*N*hop]. */
int qa_hcodec_decode(qa_hcodec* h, const int64_t* acoustic_codes, const int64_t* semantic_codes, int64_t B,
                     int64_t N, float* wav_out, void* stream);

/* Per-clip lengths in one call (non-causal H-Codec 1.0; non-causal H-Codec 2.0, section 33): clip b behaves as
 * qa_hcodec_encode / _decode would for it alone at its own length.  frames: HOST memory, int64 [B], the clips' lengths in CODE frames,
 * 1 .. N each (N = T / encoder hop; H-Codec 2.0: hop * frame_stride = 3840 samples), read during the call and checked before anything is
 * launched (QA_ERR_INVALID names the row).  H-Codec 1.5 (which has the _adaptive_ragged calls below) and causal handles, 1.0 or 2.0, are
 * refused with QA_ERR_UNSUPPORTED.  A call whose lengths all equal N is the rectangular call, through the same launches.
 *   encode: samples of wav from frames[b] * encoder hop on and feature frames from frames[b] * (n_feat_frames / N) on are padding that is
 *           never read (NaN there changes nothing); codes at frames >= frames[b] are written as -1, the dropped code, so the output is
 *           also a legal input of qa_hcodec_decode.
 *   decode: code entries at frames >= frames[b] are ignored, whatever they hold; wav_out[b] is exactly 0 from sample
 *           frames[b] * 2 * hop (H-Codec 2.0: frames[b] * frame_stride * hop) on. */
int qa_hcodec_encode_ragged(qa_hcodec* h, const float* wav, int64_t B, int64_t T, const int64_t* frames,
                            const float* feat, int64_t feat_stride_b, int64_t feat_stride_c, int64_t feat_stride_t,
                            int64_t n_feat_frames, int64_t* acoustic_codes, int64_t* semantic_codes, void* stream);
int qa_hcodec_decode_ragged(qa_hcodec* h, const int64_t* acoustic_codes, const int64_t* semantic_codes, int64_t B, int64_t N,
                            const int64_t* frames, float* wav_out, void* stream);

/* The causal H-Codec 1.0 acoustic encoder as a stream: SEANetEncoder -> Transformer -> strided out conv ->
 * ResidualVQ, chunk by chunk.  The embeddings and acoustic codes of a step equal what ONE qa_hcodec_encode of the concatenated waveform
 * gives for the same code frames (spec.causal = 1 makes every frame a function of the past alone); the reference has no such call.
 *   qa_hcodec_stream_begin   allocates the state for B rows and up to max_frames CODE frames (first-chunk minimum .. 4096: the
 *                            Transformer holds 8192 positions at 2 per code frame): per stateful convolution its last ctx = k_eff -
 *                            stride input rows, per Transformer layer the LSTM's (h, c) and the roped K / V rows.  The state is an allocation
 *                            of its own, so offline encode / decode / forward calls on the same handle between two steps change nothing.
 *                            On a handle that already streams it frees the old stream and starts a new one.
 *   qa_hcodec_stream_encode  the next n_samples samples of every row, wav [B, n_samples] (device), n_samples a positive multiple of the
 *                            samples of a code frame (640; a trailing partial frame is the caller's to zero-pad, as pad_wav does), n =
 *                            n_samples / 640 code frames -> acoustic_codes int64 [B, nq, n] and / or emb fp32 [B, n, code_dim] (either
 *                            may be NULL, not both; the outputs do not depend on which are asked for).  The FIRST chunk of a stream pads
 *                            its left edge with the reflection of its own frames, which equals the offline padding only from
 *                            first_min_frames code frames on (2 for the shipped geometry): a shorter first chunk is refused.
 *   qa_hcodec_stream_reset   back to offset 0: the next step is a first step again.
 *   qa_hcodec_stream_end     frees the state; harmless on a handle that does not stream.
 *   qa_hcodec_stream_offset  code frames streamed since begin / reset, -1 when not streaming.
 *   qa_hcodec_stream_geometry  host logic, no device: the samples of a code frame, the first-chunk minimum and the contexts of the stateful
 *                            convolutions in graph order (conv0, per stage the residual k3 and the down conv, the out conv) written to
 *                            ctx[0 .. *n_ctx) (ctx may be NULL; cap: its capacity).
 * Refused, before anything is launched and with the state and the offset left as they were: a non-causal handle, H-Codec 1.5 / 2.0
 * (QA_ERR_UNSUPPORTED), a step without begin, n_samples that is not a positive multiple of the hop, a first chunk below the minimum, a
 * step beyond max_frames, a stream under capture (the offset is host state). */
int qa_hcodec_stream_begin(qa_hcodec* h, int64_t B, int64_t max_frames);
int qa_hcodec_stream_encode(qa_hcodec* h, const float* wav, int64_t n_samples, int64_t* acoustic_codes, float* emb, void* stream);
int qa_hcodec_stream_reset(qa_hcodec* h);
int qa_hcodec_stream_end(qa_hcodec* h);
int64_t qa_hcodec_stream_offset(const qa_hcodec* h);
int qa_hcodec_stream_geometry(const qa_hcodec_spec* spec, int64_t* samples_per_frame, int64_t* first_min_frames, int32_t* ctx, int32_t cap,
                              int32_t* n_ctx);
/* Per-row lengths, offsets and resets in one step: the rows of a stream need not start, step or end together.
 * Between two of its resets (or begin and its first reset) the concatenated outputs of a row over the steps in which it had frames equal
 * what one offline causal qa_hcodec_encode of that row's own concatenated waveform gives, whatever the other rows did meanwhile.
 *   qa_hcodec_stream_encode_rows  as qa_hcodec_stream_encode, row b consuming only its first frames[b] code frames of the rectangle wav
 *                            [B, n_samples]; frames is HOST memory, int64 [B], 0 <= frames[b] <= n = n_samples / 640, 0: the row idles -
 *                            its state and offset stay as they are, bit for bit.  Samples behind a row's frames are never read (they may be
 *                            non-finite).  Outputs in the rectangular layouts: behind a row's frames acoustic_codes hold -1 (the dropped
 *                            code, as qa_hcodec_encode_ragged writes it) and emb holds exact zeros; emb, where given, must be 16-byte
 *                            aligned (those zeros are written as float4; checked, refused otherwise).  When every row sits at one offset and
 *                            frames[b] == n for all b the step IS qa_hcodec_stream_encode: same launches, same bits.
 *   qa_hcodec_stream_reset_rows  the named rows (HOST int64 [n_rows], distinct, 0 .. B - 1) back to offset 0: their next step with frames
 *                            is a first step (reflect fill, LSTM state zeroed, earlier K / V rows invisible); all other rows continue.
 *   qa_hcodec_stream_offsets out [B] (host): the code frames of every row since begin / its reset.  qa_hcodec_stream_offset returns the
 *                            largest of them - the one offset of a stream that only uses the calls above.
 * qa_hcodec_stream_encode on a stream whose rows sit at different offsets gives every row all n frames at its own offset.
 * Refused before anything is launched, state and every offset untouched: frames[b] outside 0 .. n; a row at offset 0 with 0 < frames[b] <
 * first_min_frames (let it idle until enough is buffered); offset[b] + frames[b] > max_frames for any row (the message names it); every
 * row idle; a row index out of range or named twice; a stream under capture; a handle that does not stream. */
int qa_hcodec_stream_encode_rows(qa_hcodec* h, const float* wav, int64_t n_samples, const int64_t* frames, int64_t* acoustic_codes, float* emb,
                                 void* stream);
int qa_hcodec_stream_reset_rows(qa_hcodec* h, const int64_t* rows, int64_t n_rows);
int qa_hcodec_stream_offsets(const qa_hcodec* h, int64_t* out);
/* The same stream without an end: the encoder's Transformer under a sliding window of left_context TRANSFORMER
 * frames (two per code frame), its K / V rows a ring (qa_transformer_stream_begin_ring).  The window is a property of the stream, not of
 * the spec.  This is NOT the shipped full-causal encoder: it is the SEANet encoder whose Transformer was built with
 * use_sliding_window=True, left_context=W, a parameter of the reference's block that vq/codec.py never sets; its embeddings and codes
 * differ from the full-causal ones.  max_chunk_frames (code frames, at least the first-chunk minimum) is the most one step may take per
 * row.  _encode, _encode_rows, _reset, _reset_rows, _offset(s) and _end are the calls above.  Refused before any launch: left_context
 * < 1, a ring above 8192 rows, a chunk above max_chunk_frames, a row past 2^24 Transformer positions (2^23 code frames, about 93 hours),
 * per-row lengths on a step of more than 8 code frames.  _capacity: the code frames the K / V rows hold (ring or linear), -1 when not
 * streaming. */
int qa_hcodec_stream_begin_ring(qa_hcodec* h, int64_t B, int32_t left_context, int64_t max_chunk_frames);
int64_t qa_hcodec_stream_capacity(const qa_hcodec* h);

/* H-Codec 1.5 (spec.adaptive != 0): Codec.encode / Codec.decode of QuarkAudio-HCodec/HCodec-1.5/vq/codec_adaptive.py:150-199.
 * The number of groups G is data dependent (the reference syncs the host too: modeling_flexicodec_new.py:910), so
 *   - encode writes int64 [B, nq, G] length-injected codes (code' = (len-1)*codebook_size + code) compactly into buffers of
 *     capacity B*nq*N25 elements and returns G through *n_groups (the call synchronises `stream` once);
 *   - qa_hcodec_adaptive_frames returns max_b sum_g len[b,g] (= N25 of the clip) for a batch of codes, so the caller can size
 *     wav_out = [B, frames * 2 * hop] before qa_hcodec_decode_adaptive.
 * threshold: the per-call similarity threshold of Codec.encode(..., threshold=t) (codec_adaptive.py:150-158): 0 = the model's
 *   manual_threshold (spec.threshold), otherwise in (0, 1]. */
int qa_hcodec_encode_adaptive(qa_hcodec* h, const float* wav, int64_t B, int64_t T,
                              const float* feat, int64_t feat_stride_b, int64_t feat_stride_c, int64_t feat_stride_t,
                              int64_t n_feat_frames, int64_t* acoustic_codes, int64_t* semantic_codes, int64_t* n_groups,
                              float threshold, void* stream);
int qa_hcodec_adaptive_frames(qa_hcodec* h, const int64_t* semantic_codes, int64_t B, int64_t G, int64_t* frames, void* stream);
int qa_hcodec_decode_adaptive(qa_hcodec* h, const int64_t* acoustic_codes, const int64_t* semantic_codes, int64_t B,
                              int64_t G, int64_t frames, float* wav_out, void* stream);

/* Per-clip lengths in one H-Codec 1.5 call (non-causal models): row b equals qa_hcodec_encode_adaptive /
 * _decode_adaptive on clip b alone (B = 1) at its own length, with its own group count and no padded query token among its keys - which the
 * rectangular calls above do not give even for clips of equal length (they keep the reference's batch semantics).  frames: HOST memory,
 * int64 [B], code frames 1 .. N each, checked before anything is launched (QA_ERR_INVALID names the row).  A call with lengths always
 * takes the masked path, also when every length is N.  spec.causal, causal aggregators and a causal bottleneck are QA_ERR_UNSUPPORTED.
 *   encode: N = T / encoder hop.  *n_groups is the largest group count G over the clips; codes are written compactly as [B, nq, G], and the
 *           entries of clip b behind its own groups are -1: in this wire format a legal entry of length 0 (floor(-1 / K) + 1 = 0), and the
 *           dropped code, so the output is valid input for qa_hcodec_decode_adaptive and for qa_hcodec_decode_adaptive_ragged.  Samples
 *           and feature frames behind a clip's length are never read.
 *   qa_hcodec_adaptive_clip_frames: sum_g len[b, g] of every row as host int64 [B] (qa_hcodec_adaptive_frames returns their maximum),
 *           behind the same single synchronisation.
 *   decode: codes [B, nq, G]; wav_out [B, 2 * N * hop].  Row b de-aggregates at most frames[b] frames, its bottleneck transformer and
 *           decoder see frames[b] frames, and wav_out[b] is exactly 0 from sample frames[b] * 2 * hop on. */
int qa_hcodec_encode_adaptive_ragged(qa_hcodec* h, const float* wav, int64_t B, int64_t T, const int64_t* frames,
                                     const float* feat, int64_t feat_stride_b, int64_t feat_stride_c, int64_t feat_stride_t,
                                     int64_t n_feat_frames, int64_t* acoustic_codes, int64_t* semantic_codes, int64_t* n_groups,
                                     float threshold, void* stream);
int qa_hcodec_adaptive_clip_frames(qa_hcodec* h, const int64_t* semantic_codes, int64_t B, int64_t G, int64_t* frames_out, void* stream);
int qa_hcodec_decode_adaptive_ragged(qa_hcodec* h, const int64_t* acoustic_codes, const int64_t* semantic_codes, int64_t B, int64_t G,
                                     int64_t N, const int64_t* frames, float* wav_out, void* stream);

/* Semantic decoder of H-Codec (semantic_module.Decoder, QuarkAudio-HCodec/HCodec-1.0/vq/semantic_module.py:205-300): it rebuilds
 * the SSL features from the summed semantic code vectors.  conv1 (k3, no bias) code_dim -> channels; block i: a Conv1d k3 (stride 1)
 * or a ConvTranspose1d k = 2 s (stride s > 1, even) from the previous width to widths[i], then two residual units; conv2 (k3, no bias)
 * widths[n_blocks - 1] -> output_channels.  Every width a multiple of 32. */
typedef struct qa_semantic_decoder_spec {
    int32_t code_dim, channels, n_blocks;
    int32_t strides[4];
    int32_t widths[4];
    int32_t output_channels;
} qa_semantic_decoder_spec;

/* Attach the semantic decoder to a codec handle (weights: `semantic_decoder.*` of the reference's state_dict, host memory).  It is
 * only read by qa_hcodec_forward*; encode / decode do not change.  On failure (first missing or mis-shaped key in the error message)
 * the handle keeps what it had. */
int qa_hcodec_load_semantic_decoder(qa_hcodec* h, const qa_semantic_decoder_spec* spec, const qa_tensor* tensors, int64_t n_tensors);
/* 1 if a semantic decoder is attached, 0 if not, negative on a null handle */
int qa_hcodec_has_semantic_decoder(const qa_hcodec* h);

/* Codec.forward in eval mode (HCodec-1.0/vq/codec.py:138-162, HCodec-2.0/vq/codec.py:54-72): encode, RVQ and decode on the device
 * (the codes never leave it), and the semantic decoder on the looked-up semantic embedding.  wav / feat as qa_hcodec_encode;
 * recon: fp32 [B, N25 * upsample * hop] (= decode(encode(wav, feat))); pred_feat: fp32 [B, output_channels, N25 * prod(strides)]. */
int qa_hcodec_forward(qa_hcodec* h, const float* wav, int64_t B, int64_t T,
                      const float* feat, int64_t feat_stride_b, int64_t feat_stride_c, int64_t feat_stride_t,
                      int64_t n_feat_frames, float* recon, float* pred_feat, void* stream);
/* H-Codec 1.5 (HCodec-1.5/vq/codec_adaptive.py:100-148) at the model's threshold (spec.threshold).  recon: fp32 [B, 2 * N25 * hop];
 * pred_feat as above, from the semantic embedding de-aggregated back to N25 frames; token_lengths: int64 [B, G] written compactly
 * into a buffer of capacity B * N25; G returned through *n_groups (one host synchronisation, as encode). */
int qa_hcodec_forward_adaptive(qa_hcodec* h, const float* wav, int64_t B, int64_t T,
                               const float* feat, int64_t feat_stride_b, int64_t feat_stride_c, int64_t feat_stride_t,
                               int64_t n_feat_frames, float* recon, float* pred_feat, int64_t* token_lengths, int64_t* n_groups,
                               void* stream);

/* Test hook: when enabled, encode/decode snapshot their named intermediates (costs copies; off by default). */
int qa_hcodec_enable_taps(qa_hcodec* h, int on);
/* Test hook: copy the named snapshot of the LAST encode/decode (still in the handle's workspace) into
 * `dst` (device, fp32, capacity `cap` elements).  Returns the element count or a negative status.  Layout is
 * the library's: time-major, channel-last ([B, frames, channels]).  Names: see DESIGN.md "taps". */
int64_t qa_hcodec_tap(qa_hcodec* h, const char* name, float* dst, int64_t cap, void* stream);

/* ---- kernel-level entry points (used by the parity tests and available to integrators) ------------- */

/* Residual nearest-codebook search.  x: [n_vec, D]; codebooks: [Q, K, D]; indices out: int64 [n_vec, Q];
 * quantized_out (nullable): [n_vec, D] = sum_q E_q[idx_q].  Ties resolve to the lowest index. */
int qa_rvq_search(const float* x, int64_t n_vec, const float* codebooks, int32_t Q, int32_t K, int32_t D,
                  int64_t* indices, float* quantized_out, void* stream);
/* indices: int64 [n_vec, Q] -> out [n_vec, D] = sum_q E_q[idx_q].  idx == -1 is a DROPPED code and contributes a zero vector, as in the
 * third-party ResidualVQ.get_output_from_indices the reference calls (vq/codec.py:183-184; upstream masks -1, the quantize-dropout
 * convention).  Other out-of-range indices are NOT detected on device (clamped for memory safety); the caller guarantees
 * -1 <= idx < K - qa_codes_check_async(codes, n, -1, K, ...) is the check (the reference would raise IndexError). */
int qa_rvq_lookup(const int64_t* indices, int64_t n_vec, const float* codebooks, int32_t Q, int32_t K, int32_t D,
                  float* out, void* stream);

/* Range check of integer codes before a decode (the reference's F.embedding raises IndexError on the host, or trips a device-side
 * assert on a GPU): *bad = number of entries of codes[0..n) outside [0, limit).  One tiny kernel + one 4-byte copy; synchronises
 * `stream`.  The decode entry points themselves never synchronise and clamp indices for memory safety. */
int qa_codes_check(const int64_t* codes, int64_t n, int64_t limit, int64_t* bad, void* stream);
/* The same check without a host synchronisation: *bad_count_dev (DEVICE int64, zeroed by the caller) += number of entries of
 * codes[0..n) outside [lo, limit).  The caller reads the counter after whatever synchronisation it performs anyway (the Python mirror
 * reads it behind the decode call's own: one host round trip per decode instead of two). */
int qa_codes_check_async(const int64_t* codes, int64_t n, int64_t lo, int64_t limit, int64_t* bad_count_dev, void* stream);

/* torchaudio.transforms.Resample(orig_freq, new_freq) with its defaults (sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99),
 * the 48 kHz -> 16 kHz step in front of HuBERT in H-Codec 2.0 (HCodec-2.0/audio_tokenizer.py:44,51).
 * qa_resample_length = ceil(new * T / orig) samples per clip; wav [B, T] -> out [B, qa_resample_length] (device). */
int64_t qa_resample_length(int64_t T, int32_t orig_freq, int32_t new_freq);
int qa_resample(const float* wav, int64_t B, int64_t T, int32_t orig_freq, int32_t new_freq, float* out, void* stream);
/* Per-clip lengths in one resample call: row b equals qa_resample on wav[b, :lengths[b]] alone.  lengths: HOST
 * memory, int64 [B], SAMPLES at orig_freq, 1 .. T each, checked before anything is launched (QA_ERR_INVALID names the row); the values
 * travel in the launches' arguments, nothing is copied from the caller's memory after the call returns.  Samples t >= lengths[b] are
 * never loaded (they read as zero); out[b, o] is written as exactly 0 for o >= qa_resample_length(lengths[b]), where a zero-filled
 * row would carry the filter's ringing. */
int qa_resample_ragged(const float* wav, int64_t B, int64_t T, const int64_t* lengths, int32_t orig_freq, int32_t new_freq, float* out,
                       void* stream);

/* Implicit-GEMM Conv1d over channel-last activations (covers nn.Linear with ksize = 1):
 *   y[b, t, n] = post( res[b,t,n] + gamma[n] * act( bias[n] + sum_{j,c} pro(x[b, src(t,j), c]) * w[n, j, c] ) )
 * with src(t,j) = t*stride - pad_left + j resolved by pad_mode (0 zero, 1 reflect as SConv1d does).
 * Exposed for kernel-level parity tests.  See DESIGN.md for the full argument contract. */
typedef struct qa_conv_args {
    const float* x;        /* [B, T_in, C_in] */
    const float* w;        /* [N, ksize, C_in]  (library layout) */
    const float* bias;     /* [N] or NULL */
    const float* gamma;    /* [N] or NULL */
    const float* residual; /* [B, T_out, N] (row stride ldr) or NULL */
    const float* gate;     /* [B, T_out, N] (row stride ldg) or NULL: y = silu(gate) * (acc + bias) */
    float* y;              /* [B, T_out, N] with row stride ldy */
    int64_t B, T_in, C_in, T_out, N;
    int64_t ldx;           /* row stride of x in floats (>= C_in) */
    int64_t ldy, ldr, ldg;
    int32_t ksize, stride, pad_left, pad_right, pad_mode;
    int32_t prologue;      /* 0 none, 1 ELU applied to x on load */
    int32_t act;           /* 0 none, 1 ELU, 2 GELU(erf), 3 SiLU, 6 ReLU */
    int32_t post_act;      /* applied after the residual add: 0 none, 1 ELU */
    int32_t in_rep;        /* 0/1 none; r > 1: x is read as x.repeat_interleave(r) along frames (zero padding only) */
} qa_conv_args;
int qa_conv1d_cl(const qa_conv_args* args, void* stream);

/* ---- pre-split weight images (knob QA_GEMM_PRESPLIT) ---------------------------------------------------------
 * conv_gemm's default arithmetic splits both operands into three bf16 planes.  Weights do not change between calls, so every model
 * handle builds the planes of all its weights once, at load, and its launches that take a 128-column tile read them instead of
 * splitting in the K loop (narrower tiles keep the in-loop split) - the same bits either way.  These entry points give a caller-owned weight (qa_conv1d_cl) the same route, and tests a way to read an image:
 *   qa_weight_planes         writes the image of the device array w[0 .. n), n % 8 == 0, into `planes` (6 n bytes of device memory,
 *                            16-byte aligned): per group of 8 floats three 16-byte units, the group's h, m and l planes as 8 bf16 each;
 *   qa_weight_planes_attach  from now on a qa_conv1d_cl whose weight (all N rows) lies inside w[0 .. n), on an 8-float boundary,
 *                            reads `planes` when it takes a 128-column tile; w must not change while attached, and ranges must not overlap;
 *   qa_weight_planes_detach  undoes it (before either buffer is freed);
 *   qa_weight_planes_bytes   bytes of all images attached in this process, the handles' included;
 *   qa_weight_plane_offset   host logic, no device: byte offset inside the image of element `index`, plane 0 (h), 1 (m) or 2 (l). */
int qa_weight_planes(const float* w, int64_t n, void* planes, void* stream);
int qa_weight_planes_attach(const float* w, int64_t n, const void* planes);
int qa_weight_planes_detach(const float* w);
int64_t qa_weight_planes_bytes(void);
int64_t qa_weight_plane_offset(int64_t index, int32_t plane);

/* ---- host logic exposed for CPU tests (no device needed) ------------------------------------------------
 * SConv1d geometry of the reference (encoder_modules/conv.py:54-61,195-211, non-causal): for an input of L frames,
 * kernel k (dilation 1) and stride s it yields T_out = ceil(L/s) and the (left, right + extra) reflect paddings. */
int qa_sconv_geometry(int64_t L, int32_t ksize, int32_t stride, int64_t* T_out, int32_t* pad_left, int32_t* pad_right);
/* Source frame read by padded position r of an L-frame signal: index in [0, L) or -1 for "reads zero".  pad_mode 0 zero,
 * 1 reflect with the short-input rule of pad1d (encoder_modules/conv.py:79-96); max_pad = max(pad_left, pad_right). */
int64_t qa_resolve_frame(int64_t r, int64_t L, int32_t max_pad, int32_t pad_mode);

/* ---- measurement hook (bench.py) ------------------------------------------------------------------------
 * Between qa_profile_begin() and qa_profile_end() every implicit-GEMM launch is bracketed by HIP events recorded on
 * the stream it is launched on.  qa_profile_end fills out[cfg*4 + {0,1,2,3}] = {algorithmic FLOPs, elapsed ms, launches,
 * algorithmic bytes (input frames + weights + outputs + fused residual / gate reads, each once)} for the six tile
 * configurations cfg = 0 (128x32), 1 (128x64), 2 (128x128), 3 (64x128), 4 (64x64), 5 (256x128); n_out >= 24.  Not thread-safe;
 * process-wide. */
int qa_profile_begin(void);
int qa_profile_end(double* out, int32_t n_out);
/* qa_profile_begin_ex(mask): bit 0 = the implicit-GEMM launches (= qa_profile_begin), bit 1 = the byte-bound kernels (norms, depthwise
 * conv, RoPE, ISTFT, RVQ look-up / pick, the fused SEANet front ...), each recorded with its ALGORITHMIC bytes (every input and output
 * element once).  qa_profile_end_hbm (call it before qa_profile_end) fills out[kind*3 + {0,1,2}] = {bytes, elapsed ms, launches} for
 * kind in [0, qa_profile_hbm_kinds()); n_out >= 3 * kinds; qa_profile_hbm_name(kind) names the kernel.  bytes / ms = achieved GB/s
 * against the HBM roofline (bench.py's `roofline_hbm`). */
int qa_profile_begin_ex(int32_t mask);
int qa_profile_hbm_kinds(void);
const char* qa_profile_hbm_name(int32_t kind);
int qa_profile_end_hbm(double* out, int32_t n_out);
/* qa_set_serial(1) (or QA_SERIAL=1 in the environment) collapses the library's internal streams onto the caller's, so that a
 * profiler sees every kernel alone on the device; results are bit-identical either way.  Process-wide. */
int qa_set_serial(int32_t on);

/* Diagnostics of the in-launch LSTM recurrences of `device` (tests): out[0] recurrences launched so far, out[1] model-graph calls with
 * one possibly still in flight (not yet behind a host synchronisation), out[2] launches that took the per-step kernels because ANOTHER
 * call's recurrence was in flight (the co-residency ticket: two handles driving one device never starve each other's grid barrier),
 * out[3] 1 once a barrier time-out has degraded the device to the per-step kernels. */
int qa_debug_lstm_stats(int32_t device, int64_t* out4);
/* One LSTM recurrence alone, as a model graph issues it (tests): xw [B, T, 4d] = x W_ih^T + b_ih + b_hh and w_hh [4d, d] with the 4d
 * axis in (unit, gate) order, h_out [B, T, d], c_state [B, d] scratch; zero initial state.  The library chooses the kernel as it does
 * inside a codec call (knobs QA_LSTM_XCD, QA_LSTM_TEAM, QA_LSTM_PERSISTENT).  Waits for an in-launch recurrence and returns an error,
 * without re-running on the per-step kernels, if its step barrier timed out. */
int qa_debug_lstm(const float* xw, const float* w_hh_ug, float* h_out, float* c_state, int B, int T, int d, void* stream);
/* One chunk of a recurrence that continues (tests; the streaming Transformer's LSTM): as qa_debug_lstm on the per-step kernels, but step 0
 * starts from h_state / c_state [B, d], and both hold the state behind step T - 1 when the chunk has run. */
int qa_debug_lstm_carry(const float* xw, const float* w_hh_ug, float* h_out, float* h_state, float* c_state, int B, int T, int d,
                        void* stream);
/* The window of one causal convolution in a stream and its next state, alone (tests; stream_conv.hip): win
 * [B, ctx + n, C] = head | chunk [B, n, C], the head being state_in [B, ctx, C] or, with first != 0 (n > ctx), the reflection of the chunk
 * (position -1 - j reads frame 1 + j; state_in may then be NULL); state_out [B, ctx, C] = the last ctx rows of the window.  state_in and
 * state_out must be different buffers: for n < ctx the next state takes rows of the current one. */
int qa_debug_stream_window(const float* state_in, const float* chunk, float* win, float* state_out, int B, int ctx, int n, int C, int first,
                           void* stream);
/* The same with per-row lengths (tests): n_rows_dev / first_dev are DEVICE int [B].  Item b holds n_b = n_rows_dev[b]
 * (0 .. n) live chunk rows and takes the reflected head iff first_dev[b] != 0 (which needs n_b > ctx), else state_in (not NULL here).  Its
 * window is head | its n_b chunk rows | 0.0f - chunk rows behind n_b are never read - and state_out[b] is window rows n_b .. n_b + ctx - 1;
 * n_b = 0 copies state_in[b].  state_in == state_out is refused. */
int qa_debug_stream_window_rows(const float* state_in, const float* chunk, float* win, float* state_out, int B, int ctx, int n, int C,
                                const int* n_rows_dev, const int* first_dev, void* stream);
/* qa_debug_lstm_carry with per-row step counts (tests): nq_dev / zero_dev are DEVICE int [B].  Row b runs its first
 * nq_dev[b] (0 .. T) steps, from a zero state where zero_dev[b] != 0, and carries the state behind its own last step; a row with
 * nq_dev[b] = 0 and zero_dev[b] = 0 keeps its (h, c) bit for bit.  h_out rows behind a row's steps are unspecified (finite scratch). */
int qa_debug_lstm_carry_rows(const float* xw, const float* w_hh_ug, float* h_out, float* h_state, float* c_state, int B, int T, int d,
                             const int* nq_dev, const int* zero_dev, void* stream);
/* One rope-append plus attention of a stream step over K / V caches [B, cap, H hd] the caller owns (tests; DESIGN.md sections 42, 46):
 * qkv [B n, 3 H hd] (q is roped in place), out [B n, H hd], hd 64 / 96 / 128, window `context` (0: none).  Every item sits at pos0, or -
 * row_pos0_dev / row_nq_dev, DEVICE int [B], both or neither - item b at row_pos0_dev[b] with its first row_nq_dev[b] frames.  ring != 0:
 * the caches are rings (context >= 1, cap >= context - 1 + n, positions below 2^24), else linear (pos0 + n <= cap).  long_form != 0:
 * attention_kernel in place of the short kernel (n <= 16) - rows moving together only; its ring mode needs cap >= context + n and
 * every row of the ring finite.  The RoPE table and the partial records are the call's own; synchronous. */
int qa_debug_stream_attn(float* qkv, float* kc, float* vc, float* out, int B, int n, int H, int hd, int cap, int context, int ring, int pos0,
                         const int* row_pos0_dev, const int* row_nq_dev, int long_form, void* stream);
/* Attention launches the host has issued in this process so far, by arithmetic (tests): out2[0] the fp32 chain (QA_ATT_MATH = 0, and
 * every launch of a UniSE LM handle), out2[1] split-6.  Counted where the host launches: a launch recorded into a captured graph counts
 * once, at capture, and its replays do not count. */
int qa_debug_att_stats(int64_t* out2);

/* ---- tuning knobs -------------------------------------------------------------------------------------------
 * Every A/B switch of the library is one row of a table (csrc/knobs.h; INTEGRATION.md lists them): an integer whose initial
 * value is the environment variable of the same name (e.g. QA_LSTM_PERSISTENT, QA_LM_MLP_FUSED) and which qa_set_knob()
 * overrides at run time.  Knobs are read by the host-side launch code at launch (QA_LM_MLP_FUSED: at qa_lm_create) time.  No knob changes results beyond fp32 summation order - except the opt-in reduced-precision values 2 / 3 of QA_GEMM_MATH; none selects a CPU path.  Process-wide. */
int qa_knob_count(void);
int qa_knob_info(int32_t index, const char** name, int64_t* value, int64_t* default_value, const char** doc);
int qa_set_knob(const char* name, int64_t value);
int qa_get_knob(const char* name, int64_t* value);

/* ---- SSL front-end ---------------------------------------------------------------------------
 * HCodecTokenizer.extract_wav2vec2_features (QuarkAudio-HCodec/HCodec-1.0/audio_tokenizer.py:35-48, HCodec-1.5/audio_tokenizer.py:53-67):
 * and UniSE's Model.extract_semantic_features (QuarkAudio-UniSE/model/model.py:38-51, microsoft/wavlm-base-plus, no compression):
 * zero-pad `pad` samples each side, run the HuBERT / wav2vec 2.0 / WavLM model (transformers HubertModel / Wav2Vec2Model / WavLMModel: 7-layer
 * Conv1d feature extractor, feature projection, grouped positional convolution, post-LN or stable-LN encoder), average the
 * selected hidden states, compress sign * |x|^e.  Weights: the HF state_dict (keys feature_extractor.conv_layers.*,
 * feature_projection.*, encoder.pos_conv_embed.conv.{parametrizations.weight.original0/1 | weight_g/weight_v | weight}, ...). */
typedef struct qa_ssl_spec {
    int32_t n_conv;             /* 7 */
    int32_t conv_dim[8];        /* 512 x 7 */
    int32_t conv_kernel[8];     /* 10,3,3,3,3,2,2 */
    int32_t conv_stride[8];     /* 5,2,2,2,2,2,2 */
    int32_t conv_bias;          /* 0 HuBERT base; 1 wav2vec2-large / XLSR */
    int32_t feat_norm_layer;    /* 0 = "group" (GroupNorm on layer 0 only), 1 = "layer" (LayerNorm after every conv) */
    int32_t hidden;             /* 768 / 1024 */
    int32_t n_layers;           /* 12 / 24 */
    int32_t n_heads;            /* 12 / 16 */
    int32_t intermediate;       /* 3072 / 4096 */
    int32_t stable_layer_norm;  /* 0 post-LN (base), 1 pre-LN + final LN (large / XLSR) */
    int32_t pos_kernel;         /* 128 */
    int32_t pos_groups;         /* 16 */
    int32_t pad;                /* 160 (F.pad(wavs, (160, 160))) */
    int32_t n_select;           /* number of hidden states averaged; 0 = all n_layers + 1 (torch.stack(hidden_states).mean) */
    int32_t select[32];         /* their indices into hidden_states (1.5: 11, 14, 16) */
    float layer_norm_eps;       /* 1e-5 */
    float compress_exponent;    /* 0.3; <= 0: return the plain average (UniSE, QuarkAudio-UniSE/model/model.py:38-51) */
    int32_t rel_pos_buckets;    /* 0 HuBERT / wav2vec2; 320 WavLM: gated relative position bias (WavLMAttention), keys
                                   encoder.layers.0.attention.rel_attn_embed.weight, ...attention.gru_rel_pos_{linear,const} */
    int32_t rel_pos_max_distance; /* 800 */
} qa_ssl_spec;
typedef struct qa_ssl qa_ssl;
int qa_ssl_create(qa_ssl** out, const qa_ssl_spec* spec, const qa_tensor* tensors, int64_t n_tensors, int device);
void qa_ssl_destroy(qa_ssl* h);
/* frames the model yields for T samples (after padding); negative status when T is too short */
int64_t qa_ssl_frames(const qa_ssl* h, int64_t T);
/* wav float32 [B, T] (device) -> feats float32 [B, frames, hidden] (device, channel-last: what qa_hcodec_encode takes as `feat`
 * with strides (frames*hidden, 1, hidden)) */
int qa_ssl_forward(qa_ssl* h, const float* wav, int64_t B, int64_t T, float* feats, void* stream);
/* The same for a batch of clips of different lengths: row b of wav [B, T] holds a clip in its first lengths[b]
 * samples, and behaves as qa_ssl_forward would for those samples alone - `pad` zeros on each side of ITS samples, its GroupNorm over its
 * own frames, the positional convolution zero-padded at its own end, attention over its own keys.  feats is [B, qa_ssl_frames(T), hidden]:
 * n_b = qa_ssl_frames(lengths[b]) frames in feats[b, :n_b], exactly 0.0f in feats[b, n_b:].  What wav holds behind a clip's end is never
 * read.  lengths: HOST memory, int64 [B], in SAMPLES, each from the shortest input that yields one frame up to T; read during the call
 * (the caller may free it on return) and checked before anything is launched - QA_ERR_INVALID names the row and its value
 * ("lengths[1] = 79 ...").  lengths == NULL, or every entry equal to T, is qa_ssl_forward: the same launches, bit-identical output. */
int qa_ssl_forward_ragged(qa_ssl* h, const float* wav, int64_t B, int64_t T, const int64_t* lengths, float* feats, void* stream);

/* ---- mimi StreamingTransformer: causal / context windows and the streaming state --------------------------
 * Replaces StreamingTransformer (QuarkAudio-HCodec/HCodec-1.5/adaptive/model_blocks/mimi/transformer.py:605-698) in the
 * configuration H-Codec 1.5 instantiates it with (:722-736): positional_embedding "rope", norm "layer_norm", gating "none",
 * LayerScale, no biases.  Weights: `<prefix>.layers.N.{self_attn.in_proj_weight, self_attn.out_proj.weight, norm1.*, norm2.*,
 * linear1.weight, linear2.weight, layer_scale_1.scale, layer_scale_2.scale}`.
 *   qa_mimi_forward       forward() outside streaming: no mask unless causal; causal: key j visible to query i iff
 *                         0 <= i - j < context (context 0 = unbounded)                          (transformer.py:403-413)
 *   qa_mimi_stream_begin  `with model.streaming(B)` / streaming_forever(B): one RingKVCache of capacity `context` per layer
 *                         (:212-241,345-370); needs causal = 1 and context > 0 like the reference (:349-353,382)
 *   qa_mimi_stream_step   forward() inside streaming on a chunk x [B, T, d], T <= context: RoPE at the running offset, the
 *                         chunk's keys / values written to slots (offset + t) % context BEFORE the queries attend, positions
 *                         and validity of the slots as RingKVCache.complete() computes them (:243-281) - including its
 *                         treatment of the slot at the write cursor, which leaves context - 1 visible keys per query
 *   qa_mimi_stream_reset  reset_streaming(): offsets to zero, cache contents kept but invisible (:239-241)
 *   qa_mimi_stream_end    leaving the context manager (streaming.py:100-105)
 * x and y are fp32 [B, T, d_model] device buffers (y may alias x). */
typedef struct qa_mimi_spec {
    int32_t d_model;          /* 512 / 1024 */
    int32_t num_heads;        /* 8 */
    int32_t num_layers;       /* 32 */
    int32_t dim_feedforward;  /* 2048 */
    int32_t causal;           /* config_adaptive_v3.yaml ships false */
    int32_t context;          /* 16 */
} qa_mimi_spec;
typedef struct qa_mimi qa_mimi;
int qa_mimi_create(qa_mimi** out, const qa_mimi_spec* spec, const qa_tensor* tensors, int64_t n_tensors, const char* prefix,
                   int device);
void qa_mimi_destroy(qa_mimi* m);
int qa_mimi_forward(qa_mimi* m, const float* x, int64_t B, int64_t T, float* y, void* stream);
int qa_mimi_stream_begin(qa_mimi* m, int64_t B);
int qa_mimi_stream_step(qa_mimi* m, const float* x, int64_t T, float* y, void* stream);
int qa_mimi_stream_reset(qa_mimi* m);
int qa_mimi_stream_end(qa_mimi* m);
/* tokens seen since begin / reset; -1 outside streaming */
int64_t qa_mimi_stream_offset(const qa_mimi* m);

/* ---- codec Transformer: offline, cache mode and a streaming state ------------------------------------
 * The block every H-Codec version runs in its encoder and decoder (QuarkAudio-HCodec/HCodec-1.0/vq/encoder_modules/transformer.py:396-489:
 * RMSNorm -> nn.LSTM -> QKV + rotate-half RoPE -> attention -> O, RMSNorm -> SwiGLU), on its own.  Weights: `<prefix>.layers.N.
 * {self_attn.rnn.{weight,bias}_{ih,hh}_l0, self_attn.{q,k,v}_proj.{weight,bias}, self_attn.o_proj.weight, input_layernorm.weight,
 * post_attention_layernorm.weight, mlp.w1/w2/w3.weight}`.  x and y are fp32 [B, frames, hidden_size] device buffers, x != y.
 *   qa_transformer_forward         forward(x): no mask; causal: key j visible to query i iff j <= i and (left_context == 0 or
 *                                  i - j < left_context)                                                      (transformer.py:436-475)
 *   qa_transformer_cache_*         past_key_values: per layer the roped K and V rows [B, capacity, d], capacity <= 8192
 *   qa_transformer_forward_cached  forward(x, past_key_values, use_cache=True) as the reference runs it: the LSTM starts from zero on
 *                                  every call (:133), RoPE at positions len .. len + n - 1 (:459-467), keys = cache | chunk.  Non-causal:
 *                                  every query sees every key, the later ones of its own chunk included.  Causal with an empty cache: the
 *                                  offline causal call, which also fills the cache.  Causal with a non-empty cache is refused - the
 *                                  reference's (T, T) mask cannot be combined with cached keys and raises there.
 *   qa_transformer_stream_*        what the reference cannot do and the causal graph allows exactly: the concatenated outputs of any
 *                                  chunking equal qa_transformer_forward of the concatenated input (up to fp32 summation order).  State
 *                                  per layer: the LSTM's (h, c) and the K / V rows; one running offset.  A step of n frames carries the
 *                                  recurrence on from (h, c), ropes at offset + t, writes its K / V rows, then attends: the query at
 *                                  p = offset + i sees key j iff j <= p and (left_context == 0 or p - j < left_context).  Needs causal = 1.
 *                                  offset + n > capacity is refused before anything is launched and leaves the state untouched.
 *                                  _reset: offset and LSTM states to zero (cached rows stay and are invisible); _offset: frames since
 *                                  begin / reset, -1 outside streaming. */
typedef struct qa_transformer_spec {
    int32_t hidden_size;          /* 512 / 768 / 1024 / 1536; a multiple of 128 */
    int32_t intermediate_size;
    int32_t num_attention_heads;  /* head_dim = hidden_size / heads in {64, 96, 128} */
    int32_t num_hidden_layers;
    int32_t causal;
    int32_t left_context;         /* > 0: use_sliding_window with this left_context; needs causal */
} qa_transformer_spec;
typedef struct qa_transformer qa_transformer;
typedef struct qa_transformer_cache qa_transformer_cache;
int qa_transformer_create(qa_transformer** out, const qa_transformer_spec* spec, const qa_tensor* tensors, int64_t n_tensors,
                          const char* prefix, int device);
void qa_transformer_destroy(qa_transformer* h);
int qa_transformer_forward(qa_transformer* h, const float* x, int64_t B, int64_t T, float* y, void* stream);
int qa_transformer_cache_create(qa_transformer* h, int64_t B, int64_t capacity, qa_transformer_cache** out);
void qa_transformer_cache_destroy(qa_transformer_cache* c);
int64_t qa_transformer_cache_length(const qa_transformer_cache* c);
int qa_transformer_cache_reset(qa_transformer_cache* c);
int qa_transformer_forward_cached(qa_transformer* h, qa_transformer_cache* cache, const float* x, int64_t B, int64_t n, float* y,
                                  void* stream);
int qa_transformer_stream_begin(qa_transformer* h, int64_t B, int64_t capacity);
int qa_transformer_stream_step(qa_transformer* h, const float* x, int64_t n, float* y, void* stream);
int qa_transformer_stream_reset(qa_transformer* h);
int qa_transformer_stream_end(qa_transformer* h);
int64_t qa_transformer_stream_offset(const qa_transformer* h);
/* Per-row lengths, offsets and resets, the block-level twin of qa_hcodec_stream_encode_rows in Transformer frames:
 * row b consumes its first frames[b] (HOST int64 [B], 0 .. n) rows of x [B, n, d] at its own offset; x behind them is never read, y there
 * is exact zeros (x and y 16-byte aligned: checked); an idle row keeps its state and offset.  _reset_rows: the named rows (HOST, distinct) back to offset 0, their LSTM state
 * zeroed by their next step; _offsets: out [B] (host); _offset returns the largest.  Rows that move together with frames[b] == n take the
 * launches of qa_transformer_stream_step.  Refused before any launch, everything untouched: frames[b] outside 0 .. n, offset[b] + frames[b]
 * > capacity (the row is named), every row idle, a row index out of range or repeated, a stream under capture, and - with left_context > 0 -
 * a ragged step that does not fit the short-chunk attention (more than 16 frames, QA_TR_SHORT_ATTN = 0, or over 256 query rows under
 * QA_TR_SHORT_ATTN = 1): the long-chunk attention has its per-item form without a window only. */
int qa_transformer_stream_step_rows(qa_transformer* h, const float* x, int64_t n, const int64_t* frames, float* y, void* stream);
int qa_transformer_stream_reset_rows(qa_transformer* h, const int64_t* rows, int64_t n_rows);
int qa_transformer_stream_offsets(const qa_transformer* h, int64_t* out);
/* A stream without an end: under a sliding window (causal, left_context = W > 0) the K / V rows are RINGS of
 * qa_transformer_stream_capacity rows - the smallest multiple of 32 that is at least W + max_chunk - and position p sits in row p mod
 * capacity.  _begin_ring replaces _begin (on a handle that already streams it frees the old stream); _step, _step_rows, _reset,
 * _reset_rows, _offset(s) and _end are the calls above, unchanged.  A step takes at most max_chunk frames per row at any offset below
 * 2^24 positions (a float holds those exactly); until the ring wraps, a step on the short-chunk attention gives the bits of a linear
 * stream of the same capacity.  Positions at or beyond the 8192 of the static RoPE table take their angle from the table's own formula.
 * Refused before any launch, state untouched, the message naming the value: a handle without a window, a capacity above 8192 rows, a
 * chunk above max_chunk (the row is named), a row that would pass 2^24 positions, a stream under capture, per-row lengths on a chunk that
 * does not fit the short-chunk attention.  _capacity: the rows of the cache of a ring or linear stream, -1 when not streaming. */
int qa_transformer_stream_begin_ring(qa_transformer* h, int64_t B, int64_t max_chunk);
int64_t qa_transformer_stream_capacity(const qa_transformer* h);

/* ---- BiCodec detokenizer ------------------------------------------------------------------------
 * BiCodec.detokenize(semantic_tokens, global_tokens) (QuarkAudio-UniSE/model/bicodec/bicodec.py:182-199), the stage
 * Model.test_step ends with (model/model.py:193,223): codebook look-up + out_project, FSQ look-up + speaker projection (d-vector),
 * the AdaLN-Vocos prenet, and the Snake / ConvTranspose1d / dilated-residual wave generator.  Shapes of the Spark-TTS BiCodec
 * checkpoint (its config.yaml is not part of the reference tree) are the defaults of unified_audio_amd.BiCodecSpec.
 * Weights: the `BiCodec.state_dict()` entries quantizer.codebook / quantizer.out_project, speaker_encoder.quantizer.project_out,
 * speaker_encoder.project, prenet.*, decoder.* (weight_g / weight_v or plain weight). */
typedef struct qa_bicodec_spec {
    int32_t latent_dim;        /* 1024  quantizer.input_dim = prenet in / out = d-vector width = decoder.input_channel */
    int32_t codebook_size;     /* 8192 */
    int32_t codebook_dim;      /* 8 */
    int32_t spk_latent_dim;    /* 128 */
    int32_t token_num;         /* 32 global tokens */
    int32_t n_levels;          /* 6 */
    int32_t levels[8];         /* 4,4,4,4,4,4 (FSQ) */
    int32_t vocos_dim;         /* 384 */
    int32_t vocos_inter;       /* 2048 */
    int32_t vocos_layers;      /* 12 */
    int32_t gen_channels;      /* 1536 */
    int32_t n_rates;           /* 4 */
    int32_t rates[8];          /* 8,5,4,2 */
    int32_t kernel_sizes[8];   /* 16,11,8,4 */
} qa_bicodec_spec;
typedef struct qa_bicodec qa_bicodec;
int qa_bicodec_create(qa_bicodec** out, const qa_bicodec_spec* spec, const qa_tensor* tensors, int64_t n_tensors, int device);
void qa_bicodec_destroy(qa_bicodec* h);
/* samples per semantic token = prod(rates) (320) */
int64_t qa_bicodec_hop(const qa_bicodec* h);
/* semantic_tokens int64 [B, T], global_tokens int64 [B, token_num] (the reference's [B, 1, token_num], contiguous) -> wav_out
 * fp32 [B, T * hop] (the reference returns [B, 1, T * hop]).  Out-of-range tokens are clamped for memory safety only: validate
 * with qa_codes_check where the reference's F.embedding would raise. */
int qa_bicodec_detokenize(qa_bicodec* h, const int64_t* semantic_tokens, const int64_t* global_tokens, int64_t B, int64_t T,
                          float* wav_out, void* stream);
/* Per-clip lengths in one call: clip b behaves as qa_bicodec_detokenize would for it alone at its own length.
 * lengths: HOST memory, int64 [B], the clips' lengths in TOKENS, 1 .. T each, read during the call (the caller may free it on return)
 * and checked before anything is launched (QA_ERR_INVALID names the row and its value).  Entries of semantic_tokens at or behind
 * lengths[b] are ignored, whatever they hold (-1 included): they are never read.  wav_out fp32 [B, T * hop]: wav_out[b] is exactly 0
 * from sample lengths[b] * hop on.  global_tokens have no length.  A call whose lengths all equal T is the rectangular call, through the
 * same launches. */
int qa_bicodec_detokenize_ragged(qa_bicodec* h, const int64_t* semantic_tokens, const int64_t* global_tokens, int64_t B, int64_t T,
                                 const int64_t* lengths, float* wav_out, void* stream);
/* test hooks, as qa_hcodec_enable_taps / qa_hcodec_tap: z_q, d_vector, prenet.down, prenet.backbone, prenet.out, gen.block{i} */
int qa_bicodec_enable_taps(qa_bicodec* h, int on);
int64_t qa_bicodec_tap(qa_bicodec* h, const char* name, float* dst, int64_t cap, void* stream);

/* ---- BiCodec encoder side: tokenize (semantic + global tokens) -----------------------------------------------------
 * BiCodec.get_semantic_tokens(batch) (QuarkAudio-UniSE/model/bicodec/bicodec.py:167-172): the XLSR-53 feature mix [B, N, 1024]
 * -> Encoder (VocosBackbone 1024 -> 384 with vocos_layers ConvNeXt layers, two ratio-1 SamplingBlocks (3 x) each followed by a
 * 2-layer VocosBackbone, Linear 384 -> latent_dim; modules/encoder_decoder/feat_encoder.py:29-92) -> FactorizedVectorQuantize.tokenize
 * (weight-normed 1x1 in_project latent_dim -> codebook_dim, F.normalize of latents and codebook, nearest code with the first
 * index winning a tie; modules/vq/factorized_vector_quantize.py:148-152,169-187), and BiCodec.get_global_tokens(batch)
 * (bicodec.py:174-178): mel spectrogram of the reference clip (torchaudio MelSpectrogram, power 1, slaney, no log) -> ECAPA-TDNN latent
 * (speaker/ecapa_tdnn.py, the pooling / x-vector head is not needed) -> PerceiverResampler (speaker/perceiver_encoder.py) -> ResidualFSQ
 * indices (fsq/residual_fsq.py, one quantizer).  A handle of its own: a detokenize-only checkpoint never needs these weights.
 * Weights: the `BiCodec.state_dict()` entries encoder.*, quantizer.in_project.* (weight_g / weight_v or plain weight),
 * quantizer.codebook.weight, speaker_encoder.speaker_encoder.* (BatchNorm running statistics folded into per-channel epilogue
 * constants), speaker_encoder.perceiver_sampler.* and speaker_encoder.quantizer.project_in.*. */
typedef struct qa_bicodec_enc_spec {
    int32_t input_channels;    /* 1024  encoder.input_channels (XLSR-53 hidden width) */
    int32_t vocos_dim;         /* 384 */
    int32_t vocos_inter;       /* 2048 */
    int32_t vocos_layers;      /* 12    layers of the input backbone (the two backbones behind the SamplingBlocks have 2) */
    int32_t latent_dim;        /* 1024  encoder.out_channels = quantizer.input_dim */
    int32_t codebook_size;     /* 8192 */
    int32_t codebook_dim;      /* 8 */
    /* global tokens: mel_params (bicodec.py:201-221) and the speaker encoder (speaker_encoder.py:33-60) */
    int32_t sample_rate;       /* 16000 */
    int32_t n_fft;             /* 1024 */
    int32_t win_length;        /* 640   must be 2 * hop_length (the framed-signal DFT) */
    int32_t hop_length;        /* 320 */
    float mel_fmin;            /* 10 */
    float mel_fmax;            /* 0 = sample_rate / 2 (mel_fmax: null) */
    int32_t mel_dim;           /* 128   num_mels = speaker_encoder.input_dim */
    int32_t ecapa_channels;    /* 512 */
    int32_t spk_latent_dim;    /* 128 */
    int32_t token_num;         /* 32 */
    int32_t n_levels;          /* 6 */
    int32_t levels[8];         /* 4,4,4,4,4,4 */
    int32_t perceiver_depth;   /* 2 */
    int32_t perceiver_heads;   /* 8 */
    int32_t perceiver_dim_head;/* 64 */
} qa_bicodec_enc_spec;
typedef struct qa_bicodec_enc qa_bicodec_enc;
int qa_bicodec_enc_create(qa_bicodec_enc** out, const qa_bicodec_enc_spec* spec, const qa_tensor* tensors, int64_t n_tensors, int device);
void qa_bicodec_enc_destroy(qa_bicodec_enc* h);
/* feat fp32 [B, N, input_channels] channel-last (the reference's batch["feat"], contiguous) -> semantic_out int64 [B, N] */
int qa_bicodec_get_semantic_tokens(qa_bicodec_enc* h, const float* feat, int64_t B, int64_t N, int64_t* semantic_out, void* stream);
/* wav fp32 [B, T] -> global_out int32 [B, token_num] (the reference's [B, 1, token_num]).  The mel spectrogram is taken of the
 * reference clip of ref_len samples: wav[b, k % T] for k < ref_len, BiCodecTokenizer.get_ref_clip's tile-and-truncate
 * (audio_tokenizer.py:54-72) as index arithmetic; ref_len <= 0 takes the rows as they are (BiCodec.get_global_tokens on batch["ref_wav"]).
 * ref_len must exceed n_fft / 2 (the reflect padding of the centred STFT). */
int qa_bicodec_get_global_tokens(qa_bicodec_enc* h, const float* wav, int64_t B, int64_t T, int64_t ref_len, int32_t* global_out,
                                 void* stream);
/* BiCodec.tokenize(batch) (bicodec.py:151-165): both of the above on one stream */
int qa_bicodec_tokenize(qa_bicodec_enc* h, const float* feat, int64_t B, int64_t N, const float* ref_wav, int64_t T_ref, int64_t ref_len,
                        int64_t* semantic_out, int32_t* global_out, void* stream);
/* Per-clip lengths in one call: row b behaves as the rectangular call above would for that clip alone at its own
 * length.  Every length vector is HOST memory, int64 [B], read during the call (the caller may free it on return) and checked before
 * anything is launched (QA_ERR_INVALID names the entry point, the row and its value); a vector whose entries all equal the full extent
 * makes the rectangular call, through the same launches.
 *   get_semantic_tokens_ragged: frame_lengths in FEATURE FRAMES, 1 .. N each.  Rows of feat at or behind frame_lengths[b] are padding
 *       that is never read (NaN there changes nothing); semantic_out[b, n] = -1 for n >= frame_lengths[b].
 *   get_global_tokens_ragged: lengths in SAMPLES, 1 .. T each.  The reference clip of row b is wav[b, k % lengths[b]] for k < ref_len:
 *       get_ref_clip on the clip alone; samples at or behind lengths[b] are never read.  ref_len must be positive unless every length is T.
 *   tokenize_ragged: both of the above on one stream, every check of both in front of the first launch.  The two vectors count
 *       different things: frame_lengths the rows of feat, lengths the samples of ref_wav (the front-end's frame rule relates them,
 *       qa_ssl_frames). */
int qa_bicodec_get_semantic_tokens_ragged(qa_bicodec_enc* h, const float* feat, int64_t B, int64_t N, const int64_t* frame_lengths,
                                          int64_t* semantic_out, void* stream);
int qa_bicodec_get_global_tokens_ragged(qa_bicodec_enc* h, const float* wav, int64_t B, int64_t T, const int64_t* lengths, int64_t ref_len,
                                        int32_t* global_out, void* stream);
int qa_bicodec_tokenize_ragged(qa_bicodec_enc* h, const float* feat, int64_t B, int64_t N, const int64_t* frame_lengths, const float* ref_wav,
                               int64_t T_ref, const int64_t* lengths, int64_t ref_len, int64_t* semantic_out, int32_t* global_out,
                               void* stream);
/* test hooks: enc.backbone (input backbone), enc.down (after the SamplingBlock stages), enc.out [B, N, latent_dim],
 * vq.latent [B * N, codebook_dim] (in_project output after F.normalize); mel [B, frames, mel_dim], ecapa.layer1 [B, frames, C],
 * ecapa.layers234 [B, frames, 3 C] (the concatenation of the three SE-Res2 block outputs), ecapa.latent [B, frames, 1536],
 * perceiver.out [B, token_num, spk_latent_dim], fsq.bounded [B, token_num, n_levels] */
int qa_bicodec_enc_enable_taps(qa_bicodec_enc* h, int on);
int64_t qa_bicodec_enc_tap(qa_bicodec_enc* h, const char* name, float* dst, int64_t cap, void* stream);
/* Wav2Vec2FeatureExtractor(do_normalize=True) on equal-length rows (audio_tokenizer.py:74-90, nothing padded):
 * out[b, :] = (wav[b, :] - mean) / sqrt(var + eps) with the population variance; eps = 1e-7 in the reference.  out may alias wav. */
int qa_wav_normalize(const float* wav, int64_t B, int64_t T, float* out, float eps, void* stream);
/* Rows of unequal length: lengths is HOST memory, int64 [B], in SAMPLES, 1 .. T each, read during the call and
 * checked before anything is launched (QA_ERR_INVALID names the row and its value).  out[b, :lengths[b]] is the row above of
 * wav[b, :lengths[b]] alone - mean and variance over the clip's own samples, summed in the order qa_wav_normalize sums a [1, lengths[b]]
 * row - and out[b, lengths[b]:] is exactly 0; samples at or behind lengths[b] are never read.  out may alias wav. */
int qa_wav_normalize_ragged(const float* wav, int64_t B, int64_t T, const int64_t* lengths, float* out, float eps, void* stream);

/* ---- BiCodec.forward (QuarkAudio-UniSE/model/bicodec/bicodec.py:113-149, eval mode) ----------------------------------------------
 * Needs both handles: the tokenizer (qa_bicodec_enc, which owns the ECAPA latent the x-vector head pools) and the detokenizer
 * (qa_bicodec, which owns the prenet output the postnet reads).  The forward-only weights are optional: tokenize / detokenize never
 * read them.  x-vector head: ASTP attentive statistics pooling with global context
 * (speaker/pooling_layers.py:92-148, [frames; mean; std] 4608 -> 128 -> 1536), BatchNorm1d(3072),
 * Linear(3072 -> xvector_dim) (speaker/ecapa_tdnn.py:195-212).  postnet: feat_decoder.Decoder without condition (Linear, two ratio-1
 * SamplingBlocks each with a 2-layer VocosBackbone, a VocosBackbone with plain LayerNorm, Linear, optional tanh). */
typedef struct qa_bicodec_forward_spec {
    int32_t postnet_input_channels; /* 1024  = latent_dim (the prenet output) */
    int32_t postnet_vocos_dim;      /* 384 */
    int32_t postnet_vocos_inter;    /* 2048 */
    int32_t postnet_vocos_layers;   /* 6 */
    int32_t postnet_out_channels;   /* 1024  (the XLSR-53 feature width) */
    int32_t postnet_tanh;           /* 0     use_tanh_at_final */
    int32_t xvector_dim;            /* 1024  speaker_encoder.out_dim */
} qa_bicodec_forward_spec;
/* Attach the forward-only weights (host memory, the reference's keys speaker_encoder.speaker_encoder.{pool.linear1, pool.linear2, bn,
 * linear}.* and postnet.*).  The two handles must describe the same model (latent width, codebook, global tokens) on one device.  On
 * failure (the first missing or mis-shaped key in the error message) both handles keep what they had. */
int qa_bicodec_load_forward(qa_bicodec* dec, qa_bicodec_enc* enc, const qa_bicodec_forward_spec* spec, const qa_tensor* tensors,
                            int64_t n_tensors);
/* 1 if the forward-only weights are attached, 0 if not, negative on a null handle */
int qa_bicodec_has_forward(const qa_bicodec* dec, const qa_bicodec_enc* enc);
/* feat fp32 [B, N, input_channels], ref_wav fp32 [B, T_ref] (the whole rows: get_global_tokens with ref_len = 0).  Outputs (device):
 * semantic_out int64 [B, N], global_out int64 [B, token_num] (the tokens detokenize is run on), recons fp32 [B, N * hop]
 * (= qa_bicodec_detokenize of those tokens, bit for bit), pred_feat fp32 [B, postnet_out_channels, N] (channel-first), x_vector
 * fp32 [B, xvector_dim], d_vector fp32 [B, latent_dim], perplexity and cluster_size fp32 scalars: the code statistics over all B * N
 * semantic tokens (factorized_vector_quantize.py:98-103; active_num is cluster_size), summed in a fixed order. */
int qa_bicodec_forward(qa_bicodec* dec, qa_bicodec_enc* enc, const float* feat, int64_t B, int64_t N, const float* ref_wav, int64_t T_ref,
                       int64_t* semantic_out, int64_t* global_out, float* recons, float* pred_feat, float* x_vector, float* d_vector,
                       float* perplexity, float* cluster_size, void* stream);
/* Kernel-level entry point of forward's code statistics (tests): indices int64 [n] (device, 0 < n < 2^24, entries outside
 * [0, codebook_size) are not counted), codebook_size <= 16384 -> perplexity, cluster_size (device fp32 scalars). */
int qa_code_usage(const int64_t* indices, int64_t n, int32_t codebook_size, float* perplexity, float* cluster_size, void* stream);

/* ---- UniSE AR-LM ------------------------------------------------------------------------------------ */

typedef struct qa_lm_spec {
    int32_t hidden;        /* 512   QuarkAudio-UniSE/conf/config.yaml:131-146 */
    int32_t n_layers;      /* 12 */
    int32_t n_heads;       /* 8 */
    int32_t intermediate;  /* 2048 = 4*hidden (llm.py:69) */
    int32_t global_size;   /* 4096 */
    int32_t semantic_size; /* 8192 */
    int32_t feats_dim;     /* 768 */
    int32_t num_tasks;     /* 3 */
    float rope_theta;      /* 10000 */
    float rms_eps;         /* 1e-6 */
} qa_lm_spec;

typedef struct qa_lm qa_lm;

int qa_lm_create(qa_lm** out, const qa_lm_spec* spec, const qa_tensor* tensors, int64_t n_tensors, int device);
void qa_lm_destroy(qa_lm* lm);

/* LLM_SFT.generate with do_sample=False (the reference's test path, model/model.py:173): greedy decoding of
 * `global_length`+1 global tokens (last one discarded) then `semantic_length` semantic tokens.
 *   task        0 se, 1 tse, 2 rtse (config.yaml:132-136)
 *   enroll_feats [B, n_enroll, feats_dim] or NULL (SE prompt); mix_feats [B, n_mix, feats_dim]
 *   global_ids  int64 [B, global_length]; semantic_ids int64 [B, semantic_length]  (offsets already subtracted)
 * top_k / top_p / temperature are accepted for signature parity; with greedy decoding they cannot change the
 * argmax (llm.py:262-286) and are validated only (0 < temperature <= 1, llm.py:278). */
int qa_lm_generate(qa_lm* lm, int32_t task, const float* enroll_feats, int64_t n_enroll, const float* mix_feats,
                   int64_t n_mix, int64_t B, int32_t global_length, int32_t semantic_length, float temperature,
                   int32_t top_k, float top_p, int64_t* global_ids, int64_t* semantic_ids, void* stream);

/* LLM_SFT.generate with do_sample=True (the signature default, llm_sft.py:106): every step filters the logits of the active
 * vocabulary slice as CustomLlamaModel.sample_logits does (llm.py:253-288: top-k threshold with ties kept, nucleus filter on the
 * un-tempered logits that keeps the token crossing top_p, / temperature, softmax) and draws one token per sequence.  The
 * reference draws from torch's global generator; here the draw is a Philox4x32-10 uniform keyed by (seed, sequence, step), so the
 * same seed reproduces the same streams and the DISTRIBUTION equals the reference's (the streams cannot). */
int qa_lm_generate_sampled(qa_lm* lm, int32_t task, const float* enroll_feats, int64_t n_enroll, const float* mix_feats,
                           int64_t n_mix, int64_t B, int32_t global_length, int32_t semantic_length, float temperature,
                           int32_t top_k, float top_p, uint64_t seed, int64_t* global_ids, int64_t* semantic_ids, void* stream);

/* qa_lm_generate / qa_lm_generate_sampled over a batch whose enrollments differ in length (TSE / rTSE: the enrollment is a recording of
 * the user's choosing).  Row b behaves as LLM_SFT.generate would for that sequence ALONE with its first n_enroll[b] frames: prompt
 * [task, enroll_sos, adapter(enroll_feats[b, :n_enroll[b]]), mix_sos, adapter(mix_feats[b])] at positions 0 .. L_b - 1 with
 * L_b = 3 + n_enroll[b] + n_mix, decode step t at position L_b + t over L_b + t + 1 keys.  n_mix, global_length and semantic_length
 * are common to the batch.
 *   enroll_feats [B, n_enroll_max, feats_dim] (device), required; frames at or behind n_enroll[b] are padding and never enter a row's
 *                arithmetic (they may hold anything, NaN included)
 *   n_enroll     HOST int64 [B], each in 1 .. n_enroll_max; read during the call, may be freed on return
 * Refused, before anything is launched, when enroll_feats or n_enroll is NULL, when a length is out of range (the message names the row
 * and its value) or when 3 + n_enroll_max + n_mix + global_length + 1 + semantic_length exceeds 4096.  A vector whose entries all equal
 * n_enroll_max gives, bit for bit, the logits and tokens of qa_lm_generate(_sampled) with n_enroll = n_enroll_max.  Taps as there. */
int qa_lm_generate_ragged(qa_lm* lm, int32_t task, const float* enroll_feats, int64_t n_enroll_max, const int64_t* n_enroll,
                          const float* mix_feats, int64_t n_mix, int64_t B, int32_t global_length, int32_t semantic_length, float temperature,
                          int32_t top_k, float top_p, int64_t* global_ids, int64_t* semantic_ids, void* stream);
int qa_lm_generate_ragged_sampled(qa_lm* lm, int32_t task, const float* enroll_feats, int64_t n_enroll_max, const int64_t* n_enroll,
                                  const float* mix_feats, int64_t n_mix, int64_t B, int32_t global_length, int32_t semantic_length,
                                  float temperature, int32_t top_k, float top_p, uint64_t seed, int64_t* global_ids, int64_t* semantic_ids,
                                  void* stream);

/* qa_lm_generate / qa_lm_generate_sampled over a batch whose rows differ in any of their three lengths.  The layouts are
 * qa_lm_generate_ragged's with the maxima as strides: enroll_feats [B, n_enroll_max, feats_dim] or NULL, mix_feats [B, n_mix_max, feats_dim],
 * semantic_ids [B, semantic_length_max].  Three optional HOST int64 [B] vectors, read during the call only, NULL for "every row at full width":
 *   n_enroll[b]    1 .. n_enroll_max (only with an enrollment)
 *   n_mix[b]       1 .. n_mix_max
 *   n_semantic[b]  0 .. semantic_length_max (0: the row returns global ids only)
 * Row b behaves as qa_lm_generate(_sampled) for that sequence ALONE on enroll_feats[b, :n_enroll[b]] and mix_feats[b, :n_mix[b]] with
 * semantic_length = n_semantic[b]: prompt of L_b = 1 + (1 + n_enroll[b]) + 1 + n_mix[b] positions (2 + n_mix[b] without an enrollment), the
 * global phase from position L_b, then n_semantic[b] semantic steps.  global_length is common to the batch.
 *   semantic_ids[b, t] for t >= n_semantic[b] is exactly -1 (the value qa_bicodec_detokenize_ragged ignores); the tap logits.semantic[b, t, :]
 *   is exactly 0 there.  Frames at or behind a row's counts never enter any row's arithmetic (they may hold anything, NaN included).
 * A row that has taken its last step stops reading and writing its keys and values, and a chain of rows stops at its own longest row.
 * With every given vector at full width the call is qa_lm_generate(_sampled), with n_enroll alone qa_lm_generate_ragged(_sampled): the same
 * launches, the same bits.  Refused before anything is launched, the handle staying usable: a length out of range (the message names the row
 * and its value), n_enroll without enroll_feats, a NULL mix_feats or output, the longest possible row - prompt at the maxima + global_length
 * + 1 + semantic_length_max - beyond 4096 positions, and, with n_mix or n_semantic given, a stream that is being captured (the lengths are
 * host data). */
int qa_lm_generate_rows(qa_lm* lm, int32_t task, const float* enroll_feats, int64_t n_enroll_max, const int64_t* n_enroll,
                        const float* mix_feats, int64_t n_mix_max, const int64_t* n_mix, int64_t B, int32_t global_length,
                        int32_t semantic_length_max, const int64_t* n_semantic, float temperature, int32_t top_k, float top_p,
                        int64_t* global_ids, int64_t* semantic_ids, void* stream);
int qa_lm_generate_rows_sampled(qa_lm* lm, int32_t task, const float* enroll_feats, int64_t n_enroll_max, const int64_t* n_enroll,
                                const float* mix_feats, int64_t n_mix_max, const int64_t* n_mix, int64_t B, int32_t global_length,
                                int32_t semantic_length_max, const int64_t* n_semantic, float temperature, int32_t top_k, float top_p,
                                uint64_t seed, int64_t* global_ids, int64_t* semantic_ids, void* stream);

/* LLM_SFT.forward (llm_sft.py:37-90): teacher-forced scoring of given token streams.  With Lt = global_length + semantic_length + 2,
 * input_ids = [0, global_ids + 3, 1, semantic_ids + 3 + global_size] and target_ids = [global_ids + 3, 1, semantic_ids + 3 + global_size, 2];
 * the prompt is generate's, the body runs causally over all prompt + Lt positions from position 0, and output_head covers the FULL
 * vocabulary on the last Lt rows.  Loss: F.kl_div(log_softmax(z), true_dist, 'batchmean') with true_dist = 1 - label_smoothing at the
 * target and label_smoothing / (V - 1) elsewhere (llm.py:87-104, 0 log 0 = 0); accuracy: first arg-max == target.
 *   global_ids int64 [B, global_length], semantic_ids int64 [B, semantic_length] (device; offsets subtracted).  The shifted ids must
 *   lie in [0, V) - check them with qa_codes_check (the reference's nn.Embedding raises IndexError); the kernel clamps, it never reads
 *   outside the table.
 * Outputs (device): loss_per_seq float [B] (mean KL over the sequence's Lt rows), correct_per_seq int64 [B] (rows whose arg-max is
 * the target), loss / acc float scalars over all B * Lt rows.  Every reduction runs in a fixed order: a sequence's values do not depend
 * on its batch, and QA_LM_SCORE_ROWS (head rows per launch) changes no bit.  At most 4096 positions (max_position_embeddings).
 * Asynchronous on `stream`; uses a workspace of its own (generate's buffers and captured steps are untouched). */
int qa_lm_score(qa_lm* lm, int32_t task, const float* enroll_feats, int64_t n_enroll, const float* mix_feats, int64_t n_mix, int64_t B,
                const int64_t* global_ids, int32_t global_length, const int64_t* semantic_ids, int32_t semantic_length, double label_smoothing,
                float* loss_per_seq, int64_t* correct_per_seq, float* loss, float* acc, void* stream);

/* qa_lm_score for a batch whose rows differ in length.  Layouts are qa_lm_score's with the maxima as the strides:
 * enroll_feats [B, n_enroll_max, feats_dim], mix_feats [B, n_mix_max, feats_dim], semantic_ids [B, semantic_length_max]; global_length is
 * common to the batch.  Three optional HOST int64 vectors [B], read during the call only (they may be freed on return):
 *   n_enroll[b]   in 1 .. n_enroll_max (only with an enrollment)
 *   n_mix[b]      in 1 .. n_mix_max
 *   n_semantic[b] in 0 .. semantic_length_max
 * NULL means "every row at full width".  Row b is scored as qa_lm_score scores that sequence alone on enroll_feats[b, :n_enroll[b]],
 * mix_feats[b, :n_mix[b]] and semantic_ids[b, :n_semantic[b]]: a prompt of Lp_b = 1 + (1 + n_enroll[b]) + 1 + n_mix[b] positions
 * (2 + n_mix[b] without an enrollment), Lt_b = global_length + n_semantic[b] + 2 target rows with the eos target right behind the row's
 * own last semantic id, positions 0 .. Lp_b + Lt_b - 1.  Feature frames and ids at or behind a row's lengths never enter its
 * arithmetic and are not range-checked (check ids[b, :n_semantic[b]] with qa_codes_check).
 * Outputs: loss_per_seq[b] the mean KL over the row's own Lt_b rows, correct_per_seq[b] its correct rows; the scalars pool the rows:
 * loss = (sum over all target rows of kl) / sum_b Lt_b, acc = sum_b correct_b / sum_b Lt_b.  No atomics: a row's values do not depend on
 * its neighbours, its group of 64, the padded width, QA_LM_SCORE_ROWS or taps.  The tap "logits.forced" is then PACKED:
 * [sum_b Lt_b, V], sequences in order, each with its own Lt_b rows.
 * Every check runs before the first launch, names the row and its value, and leaves the handle usable: a length out of range, n_enroll
 * without enroll_feats, a row above 4096 positions, a NULL pointer where data is needed.  Refused under a stream capture whenever a
 * vector is given (a replayed graph would repeat the captured lengths).  With every given vector uniform at full width the call IS
 * qa_lm_score: the same launches, the same bits.  Sequences go through in groups of 64, each laid out at its own longest row; inside a
 * group the body still computes the padded layout (dead attention blocks exit at once), the head and the loss run on packed rows. */
int qa_lm_score_ragged(qa_lm* lm, int32_t task, const float* enroll_feats, int64_t n_enroll_max, const int64_t* n_enroll, const float* mix_feats,
                       int64_t n_mix_max, const int64_t* n_mix, int64_t B, const int64_t* global_ids, int32_t global_length,
                       const int64_t* semantic_ids, int32_t semantic_length_max, const int64_t* n_semantic, double label_smoothing,
                       float* loss_per_seq, int64_t* correct_per_seq, float* loss, float* acc, void* stream);

/* Test hook, as qa_hcodec_enable_taps: while on, qa_lm_generate / qa_lm_generate_sampled record the logits of the active vocabulary
 * slice at every decode step (what the head computes before the pick / sampler), in storage of their own: turning taps on changes no
 * token.  Not supported under a caller's stream capture (the call is refused). */
int qa_lm_enable_taps(qa_lm* lm, int on);
/* Test hook: copy a snapshot of the LAST generate call into `dst` (device, fp32, capacity `cap` elements; NULL: only return the
 * count).  Returns the element count or a negative status.  Names: "logits.global" [B, global_length + 1, global_size] (the
 * discarded last global step included), "logits.semantic" [B, semantic_length, semantic_size]; of the LAST qa_lm_score call:
 * "logits.forced" [B, Lt, V] (the full-vocabulary teacher-forced logits). */
int64_t qa_lm_tap(qa_lm* lm, const char* name, float* dst, int64_t cap, void* stream);

/* ---- sessions: the Llama body over a cache the CALLER holds (CustomLlamaModel.llm_forward, llm.py:150-227) --------------------------
 * A qa_lm_cache is device memory of its own - K and V as [layer][max_batch][max_len][hidden] fp32 plus the small buffers of the
 * one-position step - so qa_lm_generate / qa_lm_score calls between two session calls on the same handle disturb nothing, and the
 * reverse.  Several caches per handle are allowed; max_len <= 4096 (max_position_embeddings).  Its length and batch are HOST state:
 * every call below that reads or changes them is refused under a caller's stream capture (a replay would repeat the captured
 * positions).  One handle serves one stream at a time, as everywhere in this header.  qa_lm_destroy frees the caches the caller
 * left; their pointers are invalid afterwards. */
typedef struct qa_lm_cache qa_lm_cache;
int qa_lm_cache_create(qa_lm* lm, int64_t max_batch, int64_t max_len, qa_lm_cache** out);
void qa_lm_cache_destroy(qa_lm_cache* cache);
int64_t qa_lm_cache_length(const qa_lm_cache* cache); /* positions held (DynamicCache.get_seq_length) */
int64_t qa_lm_cache_batch(const qa_lm_cache* cache);  /* sequences held; 0 until the first forward call (and after a reset) */
int qa_lm_cache_reset(qa_lm_cache* cache);            /* length 0, batch free again */
/* DynamicCache.crop: keep the first `len` positions (0 <= len <= length).  Host state only: the rows behind are stale and invisible. */
int qa_lm_cache_crop(qa_lm_cache* cache, int64_t len);
/* Batch row j becomes old row idx[j] (idx: HOST int64 [n], 0 <= idx[j] < batch, n <= max_batch): DynamicCache.batch_select_indices,
 * reorder_cache and batch_repeat_interleave in one entry, e.g. one TSE prefix run at B = 1 and repeated for the S segments of a file.
 * Correct in place for any idx (permutations, repeats, growing and shrinking n); copies the first `length` positions of a row only.
 * Asynchronous on `stream`, no allocation. */
int qa_lm_cache_select(qa_lm_cache* cache, const int64_t* idx, int64_t n, void* stream);
/* inputs_embeds fp32 [B, n, hidden] (device) run at positions length .. length + n - 1, causal over length + n keys; then length += n.
 * last_hidden [B, n, hidden]: the final RMSNorm's output (last_hidden_state).  all_hidden: NULL, or [(n_layers + 1), B, n, hidden] =
 * the input of every layer, then last_hidden (output_hidden_states, llm.py:192-220).  cache NULL is use_cache = False: positions
 * 0 .. n - 1, nothing kept.  The first call on a cache fixes its batch B.  B above max_batch or length + n above max_len is an error
 * that names the limit and leaves the cache as it was.
 * n >= 2 runs the prefill kernels (implicit GEMM, flash attention with a query offset): a sequence's rows do not depend on the batch
 * it sits in.  n = 1 runs the fused decode-step launches of qa_lm_generate on the caller's rows (more than 64 sequences: in groups of
 * 64); there too a row does not depend on its batch.  The two paths sum in different orders, so one position fed as n = 1 and the
 * same position inside a longer chunk agree to fp32 rounding, not bit for bit.
 * Asynchronous on `stream`.  n = 1 with a cache allocates nothing; other shapes use a session workspace of the handle that grows to
 * the largest B * n seen (growing waits for the device). */
int qa_lm_forward(qa_lm* lm, qa_lm_cache* cache, const float* inputs_embeds, int64_t B, int64_t n, float* last_hidden, float* all_hidden,
                  void* stream);
/* Per-row lengths (ragged sessions).  Every row of a cache has a length of its own; the calls above see a cache whose rows are all
 * equally long exactly as before.  On a cache with unequal rows: qa_lm_cache_length is the LONGEST row; qa_lm_cache_crop(len) needs
 * len <= the longest row and sets every row to min(its length, len); qa_lm_cache_select gives row j the contents AND the length of old
 * row idx[j] (each move copies that row's own length); qa_lm_cache_reset clears every length; qa_lm_forward(n) feeds n positions to every
 * row at the row's own position (the ragged call below with n[b] = n), so a greedy loop after a ragged prefill keeps calling it with
 * n = 1.
 *
 * qa_lm_forward_ragged: inputs_embeds and last_hidden [B, n_max, hidden], all_hidden NULL or [(n_layers + 1), B, n_max, hidden]; n is
 * a HOST int64 [B] with 0 <= n[b] <= n_max, read during the call only (the lengths reach the device as kernel arguments, into an array
 * the cache owns).  Row b's first n[b] positions run at positions len[b] .. len[b] + n[b] - 1, causal over the row's own len[b] + n[b]
 * keys; then len[b] += n[b].  The row's result is what qa_lm_forward gives that sequence alone, bit for bit.  Input entries t >= n[b]
 * are never read; the same entries of last_hidden and all_hidden are written as exactly 0.  n[b] = 0 is an idle row: it does not
 * advance and no K / V position is written for it.  No row writes a K / V position at or behind its new length, so a row may end at
 * max_len with n[b] < n_max, and an idle row may already stand at max_len.  A call whose n is all zeros succeeds and launches nothing.
 * `cache` is required.  Every check (NULL n, n[b] outside 0 .. n_max, len[b] + n[b] > max_len, B against max_batch and the fixed
 * batch) runs before the first launch, names the row and its value, and leaves the cache as it was.  Refused under a stream capture.
 * The path follows n_max alone: n_max >= 2 the chunk kernels, n_max = 1 the fused step in groups of 64.  With every row at one length
 * and every n[b] = n_max the call IS qa_lm_forward: the same launches, the same bits.
 * qa_lm_cache_lengths: out HOST int64 [batch] <- the rows' lengths.
 * qa_lm_cache_crop_rows: lens HOST int64 [batch], 0 <= lens[b] <= length of row b; host state only, like qa_lm_cache_crop.  A row
 * joins a running batch as: select (grow by one row), crop_rows (the new row to 0), forward_ragged with n = [0, .., 0, L]. */
int qa_lm_forward_ragged(qa_lm* lm, qa_lm_cache* cache, const float* inputs_embeds, int64_t B, int64_t n_max, const int64_t* n,
                         float* last_hidden, float* all_hidden, void* stream);
int qa_lm_cache_lengths(const qa_lm_cache* cache, int64_t* out);
int qa_lm_cache_crop_rows(qa_lm_cache* cache, const int64_t* lens);
/* The submodules of LLM_SFT as device calls, so that a caller's decode loop never leaves the library.
 * qa_lm_embed: out [n, hidden] = codec_embedding[ids[i]] (ids device int64, raw vocabulary ids).  The kernel clamps for memory safety;
 *   check the ids with qa_codes_check first (the reference's nn.Embedding raises IndexError).
 * qa_lm_head: logits [rows, width] = hidden [rows, hidden] x output_head[lo .. lo + width - 1]^T; `hidden` is last_hidden (norm applied).
 * qa_lm_prompt: out [B, L, hidden] = [task, (enroll_sos, adapter(enroll_feats)), mix_sos, adapter(mix_feats)] (llm_sft.py:110-128),
 *   L = 1 + (enroll_feats ? 1 + n_enroll : 0) + 1 + n_mix; arguments as qa_lm_generate. */
int qa_lm_embed(qa_lm* lm, const int64_t* ids, int64_t n, float* out, void* stream);
int qa_lm_head(qa_lm* lm, const float* hidden, int64_t rows, int32_t lo, int32_t width, float* logits, void* stream);
int qa_lm_prompt(qa_lm* lm, int32_t task, const float* enroll_feats, int64_t n_enroll, const float* mix_feats, int64_t n_mix, int64_t B,
                 float* out, void* stream);
/* qa_lm_prompt with per-row lengths (n_enroll / n_mix: HOST int64 [B] as in qa_lm_score_ragged, NULL = full width): out
 * [B, Lp_max, hidden] with Lp_max = 1 + (enroll_feats ? 1 + n_enroll_max : 0) + 1 + n_mix_max; row b is left-aligned over its own
 * Lp_b = 1 + (1 + n_enroll[b]) + 1 + n_mix[b] positions (2 + n_mix[b] without an enrollment) - what qa_lm_prompt gives the row alone on
 * its trimmed features, bit for bit - with exact zeros behind.  Padding frames are never copied.  The result feeds
 * qa_lm_forward_ragged with n[b] = Lp_b.  Checks and the stream-capture refusal as in qa_lm_score_ragged; uniform vectors at full width
 * are qa_lm_prompt. */
int qa_lm_prompt_ragged(qa_lm* lm, int32_t task, const float* enroll_feats, int64_t n_enroll_max, const int64_t* n_enroll, const float* mix_feats,
                        int64_t n_mix_max, const int64_t* n_mix, int64_t B, float* out, void* stream);

/* Kernel-level entry point of the sampler (parity / distribution tests): CustomLlamaModel.sample_logits (llm.py:253-288) on
 * logits [B, width] (row stride ld, device).  out_index int64 [B] (device).  do_sample = 0: arg-max (first maximum).
 * Synchronises `stream`. */
int qa_sample_logits(const float* logits, int64_t B, int64_t width, int64_t ld, int32_t top_k, float top_p, float temperature,
                     int32_t do_sample, uint64_t seed, int64_t* out_index, void* stream);

/* ---- UniSE condition encoder and the pre-training-stage entry points of the LM --------------------------------------------------
 * CustomLlamaModel's condition path (QuarkAudio-UniSE/model/llm/llm.py:52-54,130-132,304-306): cond_input_layer (Linear cond_dim -> dim),
 * cond_encoder (ConformerEncoder, model/llm/conformer.py:384-484) and cond_output_layer (Linear dim -> hidden_out), eval mode, fp32.
 * One ConformerLayer: x = 0.5 FF1(x) + x; x = Attn(LN(x)) + x; x = Conv(x) + x; x = 0.5 FF2(x) + x; x = LN(x), with FF = LN -> Linear ->
 * SiLU -> Linear, Attn = biased q / k / v / out projections around softmax(Q K^T / sqrt(dim_head)) V with rotary embedding on the first
 * pe_attn_head heads, Conv = LN -> 1x1 (d -> 2d) -> GLU -> depthwise k "same" -> BatchNorm1d (running statistics) -> SiLU -> 1x1.
 * Weights: the reference's keys `cond_input_layer.*`, `cond_encoder.layers.N.*`, `cond_output_layer.*`; with cond_dim = hidden_out = 0 the
 * handle is a bare ConformerEncoder and the keys are `layers.N.*`.  A missing key, or a key under those prefixes the model does not
 * have, fails the create (num_batches_tracked and rotary_embedding.inv_freq are accepted and ignored). */
typedef struct qa_cond_encoder_spec {
    int32_t cond_dim;         /* 80    log-mel bins; 0 = bare ConformerEncoder */
    int32_t dim;              /* 512   conf/config.yaml:148-157 */
    int32_t n_layers;         /* 6 */
    int32_t heads;            /* 8 */
    int32_t dim_head;         /* 64 */
    int32_t dw_kernel;        /* 31    odd, <= 31 */
    int32_t ff_mult;          /* 4 */
    int32_t pe_attn_head;     /* 1     heads 0 .. p-1 of q and k are rotated; -1 = all (None) */
    int32_t rope_interleaved; /* 1     1: adjacent channel pairs (2i, 2i+1); 0: rotate-half pairs (i, i + dim_head/2) */
    int32_t hidden_out;       /* 512   the LM's hidden size; 0 = bare ConformerEncoder */
    int32_t qk_norm;          /* 0     1 ("rms_norm") is refused: not in the shipped configuration */
} qa_cond_encoder_spec;
typedef struct qa_cond_encoder qa_cond_encoder;
int qa_cond_encoder_create(qa_cond_encoder** out, const qa_cond_encoder_spec* spec, const qa_tensor* tensors, int64_t n_tensors, int device);
void qa_cond_encoder_destroy(qa_cond_encoder* h);
/* mel fp32 [B, T, cond_dim] -> out fp32 [B, T, hidden_out] (device).  mask: NULL or bytes [B, T] on the device, non-zero = valid
 * (ConformerEncoder.forward(x, mask), conformer.py:165-187): masked keys are invisible to every query and the attention module's output
 * rows of masked positions are zero before the residual; nothing else reads the mask.  A batch item without a valid position is an
 * error (a masked call copies B counters to the host and waits for them; an unmasked call is asynchronous on `stream`). */
int qa_cond_encoder_forward(qa_cond_encoder* h, const float* mel, const uint8_t* mask, int64_t B, int64_t T, float* out, void* stream);
/* the bare ConformerEncoder: x fp32 [B, T, dim] -> out [B, T, dim] (out may alias x) */
int qa_conformer_forward(qa_cond_encoder* h, const float* x, const uint8_t* mask, int64_t B, int64_t T, float* out, void* stream);
/* The two calls above over a batch whose items differ in length.  lengths: HOST int64 [B], each in 1 .. T frames, read during the call
 * (it may be freed on return).  Item b comes out as the call without a mask would give it ALONE at T = lengths[b]: keys at or behind
 * lengths[b] are invisible, the convolution module's "same" zero padding starts at lengths[b] (the mask above never reaches that module),
 * and out[b, lengths[b]:] is exactly 0.  What x / mel hold at or behind an item's length is never used (NaN included).  The vector is
 * checked on the host before anything is launched - the message names the row and its value - so the call does not wait for the device;
 * it is refused under a stream capture.  lengths NULL, or every entry equal to T: the call without a mask, same launches, same bits.
 * Taps keep their shapes; rows behind an item's length are unspecified except in conformer.N.attn, where they are zero. */
int qa_cond_encoder_forward_ragged(qa_cond_encoder* h, const float* mel, const int64_t* lengths, int64_t B, int64_t T, float* out,
                                   void* stream);
int qa_conformer_forward_ragged(qa_cond_encoder* h, const float* x, const int64_t* lengths, int64_t B, int64_t T, float* out, void* stream);
/* test hooks, as qa_hcodec_enable_taps / qa_hcodec_tap: conformer.N.ff1 (x after the first half-step), conformer.N.attn (the attention
 * module's output, masked rows zero, before the residual), conformer.N.conv (x after the convolution module), conformer.N.out; [B, T, dim] */
int qa_cond_encoder_enable_taps(qa_cond_encoder* h, int on);
int64_t qa_cond_encoder_tap(qa_cond_encoder* h, const char* name, float* dst, int64_t cap, void* stream);

/* Model.stft_logmel (QuarkAudio-UniSE/model/model.py:53-79): wav fp32 [B, n] is zero-padded by (win - hop) / 2 in front and to a multiple
 * of the hop plus (win - hop) / 2 behind, STFT (periodic Hann, center = False), magnitude, HTK mel filter bank f_min .. f_max without
 * normalisation, log(mel + 1e-10) -> out fp32 [B, qa_logmel_frames(n, hop), n_mels].  Needs win_length = 2 * hop_length, hop a multiple
 * of 16 and n_fft >= win_length; other configurations are refused.  The function has no handle: the DFT basis, the filter bank and a
 * workspace of each (device, parameter set) are built on first use and kept for the life of the process (1.7 MB + workspace for the
 * UniSE configuration), and calls with the same parameters are serialised on the host while they queue their work. */
int64_t qa_logmel_frames(int64_t n, int32_t hop_length);
int qa_logmel(const float* wav, int64_t B, int64_t n, int32_t n_fft, int32_t win_length, int32_t hop_length, int32_t n_mels, int32_t sample_rate,
              float f_min, float f_max, float* out, void* stream);
/* qa_logmel over clips of different lengths.  lengths: HOST int64 [B], each in 1 .. n samples, read during the call.  With
 * F_b = qa_logmel_frames(lengths[b], hop): out[b, :F_b] is qa_logmel of wav[b, :lengths[b]] alone, out[b, F_b:] is exactly 0, and the
 * samples at or behind lengths[b] are never used.  Checked before anything is launched (the message names the row and its value), refused
 * under a stream capture.  lengths NULL, or every entry equal to n: qa_logmel, same launches, same bits. */
int qa_logmel_ragged(const float* wav, const int64_t* lengths, int64_t B, int64_t n, int32_t n_fft, int32_t win_length, int32_t hop_length,
                     int32_t n_mels, int32_t sample_rate, float f_min, float f_max, float* out, void* stream);

/* CustomLlamaModel.generate (llm.py:291-374) on a qa_lm handle: prompt [mix_sos, cond_embeds] (cond_embeds fp32 [B, T, hidden] on the
 * device, the condition encoder's output) or NO prompt (cond_embeds NULL and T = 0: the first step runs at position 0 over an empty
 * cache).  Exactly `global_length` global steps, then semantic_sos and `semantic_length` semantic steps.  Other arguments as
 * qa_lm_generate / qa_lm_generate_sampled.  Taps: "logits.global" is [B, global_length, global_size] after these calls. */
int qa_lm_generate_cond(qa_lm* lm, const float* cond_embeds, int64_t T, int64_t B, int32_t global_length, int32_t semantic_length,
                        float temperature, int32_t top_k, float top_p, int64_t* global_ids, int64_t* semantic_ids, void* stream);
int qa_lm_generate_cond_sampled(qa_lm* lm, const float* cond_embeds, int64_t T, int64_t B, int32_t global_length, int32_t semantic_length,
                                float temperature, int32_t top_k, float top_p, uint64_t seed, int64_t* global_ids, int64_t* semantic_ids,
                                void* stream);
/* The two calls above over a batch whose conditions differ in length, by the mechanism of qa_lm_generate_ragged.  cond_embeds is
 * [B, T_max, hidden]; n_cond: HOST int64 [B], each in 1 .. T_max, read during the call.  Row b behaves as qa_lm_generate_cond would for it
 * ALONE with cond_embeds[b, :n_cond[b]]: prompt [mix_sos, cond] at positions 0 .. n_cond[b], decode step t at position 1 + n_cond[b] + t.
 * Frames at or behind n_cond[b] are never used (NaN included).  global_length and semantic_length are common to the batch.  Refused,
 * before anything is launched: a vector with cond_embeds NULL or T_max = 0; a length out of range (the message names the row and its
 * value); 1 + T_max + global_length + 1 + semantic_length above 4096; a stream capture.  n_cond NULL, or every entry equal to T_max:
 * qa_lm_generate_cond(_sampled), same launches, same bits.  Taps as there. */
int qa_lm_generate_cond_ragged(qa_lm* lm, const float* cond_embeds, int64_t T_max, const int64_t* n_cond, int64_t B, int32_t global_length,
                               int32_t semantic_length, float temperature, int32_t top_k, float top_p, int64_t* global_ids,
                               int64_t* semantic_ids, void* stream);
int qa_lm_generate_cond_ragged_sampled(qa_lm* lm, const float* cond_embeds, int64_t T_max, const int64_t* n_cond, int64_t B,
                                       int32_t global_length, int32_t semantic_length, float temperature, int32_t top_k, float top_p,
                                       uint64_t seed, int64_t* global_ids, int64_t* semantic_ids, void* stream);
/* CustomLlamaModel.forward (llm.py:107-147): as qa_lm_score with the prompt above, and with the LAST input / target position dropped
 * (llm.py:126-127): Lt = global_length + semantic_length + 1, no semantic_eos target.  "logits.forced" is [B, Lt, V]. */
int qa_lm_score_cond(qa_lm* lm, const float* cond_embeds, int64_t T, int64_t B, const int64_t* global_ids, int32_t global_length,
                     const int64_t* semantic_ids, int32_t semantic_length, double label_smoothing, float* loss_per_seq,
                     int64_t* correct_per_seq, float* loss, float* acc, void* stream);
/* qa_lm_score_cond over rows that differ in their condition frames, their semantic ids, or both, by the plan and the kernels of
 * qa_lm_score_ragged.  n_cond: HOST int64 [B], each in 1 .. T_max; n_semantic: HOST int64 [B], each in 0 .. semantic_length_max; either may
 * be NULL (every row at full width); both are read during the call.  Row b is scored as qa_lm_score_cond scores it ALONE with
 * cond_embeds[b, :n_cond[b]] and semantic_ids[b, :n_semantic[b]]: Lp_b = 1 + n_cond[b] prompt positions and
 * Lt_b = global_length + n_semantic[b] + 1 target rows - the last position of ITS OWN stream is dropped, there is no eos target.  Frames
 * and ids at or behind a row's counts are never used.  loss_per_seq[b] is the mean over the row's Lt_b targets; loss and acc pool all
 * sum Lt_b target rows; "logits.forced" is packed [sum Lt_b, V], rows in order.  Refused, before anything is launched: n_cond with
 * cond_embeds NULL or T_max = 0, a count out of range (the message names the row and its value), a row of more than 4096 positions, a
 * stream capture.  Both vectors NULL or at full width: qa_lm_score_cond, same launches, same bits. */
int qa_lm_score_cond_ragged(qa_lm* lm, const float* cond_embeds, int64_t T_max, const int64_t* n_cond, int64_t B, const int64_t* global_ids,
                            int32_t global_length, const int64_t* semantic_ids, int32_t semantic_length_max, const int64_t* n_semantic,
                            double label_smoothing, float* loss_per_seq, int64_t* correct_per_seq, float* loss, float* acc, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* QUARKAUDIO_H_ */
