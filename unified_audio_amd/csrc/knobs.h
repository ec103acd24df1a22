// knobs.h - every tuning / A-B switch of libquarkaudio_hip in ONE table (INTEGRATION.md lists the same rows).
//
// A knob is an integer.  Its initial value comes from the environment variable of the same name (read once, at the first
// use of any knob); qa_set_knob() changes it at run time, so tests and A/B sessions flip a switch inside one process
// instead of re-spawning with another environment.  Kernels never read knobs: only the host-side launch code does, at
// launch (or handle-creation) time.
#pragma once
#include <cstdint>

namespace qa {

#define QA_KNOB_TABLE(X)                                                                                                           \
    X(SERIAL, "QA_SERIAL", 0, "1: no internal stream concurrency (every kernel alone on the device; = qa_set_serial)")           \
    X(GEMM_CFG, "QA_GEMM_CFG", -1, "force the conv_gemm tile: 0 = 128x32, 1 = 128x64, 2 = 128x128, 3 = 64x128, 4 = 64x64, 5 = 256x128 (LINEAR layers; else 128x128) (-1: cost model)")             \
    X(GEMM_256, "QA_GEMM_256", 0, "r06 experiment: 256x128 block tile (4 waves, 4x2 accumulators each) for LINEAR layers with M >= 8000 and N >= 1024; value = its efficiency relative to 128x128 in 1/1000 for the cost model (0: never chosen; QA_GEMM_CFG=5 forces it)") \
    X(GEMM_BK16, "QA_GEMM_BK16", 1 << 30, "largest K that takes the BK = 16 K-chunk variant (fp32 chain: 16-wide chunks; split forms: one LDS buffer of 32 k instead of two)")                                     \
    X(GEMM_BK16_MIN_TILES, "QA_GEMM_BK16_MIN_TILES", 384, "fewest tiles of a launch that take BK = 16")                          \
    X(GEMM_MATH, "QA_GEMM_MATH", 1, "conv_gemm arithmetic: 1 = split-6 (operands split into three bf16 planes, six v_mfma_f32_16x16x32_bf16 per 32-wide k group, fp32 accumulation), 0 = the fp32 chain (v_mfma_f32_32x32x2_f32); opt-in reduced precision: 2 = split-3 (two planes, products hm, mh, hh: operands exact to 2^-16), 3 = bf16 (one plane, one product: bf16 operands, fp32 accumulation); any other value = split-6; launches marked math_fp32 (the UniSE LM) keep the fp32 chain") \
    X(GEMM_PRESPLIT, "QA_GEMM_PRESPLIT", 1, "split-6 weights from a pre-split image: a weight store builds the three bf16 planes of all its weights once, at load (6 bytes per weight beside the fp32 blob; not built when 0 at load time), and conv_gemm's 128-column tiles copy them into LDS instead of splitting the weight tile in the K loop (narrower tiles keep the in-loop split); 0 at launch = ignore the image and split in the loop; same bits either way") \
    X(GEMM_LINEAR, "QA_GEMM_LINEAR", 1, "table-free K loop for ksize-1 layers")                                                  \
    X(GEMM_XCD, "QA_GEMM_XCD", 1, "XCD-aware tile order")                                                                        \
    X(GEMM_PANEL, "QA_GEMM_PANEL", 8, "conv_gemm tile order: column panels of this many tiles, row tiles fastest inside a panel (0: column tiles fastest over the whole row; 8: +4 % on N >= 4096 shapes, +1.2 % on H-Codec 2.0)") \
    X(ATT_MATH, "QA_ATT_MATH", 1, "attention arithmetic: 1 = split-6 (Q, K, V and the probabilities as three bf16 planes, six v_mfma_f32_32x32x16_bf16 per 16-wide k group, fp32 accumulation), 0 = the fp32 chain (v_mfma_f32_32x32x2_f32); the UniSE LM keeps the fp32 chain either way") \
    X(ATT_DEBUG, "QA_ATT_DEBUG", 0, "attention_kernel debug bits, both forms: 1 always rescale, 2 extra barrier per tile, 4 wait for the prefetch at once, 8 no wave-uniform tile skip, 16 mask every tile; the split-6 form (SPLIT) only (tests): 32 / 64 / 128 zero the h / m / l plane of the operands selected by 256 Q, 512 K, 1024 V, 2048 P (none of the four: all)") \
    X(AGG_LAST_ROWS, "QA_AGG_LAST_ROWS", 1, "H-Codec 1.5 encode: the last layer of each aggregator stack runs attention, out_proj, LayerNorm 2, lin1 and lin2 on the G query rows per clip only (the rows the read-out keeps); 0 = the full last layer; same bits either way") \
    X(BATCH_SPLIT, "QA_BATCH_SPLIT", 1, "H-Codec: a one-stream phase as two half-batch lanes on two streams - clips [0, ceil(B / 2)) on the caller's stream, the rest on an internal one, enqueued layer by layer and joined before the next recurrence (bit mask): 1 = the H-Codec 1.5 bottleneck transformer (32 x 10 s: 97.5 -> 96.1 ms per step); 0 = one lane; one lane as well for B = 1, under QA_SERIAL and with taps on; same bits either way") \
    X(BATCH_SPLIT_MIN_ROWS, "QA_BATCH_SPLIT_MIN_ROWS", 500, "QA_BATCH_SPLIT: fewest rows (clips x frames) of the smaller lane at which a region is split (10 s clips: lanes of 250 rows lose 0.5 ms, 500 rows gain 0.3 ms; tests: 0)") \
    X(SEANET_FUSED, "QA_SEANET_FUSED", 1, "fused conv0 + first SEANet residual block")                                           \
    X(MIMI_ROPE_WINDOW, "QA_MIMI_ROPE_WINDOW", 8192, "mimi streaming: positions covered by the RoPE table before the rolling window takes over (tests shrink it)") \
    X(TR_SHORT_ATTN, "QA_TR_SHORT_ATTN", 1, "codec Transformer streaming step of 1 .. 16 frames: 1 = the split-key short-chunk attention (stream_attn.hip: fixed key ranges per workgroup, fp32, partial records merged by a second launch) while batch x frames <= 256, attention_kernel above (where it is the faster one); 2 = the short-chunk kernel for every step of <= 16 frames; 0 = attention_kernel, which steps of more than 16 frames always take") \
    X(LSTM_GRAPH, "QA_LSTM_GRAPH", 1, "replay the T step launches of an LSTM call from a cached hipGraph")                       \
    X(LSTM_PERSISTENT, "QA_LSTM_PERSISTENT", -1, "persistent recurrence kernel: -1 auto (d >= 1536), 0 off, 1 on for every supported width") \
    X(LSTM_XCD, "QA_LSTM_XCD", 1, "XCD-local LSTM recurrence for d = 512 / 768 (lstm_team_kernel with one team per XCD: one launch, W_hh in the registers of every XCD's 32 CUs, sequences dealt to the XCDs, 32-member step barrier per XCD): 0 off (the per-step kernels), 1 agent-scope hand-off forms, 2 XCD-local forms (h stores that stay in the XCD's L2; H-Codec 1.0: 42.7 against 43.3 ms)") \
    X(LSTM_TEAM, "QA_LSTM_TEAM", 1, "team recurrence for d = 1024 (lstm_team_kernel, one launch: 4 teams of 64 workgroups, W_hh resident in registers, 8 sequences per team, agent-scope hand-offs; H-Codec 1.5 decoder: 134.1 -> 128.3 ms per step, profiles/r04_lstm_team_ab.txt): 0 = the per-step kernels") \
    X(LSTM_SPIN_LIMIT, "QA_LSTM_SPIN_LIMIT", 1 << 21, "persistent recurrence: polls of a barrier word before the barrier is declared broken") \
    X(LSTM_FAULT, "QA_LSTM_FAULT", 0, "1 (tests): the step barrier of every in-launch recurrence (lstm_persistent_kernel, lstm_team_kernel) waits for one workgroup more than exists, like a starved launch") \
    X(LM_GRAPH, "QA_LM_GRAPH", 0, "1: replay one captured decode step per token")                                                \
    X(LM_MLP_FUSED, "QA_LM_MLP_FUSED", 1, "decode step: gate/up + SwiGLU + down of 16 activation columns per workgroup in one launch emitting K-slice partials, summed by a reduce launch (0: separate gate/up and down launches)") \
    X(LM_PF, "QA_LM_PF", 7, "decode step: cross-launch L2 weight prefetch planes (bit mask; lm_decode.h PfArgs): 1 qkv launch -> o_proj weights, 2 o_proj launch -> fused-MLP weights, 4 MLP launch -> next layer's qkv weights (last layer: the head slice), 8 head launch -> layer 0 qkv weights") \
    X(LM_ROWSPLIT, "QA_LM_ROWSPLIT", 3, "decode step at 9 .. 16 sequences: two 8-row groups instead of one 16-row group in the qkv launch (bit 1) and the fused-MLP launch (bit 2)") \
    X(LM_CHAINS, "QA_LM_CHAINS", 0, "generate: number of concurrent chains on internal streams (0: ceil(B / 64) - one chain serves up to 64 sequences, two row groups of 32 per launch; a count that would put more than 64 sequences into a chain is raised)") \
    X(LM_SCORE_ROWS, "QA_LM_SCORE_ROWS", 4096, "qa_lm_score: target rows per output_head launch (the logits buffer holds this many rows of the full vocabulary; any value gives the same bits)")

enum Knob {
#define QA_KNOB_ENUM(id, name, def, doc) K_##id,
    QA_KNOB_TABLE(QA_KNOB_ENUM)
#undef QA_KNOB_ENUM
        K_COUNT
};

long long knob(Knob k);
void knob_set(Knob k, long long v);

}  // namespace qa
