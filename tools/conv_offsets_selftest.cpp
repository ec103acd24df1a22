// conv_offsets_selftest.cpp - the host check behind the 32-bit entries of conv_gemm's source-frame table (csrc/conv_offsets.h, DESIGN.md
// section 41) as a stand-alone host program for the host sanitizers: the limit itself, one below and one above it, T_out = 1, T_out > BM,
// operands whose product leaves int64 (signed overflow is a report under -fsanitize=undefined), and the bound against a brute-force walk
// over every tile position of small grids.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer \
//       -I unified_audio_amd/csrc tools/conv_offsets_selftest.cpp -o /tmp/conv_offsets_selftest && /tmp/conv_offsets_selftest
#include <cstdio>
#include <initializer_list>

#include "conv_offsets.h"

#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            return 1;                                                    \
        }                                                                \
    } while (0)

using qa::conv_tile_offset_span;
using qa::conv_tile_offsets_fit;

// the largest entry build_taps can write for a tile at m0: last clip the tile touches, last frame of it, + 1
static int64_t walked_span(int64_t bm, int64_t t_out, int64_t t_in, int64_t ldx, int64_t m0, int64_t M) {
    const int64_t last = (m0 + bm - 1 < M - 1 ? m0 + bm - 1 : M - 1) / t_out - m0 / t_out;
    return last * t_in * ldx + t_in * ldx;
}

int main() {
    const int64_t LIM = qa::CONV_OFFSET_LIMIT;
    CHECK(LIM == INT64_C(2147483648));
    int64_t span = -1;
    // clips: ceil(bm / t_out) + 1
    CHECK(conv_tile_offset_span(128, 30, 1, 1) == 6);    // 5 + 1
    CHECK(conv_tile_offset_span(128, 128, 1, 1) == 2);   // a tile that starts inside a clip ends in the next
    CHECK(conv_tile_offset_span(128, 129, 1, 1) == 2);   // T_out > BM
    CHECK(conv_tile_offset_span(64, 1000000, 7, 3) == 2 * 21);
    CHECK(conv_tile_offset_span(128, 1, 1, 1) == 129);   // T_out = 1: every row its own clip
    CHECK(conv_tile_offset_span(64, 1, 5, 4) == 65 * 20);
    CHECK(conv_tile_offset_span(256, 17, 2, 8) == 17 * 16);  // ceil(256 / 17) = 16
    // the limit itself, one below, one above: T_out > BM, two clips of T_in * ldx floats
    CHECK(conv_tile_offsets_fit(128, 1000, 1 << 15, (1 << 15) - 1, &span) && span == LIM - (1 << 16));
    CHECK(!conv_tile_offsets_fit(128, 1000, 1 << 15, 1 << 15, &span) && span == LIM);  // exactly 2^31: refused
    CHECK(conv_tile_offsets_fit(128, 1000, (LIM - 2) / 2, 1, &span) && span == LIM - 2);
    CHECK(!conv_tile_offsets_fit(128, 1000, LIM / 2, 1, &span) && span == LIM);
    CHECK(!conv_tile_offsets_fit(128, 1000, LIM / 2 + 1, 1, &span) && span == LIM + 2);
    // 2^31 - 1 exactly: 129 clips (T_out = 1, BM = 128) do not divide it, 3 x 715827882 + 1 does not either; use BM = 6, T_out = 1: 7 clips,
    // 2^31 - 1 = 7 x 306783378 + 1 - so one below the limit is reached with ldx as the free factor
    CHECK(conv_tile_offsets_fit(6, 1, 306783378, 1, &span) && span == LIM - 2);
    CHECK(!conv_tile_offsets_fit(6, 1, 306783379, 1, &span) && span == LIM + 5);
    CHECK(conv_tile_offsets_fit(1, 1, 1, (LIM - 1) / 2, &span) && span == LIM - 2);  // 2 clips of 1073741823
    CHECK(conv_tile_offsets_fit(1, 2, 1, LIM / 2 - 1, &span) && span == LIM - 2);
    CHECK(!conv_tile_offsets_fit(1, 2, 1, LIM / 2, &span) && span == LIM);
    // T_out = 1 at the three tile heights
    for (const int64_t bm : {64, 128, 256}) {
        const int64_t clips = bm + 1, clip = (LIM - 1) / clips;  // the largest clip that fits
        CHECK(conv_tile_offsets_fit(bm, 1, clip, 1, &span) && span == clips * clip && span < LIM);
        CHECK(conv_tile_offsets_fit(bm, 1, 1, clip, &span) && span == clips * clip);
        CHECK(!conv_tile_offsets_fit(bm, 1, clip + 1, 1, &span) && span == clips * (clip + 1) && span >= LIM);
    }
    // T_out > BM, by one and by far, up to the end of int64 (no bm + t_out inside)
    for (const int64_t t_out : {INT64_C(129), INT64_C(1) << 31, INT64_MAX}) {
        CHECK(conv_tile_offset_span(128, t_out, 10, 4) == 80);
        CHECK(conv_tile_offsets_fit(128, t_out, (LIM - 4) / 4 / 2, 4, &span) && span == LIM - 8);
        CHECK(!conv_tile_offsets_fit(128, t_out, LIM / 4 / 2, 4, &span) && span == LIM);
    }
    // products that leave int64 saturate instead of overflowing
    CHECK(conv_tile_offset_span(128, 1, INT64_MAX, 1) == INT64_MAX);
    CHECK(conv_tile_offset_span(128, 1, INT64_MAX, INT64_MAX) == INT64_MAX);
    CHECK(conv_tile_offset_span(128, 1000, INT64_C(1) << 32, INT64_C(1) << 31) == INT64_MAX);  // 2^63
    CHECK(conv_tile_offset_span(128, 1000, INT64_C(1) << 31, INT64_C(1) << 31) == INT64_MAX);  // 2 x 2^62
    CHECK(conv_tile_offset_span(128, 1000, INT64_C(1) << 31, (INT64_C(1) << 30)) == INT64_C(1) << 62);
    CHECK(!conv_tile_offsets_fit(128, 1, INT64_MAX, INT64_MAX, nullptr));  // a null span is allowed
    // an empty grid or clip has no entry at all
    CHECK(conv_tile_offset_span(128, 0, 5, 5) == 0 && conv_tile_offset_span(128, 5, 0, 5) == 0 && conv_tile_offset_span(128, 5, 5, 0) == 0);
    CHECK(conv_tile_offset_span(0, 5, 5, 5) == 0 && conv_tile_offset_span(128, -3, 5, 5) == 0);
    CHECK(conv_tile_offsets_fit(128, 0, 5, 5, &span) && span == 0);
    // the bound holds for, and is reached by, the tiles of small grids: every tile height, T_out around it, every tile position
    for (const int64_t bm : {1, 2, 3, 4, 8, 64}) {
        for (int64_t t_out = 1; t_out <= 2 * bm + 1; ++t_out) {
            const int64_t t_in = 3, ldx = 4, B = 2 * bm + 3, M = B * t_out;
            const int64_t bound = conv_tile_offset_span(bm, t_out, t_in, ldx);
            int64_t worst = 0;
            for (int64_t m0 = 0; m0 < M; ++m0) {  // any m0, not only multiples of bm: the bound does not lean on the alignment
                const int64_t w = walked_span(bm, t_out, t_in, ldx, m0, M);
                CHECK(w <= bound);
                worst = w > worst ? w : worst;
            }
            CHECK(worst == bound || worst == bound - t_in * ldx);  // never more than one clip of slack (bm = 3, t_out = 2 touches two, not three)
        }
    }
    std::puts("conv_offsets_selftest: ok");
    return 0;
}
