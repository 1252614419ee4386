// dec_runs.h — run-shortened decoding (DESIGN.md "Run-shortened decoding"): which rows of a padded utterance the StyleTTS decoder
// computes, where a row it skipped finds its value, and how the InstanceNorm statistics count the rows it skipped.  Plain integer
// arithmetic and one f64 sum, shared by the kernels (runs_kernels.hip, norm_kernels.hip), the schedule (decoder.cpp) and the host-side test
// (tests/native/dec_runs_check.cpp): nothing here needs HIP.
//
// Behind an utterance's n frames `hidden` is zero up to its capacity T.  Every decoder conv has 1 or 3 taps and every norm is a
// per-channel scalar over time, so after k 3-tap convs a tensor is constant over the rows [n + k, T - k); with R such convs in the
// chain every tensor of the decoder is constant over [n + R, T - R).  With
//     a = round_up(n + R + 32, 32),   b = round_down(T - R - 1, 32),   G = (b - a) / 32
// the decoder runs over the COMPACT segment of rows_c = a + (T - b) rows that stands for the rows [0, a) ++ [b, T): the G statistics
// blocks [a, b) are dropped.  Compact row a - 1's right neighbour is original row b, which holds what row a held (both constant), and
// b - 1 holds what a - 1 holds, so every compact row has its original neighbours' values in every layer.  a and b are multiples of the
// 32-row statistics block, so the kept blocks keep their rows, and each dropped block has the partial sums of block a / 32 - 1, whose
// rows [a - 32, a) are constant too (a - 32 >= n + R): dec_run_block_sum adds that block's pair G more times where the dropped
// blocks stood in the block-order sum.
#pragma once

#include <stddef.h>

#if defined(__HIPCC__)
#define ZV_DR_FN __host__ __device__ static inline
#else
#define ZV_DR_FN static inline
#endif

namespace zv
{

constexpr int DEC_RUN_BLOCK = 32;       // rows of a statistics block (kernels.h launch_stats_partial)
// Rows a run must save to be taken.  One block: a and b are block multiples, so a run saves whole blocks; every decoder kernel's
// row extent counts in units of 32 rows or more (statistics blocks, the narrowest conv row tile), so one block is the least that
// can take a workgroup away, and the table launch and the mel expansion are there whether an utterance takes its run or not.
constexpr int DEC_RUN_MARGIN = 32;

struct DecRun
{
    int rows_c;      // rows the decoder computes: T when the run is not taken
    int gap_at;      // statistics blocks in front of the gap (a / 32); 0 when the run is not taken
    int G;           // statistics blocks dropped; 0 when the run is not taken
};

// n: frames the length regulator filled (clamped to [0, T]), T: the segment's capacity, R: the reach of the decoder's 3-tap convs
ZV_DR_FN DecRun dec_run(int n, int T, int R)
{
    const DecRun whole = {T, 0, 0};
    n = n < 0 ? 0 : (n < T ? n : T);
    if (R < 0 || T - R - 1 < 0) return whole;
    const long a = ((long)n + R + 2 * DEC_RUN_BLOCK - 1) / DEC_RUN_BLOCK * DEC_RUN_BLOCK;
    const long b = (long)(T - R - 1) / DEC_RUN_BLOCK * DEC_RUN_BLOCK;
    if (b - a < DEC_RUN_BLOCK || b - a < DEC_RUN_MARGIN) return whole;
    const DecRun r = {(int)(a + (T - b)), (int)(a / DEC_RUN_BLOCK), (int)((b - a) / DEC_RUN_BLOCK)};
    return r;
}

// the expansion map: the compact row that holds original row t's value, and the original row compact row c was computed as
ZV_DR_FN int dec_run_compact_row(int t, int gap_at, int G)
{
    const int a = gap_at * DEC_RUN_BLOCK, b = a + G * DEC_RUN_BLOCK;
    return (G <= 0 || t < a) ? t : (t < b ? a - 1 : t - G * DEC_RUN_BLOCK);
}
ZV_DR_FN int dec_run_original_row(int c, int gap_at, int G) { return (G <= 0 || c < gap_at * DEC_RUN_BLOCK) ? c : c + G * DEC_RUN_BLOCK; }

// The block-order sum of a channel's f64 partial pairs (sum, sum of squares) over a compact segment's nb blocks, the pair of block
// gap_at - 1 added G more times right behind it: the chain of additions the plain sum over all nb + G blocks of the uncompacted
// segment makes.  p: the channel's pair of block 0, `stride` doubles from block to block.  Eight loads in flight, added in block
// order; with G = 0 the additions are the plain sum's.
ZV_DR_FN void dec_run_block_sum(const double *p, size_t stride, int nb, int gap_at, int G, double *sum, double *sumsq)
{
    double s1 = 0.0, s2 = 0.0;
    for (int b0 = 0; b0 < nb; b0 += 8)
    {
        double v1[8], v2[8];
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int i = 0; i < 8; i++)
        {
            const double *q = p + (size_t)(b0 + i < nb ? b0 + i : nb - 1) * stride;
            v1[i] = q[0];
            v2[i] = q[1];
        }
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int i = 0; i < 8; i++)
            if (b0 + i < nb)
            {
                s1 += v1[i];
                s2 += v2[i];
                if (b0 + i + 1 == gap_at)
                    for (int k = 0; k < G; k++)
                    {
                        s1 += v1[i];
                        s2 += v2[i];
                    }
            }
    }
    *sum = s1;
    *sumsq = s2;
}

// ---- densely packed decoding (DESIGN.md "Densely packed decoding") ----
// The compact segments of a batch back to back in ONE row space, so that the wide convs tile the batch and not every utterance by
// itself: utterance u owns the slot [row0_p, row0_p + slot) with
//     slot(u) = round_up(rows_c[u] + 1, 32),   row0_p[u] = sum of the slots in front of it,   L_p = sum of all slots.
// Rows [row0_p + rows_c, row0_p + slot) are the GUARD: at least one row, 32 when rows_c is a multiple of 32.  Every f16 conv operand
// holds zeros there, so a 3-tap conv over the packed rows [0, L_p) sees the zero row on either side of an utterance that the segment
// ends supply when every utterance is a segment of its own: each output element keeps its accumulation chain.  Every row0_p is a
// multiple of the statistics block, so an utterance's blocks are the global blocks row0_p / 32 + j.  What the convs leave in guard rows
// (outputs, partial sums of whole guard blocks) is never read; the last block of an utterance whose rows_c is no multiple of 32 also
// holds guard rows, and its pair is summed again from the rows that count (dec_pack_tail_pair) where the statistics are finalised.
constexpr int DEC_PACK_SLOT = 32;
// (an empty segment takes no rows: it has no row for a neighbour's tap to reach, and the guard in front of it stands)
ZV_DR_FN int dec_pack_slot(int rows_c) { return rows_c <= 0 ? 0 : (rows_c + DEC_PACK_SLOT) / DEC_PACK_SLOT * DEC_PACK_SLOT; }
// L_p never exceeds this, whatever the lengths: buffers, statistics partials and grids are sized by it
ZV_DR_FN long dec_pack_rows_cap(long t_rows, int nseg) { return t_rows + (long)DEC_PACK_SLOT * nseg; }

// The pair (sum, sum of squares) of one channel over the `rows` (1 .. 31) leading rows of a 32-row block, as the conv epilogues add
// it (mfma_common.h tile_stats_store, conv_gemm.hip): two sequential f64 chains, over the rows 0-3, 8-11, 16-19, 24-27 and over the
// rows 4-7, 12-15, 20-23, 28-31, a row at or past `rows` counting as zero, then the sum of the two.  x: the channel's value in the
// block's first row, ld floats from row to row; rows at or past `rows` are not read.
ZV_DR_FN void dec_pack_tail_pair(const float *x, size_t ld, int rows, double *sum, double *sumsq)
{
    double s1[2] = {0.0, 0.0}, s2[2] = {0.0, 0.0};
    for (int h = 0; h < 2; h++)
        for (int r = 0; r < 16; r++)
        {
            const int t = 4 * h + (r & 3) + 8 * (r >> 2);
            const double v = t < rows ? (double)x[(size_t)t * ld] : 0.0;
            s1[h] += v;
            s2[h] += v * v;
        }
    *sum = s1[0] + s1[1];
    *sumsq = s2[0] + s2[1];
}

}  // namespace zv
