// align_kernels.hip — mel alignment: the DTW path between two sequences of mel rows in five passes over a launch group of pairs
// (align_means, align_quant, align_cost, align_dp, align_walk; the arithmetic: align.h).  A part of misc_kernels.hip's unit.
#include "kernels.h"
#include "align.h"

namespace zv
{

// ---------------------------------------------------------------------------------------------------
// Mel alignment (kernels.h: launch_align_*; the rule: align.h).  Sequence s = 2 pair + side (0: a, 1: b) owns the rows
// [row_a | row_b, + Ta | Tb) of the group's inputs, digit planes and norms; a pair owns the cells [cell0, + Ta * Tb) of cost and choice.
//   means: grid (blocks of 64 channels, sequences): lane = channel, the four waves take the rows t = w, w + 4, ...; the four i32 sums
//          are joined through LDS and the mean (align_mean) is stored.  Without normalise the mean is 0 and no row is read.
//   quant: grid (tiles of 16 rows, sequences): 16 threads per row, each takes the words (4 channels) g, g + 16, ... of the K-byte row,
//          stores the high and the low digit of q' to the two planes (zeros behind channel M) and joins the row norm over its 16 lanes.
//   cost:  grid (tiles of 64 columns, tiles of 64 rows, pairs): wave w takes the rows 16 w .. 16 w + 15 of the tile and its four column
//          tiles.  Per k step of 64 channels a lane loads two fragments of a and eight of b (16 bytes each, straight from the planes:
//          row-major with K a multiple of 64 IS the operand layout, lane l: row l & 15, bytes 64 step + 16 (l >> 4) + j) and issues 16
//          MFMAs into 12 accumulators: hi.hi, hi.lo + lo.hi and lo.lo per column tile.  A row behind the sequence's end is read as its last
//          row and not stored.  C/D: column = lane & 15, row = 4 (lane >> 4) + register.  The tile's costs meet in LDS and leave it diagonal
//          by diagonal: cost and choice are stored skewed (align_cell), where the cells of an anti-diagonal with consecutive rows
//          are consecutive entries, so a wave's store is one run of up to 256 bytes.
//   dp:    a workgroup of ALIGN_DP_ROWS threads per pair; thread r takes the rows r, r + ALIGN_DP_ROWS, ... and is at column s - r of its
//          pass at step s, so the row above is one step ahead: its value comes through LDS (double buffered, ONE barrier per step), the
//          diagonal value is what came the step before, the left value is the thread's own.  The last thread leaves its row in LDS
//          (s_edge) for thread 0's next pass; a pass starts every P = max(Tb, ALIGN_DP_ROWS) steps, so that row is complete up to the
//          column that is read.  The cell's cost is loaded one step ahead.  In the skewed matrices the threads of a pass read and
//          store consecutive entries in every step; the row (i + j) mod Tb moves on by one per step and is taken anew per pass.
//   walk:  one wave per pair.  The 64 lanes load the 8 x 8 window of choices and costs that ends at the current cell; the walk inside
//          the window is wave uniform (every lane takes the same steps on values read by index from the lanes), then the next window is
//          loaded.  Lane 0 stores the maps; the walk goes towards smaller i and j, so the last store of an entry is its smallest.
// Nothing in HBM to zero: every entry that is read was stored in the same run.
typedef int align_i4 __attribute__((ext_vector_type(4)));

struct AlignSeq
{
    int T, row0;
};
__device__ static inline AlignSeq align_seq(const AlignPair &p, int side) { return side ? AlignSeq{p.Tb, p.row_b} : AlignSeq{p.Ta, p.row_a}; }

__global__ __launch_bounds__(256) void align_means_kernel(const float *__restrict__ x, int32_t *__restrict__ means, const AlignPair *__restrict__ pairs,
                                                          int M, float scale, uint32_t normalise)
{
    __shared__ int32_t s_sum[4][ALIGN_SUM_CHANNELS];
    const int seq = blockIdx.y;
    const AlignSeq q = align_seq(pairs[seq >> 1], seq & 1);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, c = blockIdx.x * ALIGN_SUM_CHANNELS + lane;
    int32_t s = 0;                                                 // |s| <= 4096 * 1023
    if (normalise && c < M)
#pragma unroll 8
        for (int t = wv; t < q.T; t += 4) s += (int32_t)align_quant(x[((size_t)q.row0 + t) * M + c], (double)scale);
    s_sum[wv][lane] = s;
    __syncthreads();
    if (wv == 0 && c < M)
    {
        const int64_t sum = (int64_t)s_sum[0][lane] + s_sum[1][lane] + s_sum[2][lane] + s_sum[3][lane];
        means[(size_t)seq * ALIGN_MAX_MELS + c] = normalise ? align_mean(sum, q.T) : 0;
    }
}

__global__ __launch_bounds__(256) void align_quant_kernel(const float *__restrict__ x, const int32_t *__restrict__ means, int8_t *__restrict__ hi_plane,
                                                          int8_t *__restrict__ lo_plane, int32_t *__restrict__ norms,
                                                          const AlignPair *__restrict__ pairs, int M, float scale)
{
    const int seq = blockIdx.y;
    const AlignSeq q = align_seq(pairs[seq >> 1], seq & 1);
    if ((int)blockIdx.x * ALIGN_QUANT_ROWS >= q.T) return;         // the whole workgroup
    const int K = align_k(M), g = threadIdx.x & 15, row = blockIdx.x * ALIGN_QUANT_ROWS + (threadIdx.x >> 4);
    const bool live = row < q.T;
    const size_t at = (size_t)q.row0 + (live ? row : 0);
    int32_t norm = 0;                                              // <= 256 * 2046^2 < 2^31
    for (int w = g; w < K / 4; w += 16)
    {
        uint32_t whi = 0, wlo = 0;
#pragma unroll
        for (int e = 0; e < 4; e++)
        {
            const int c = 4 * w + e;
            int32_t v = 0, hi, lo;
            if (live && c < M) v = (int32_t)align_quant(x[at * M + c], (double)scale) - means[(size_t)seq * ALIGN_MAX_MELS + c];
            bands_digits(v, hi, lo);
            whi |= ((uint32_t)hi & 0xffu) << (8 * e);
            wlo |= ((uint32_t)lo & 0xffu) << (8 * e);
            norm += v * v;
        }
        if (live)
        {
            *(uint32_t *)(hi_plane + at * K + 4 * w) = whi;
            *(uint32_t *)(lo_plane + at * K + 4 * w) = wlo;
        }
    }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) norm += __shfl_xor(norm, o, 16);
    if (live && g == 0) norms[at] = norm;
}

__global__ __launch_bounds__(256) void align_cost_kernel(const int8_t *__restrict__ hi_plane, const int8_t *__restrict__ lo_plane,
                                                         const int32_t *__restrict__ norms, uint32_t *__restrict__ cost,
                                                         const AlignPair *__restrict__ pairs, int M)
{
    __shared__ uint32_t s_c[ALIGN_TILE][ALIGN_TILE + 2];           // (a diagonal's entries lie 65 words apart: no two lanes of 32 share a bank)
    const AlignPair p = pairs[blockIdx.z];
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int bi = blockIdx.y * ALIGN_TILE, i0 = bi + wv * 16, j0 = blockIdx.x * ALIGN_TILE;
    if (bi >= p.Ta || j0 >= p.Tb) return;                          // the whole workgroup
    const int K = align_k(M), r16 = lane & 15, g4 = lane >> 4;
    if (i0 < p.Ta)                                                 // the whole wave
    {
        const int ia = i0 + r16 < p.Ta ? i0 + r16 : p.Ta - 1;
        const size_t oa = ((size_t)p.row_a + ia) * K + 16 * g4;
        size_t ob[4];
#pragma unroll
        for (int ct = 0; ct < 4; ct++)
        {
            const int jb = j0 + ct * 16 + r16 < p.Tb ? j0 + ct * 16 + r16 : p.Tb - 1;
            ob[ct] = ((size_t)p.row_b + jb) * K + 16 * g4;
        }
        align_i4 acc[4][3];                                            // [column tile][hi.hi | hi.lo + lo.hi | lo.lo]
#pragma unroll
        for (int i = 0; i < 12; i++) (&acc[0][0])[i] = align_i4{0, 0, 0, 0};
        for (int ks = 0; ks < K / 64; ks++)
        {
            const align_i4 ah = *(const align_i4 *)(hi_plane + oa + ks * 64), al = *(const align_i4 *)(lo_plane + oa + ks * 64);
#pragma unroll
            for (int ct = 0; ct < 4; ct++)
            {
                const align_i4 bh = *(const align_i4 *)(hi_plane + ob[ct] + ks * 64), bl = *(const align_i4 *)(lo_plane + ob[ct] + ks * 64);
                acc[ct][0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ah, bh, acc[ct][0], 0, 0, 0);
                acc[ct][1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ah, bl, acc[ct][1], 0, 0, 0);
                acc[ct][1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(al, bh, acc[ct][1], 0, 0, 0);
                acc[ct][2] = __builtin_amdgcn_mfma_i32_16x16x64_i8(al, bl, acc[ct][2], 0, 0, 0);
            }
        }
#pragma unroll
        for (int reg = 0; reg < 4; reg++)
        {
            const int i = i0 + 4 * g4 + reg;
            if (i >= p.Ta) continue;
            const int64_t na = norms[(size_t)p.row_a + i];
#pragma unroll
            for (int ct = 0; ct < 4; ct++)
            {
                const int j = j0 + ct * 16 + r16;
                if (j >= p.Tb) continue;
                const int64_t dot = align_combine(acc[ct][0][reg], acc[ct][1][reg], acc[ct][2][reg]);
                const int64_t c = na + (int64_t)norms[(size_t)p.row_b + j] - 2 * dot;
                s_c[i - bi][j - j0] = (uint32_t)c;
            }
        }
    }
    __syncthreads();
    // the tile's 127 anti-diagonals, 64 rows each: a wave stores one diagonal's cells, consecutive entries of the skewed matrix
    for (int t = threadIdx.x; t < (2 * ALIGN_TILE - 1) * ALIGN_TILE; t += 256)
    {
        const int ii = t & (ALIGN_TILE - 1), jj = (t >> 6) - ii, i = bi + ii, j = j0 + jj;
        if (jj >= 0 && jj < ALIGN_TILE && i < p.Ta && j < p.Tb) cost[p.cell0 + align_cell(i, j, p.Ta, p.Tb)] = s_c[ii][jj];
    }
}

__global__ __launch_bounds__(ALIGN_DP_ROWS) void align_dp_kernel(const uint32_t *__restrict__ cost, uint8_t *__restrict__ choice,
                                                                 int64_t *__restrict__ totals, const AlignPair *__restrict__ pairs)
{
    __shared__ int64_t s_d[2][ALIGN_DP_ROWS];                      // D of every thread's cell, by the step's parity
    __shared__ int64_t s_edge[ALIGN_MAX_FRAMES];                   // the last thread's row, for thread 0's next pass
    const AlignPair p = pairs[blockIdx.x];
    const int Ta = p.Ta, Tb = p.Tb, r = threadIdx.x;
    if (Ta < 1 || Tb < 1 || Ta > (int)ALIGN_MAX_FRAMES || Tb > (int)ALIGN_MAX_FRAMES) return;      // the whole workgroup (the host checks)
    const int P = align_dp_stride(Tb), steps = align_dp_steps(Ta, Tb);
    const uint32_t *cp = cost + p.cell0;
    uint8_t *kp = choice + p.cell0;
    int ncol = -r, npass = 0;                                      // the cell of the NEXT step: column (negative: not started) and pass,
    int nrow = 0, noff = 0;                                        // its row (i + column) mod Tb of the skewed matrices and its entry there
    uint32_t cn = 0;
    auto fetch = [&]() {
        const int i = npass * ALIGN_DP_ROWS + r;
        if (ncol == 0) nrow = i % Tb;                              // once per pass; then one more per step
        else if (++nrow == Tb) nrow = 0;
        const bool in = ncol >= 0 && ncol < Tb && i < Ta;
        noff = in ? nrow * Ta + i : 0;                             // below 2^24
        cn = in ? cp[noff] : 0u;
    };
    fetch();
    int64_t up = 0, left = 0;
    for (int s = 0; s < steps; s++)
    {
        const int col = ncol, i = npass * ALIGN_DP_ROWS + r, off = noff;
        const uint32_t c = cn;
        ncol++;
        if (ncol == P) ncol = 0, npass++;
        fetch();                                                   // the next cell's cost is on its way
        if (col >= 0 && col < Tb && i < Ta)
        {
            const int64_t diag = up;                               // D[i-1][col-1]: what was the row above a step ago
            if (i > 0) up = r > 0 ? s_d[(s - 1) & 1][r - 1] : s_edge[col];
            uint32_t k;
            const int64_t d = (int64_t)c + align_choose(i > 0, col > 0, diag, up, left, k);
            left = d;
            s_d[s & 1][r] = d;
            if (r == ALIGN_DP_ROWS - 1) s_edge[col] = d;
            kp[off] = (uint8_t)k;
            if (i == Ta - 1 && col == Tb - 1) totals[blockIdx.x] = d;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(64) void align_walk_kernel(const uint32_t *__restrict__ cost, const uint8_t *__restrict__ choice,
                                                        const int64_t *__restrict__ totals, AlignRow *__restrict__ rows, int32_t *__restrict__ maps,
                                                        const AlignPair *__restrict__ pairs, float scale)
{
    const AlignPair p = pairs[blockIdx.x];
    const int Ta = p.Ta, Tb = p.Tb, lane = threadIdx.x;
    if (Ta < 1 || Tb < 1) return;
    const uint32_t *cp = cost + p.cell0;
    const uint8_t *kp = choice + p.cell0;
    int32_t *map_a = maps + p.map0, *map_b = map_a + Ta;
    int i = Ta - 1, j = Tb - 1;
    uint32_t L = 0;
    double acc = 0.0;
    bool done = false;
    while (!done)
    {
        const int wi = i - (lane >> 3), wj = j - (lane & 7);
        const bool in = wi >= 0 && wj >= 0;
        const size_t at = in ? align_cell(wi, wj, Ta, Tb) : 0;
        const int k_l = in ? (int)kp[at] : (int)ALIGN_NONE;
        const int c_l = in ? (int)cp[at] : 0;
        int di = 0, dj = 0;
        while (di < ALIGN_WINDOW && dj < ALIGN_WINDOW)
        {
            const int src = di * ALIGN_WINDOW + dj;
            const int k = __shfl(k_l, src, 64);
            const uint32_t c = (uint32_t)__shfl(c_l, src, 64);
            acc = align_step(acc, c);
            L++;
            if (lane == 0)
            {
                map_a[i - di] = j - dj;
                map_b[j - dj] = i - di;
            }
            const int ni = i - di - (k != 2), nj = j - dj - (k != 1);
            if (k == (int)ALIGN_NONE || ni < 0 || nj < 0)          // (0, 0); a choice that left the matrix would be a fault of the dp pass
            {
                done = true;
                break;
            }
            di += k != 2;
            dj += k != 1;
        }
        i -= di;
        j -= dj;
    }
    if (lane == 0) rows[blockIdx.x] = AlignRow{(uint64_t)totals[blockIdx.x], align_distance(acc, L, scale), L, 0u};
}

static bool align_job_ok(const AlignJob &j)
{
    const AlignPlan p = align_plan(j.n_pairs, j.max_ta, j.max_tb, j.M);
    return p.ok && j.x && j.means && j.hi_plane && j.lo_plane && !((uintptr_t)j.hi_plane & 15) && !((uintptr_t)j.lo_plane & 15) && j.norms && j.cost &&
           j.choice && j.totals && !((uintptr_t)j.totals & 7) && j.rows && !((uintptr_t)j.rows & 7) && j.maps && j.pairs && !((uintptr_t)j.pairs & 7) &&
           j.scale > 0.0f && j.normalise <= 1u;
}

hipError_t launch_align_means(hipStream_t s, const AlignJob &j)
{
    if (!align_job_ok(j)) return hipErrorInvalidValue;
    const AlignPlan p = align_plan(j.n_pairs, j.max_ta, j.max_tb, j.M);
    hipLaunchKernelGGL(align_means_kernel, dim3(p.means_gx, p.means_gy), dim3(256), 0, s, j.x, j.means, j.pairs, j.M, j.scale, j.normalise);
    return hipGetLastError();
}

hipError_t launch_align_quant(hipStream_t s, const AlignJob &j)
{
    if (!align_job_ok(j)) return hipErrorInvalidValue;
    const AlignPlan p = align_plan(j.n_pairs, j.max_ta, j.max_tb, j.M);
    hipLaunchKernelGGL(align_quant_kernel, dim3(p.quant_gx, p.quant_gy), dim3(256), 0, s, j.x, j.means, j.hi_plane, j.lo_plane, j.norms, j.pairs, j.M, j.scale);
    return hipGetLastError();
}

hipError_t launch_align_cost(hipStream_t s, const AlignJob &j)
{
    if (!align_job_ok(j)) return hipErrorInvalidValue;
    const AlignPlan p = align_plan(j.n_pairs, j.max_ta, j.max_tb, j.M);
    hipLaunchKernelGGL(align_cost_kernel, dim3(p.cost_gx, p.cost_gy, p.cost_gz), dim3(256), 0, s, j.hi_plane, j.lo_plane, j.norms, j.cost, j.pairs, j.M);
    return hipGetLastError();
}

hipError_t launch_align_dp(hipStream_t s, const AlignJob &j)
{
    if (!align_job_ok(j)) return hipErrorInvalidValue;
    const AlignPlan p = align_plan(j.n_pairs, j.max_ta, j.max_tb, j.M);
    hipLaunchKernelGGL(align_dp_kernel, dim3(p.dp_gx), dim3(ALIGN_DP_ROWS), 0, s, j.cost, j.choice, j.totals, j.pairs);
    return hipGetLastError();
}

hipError_t launch_align_walk(hipStream_t s, const AlignJob &j)
{
    if (!align_job_ok(j)) return hipErrorInvalidValue;
    const AlignPlan p = align_plan(j.n_pairs, j.max_ta, j.max_tb, j.M);
    hipLaunchKernelGGL(align_walk_kernel, dim3(p.walk_gx), dim3(64), 0, s, j.cost, j.choice, j.totals, j.rows, j.maps, j.pairs, j.scale);
    return hipGetLastError();
}

}  // namespace zv
