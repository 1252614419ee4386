// filter_kernels.hip — waveform filter: one pass from the vocoder's waveform to the waveform every later pass sees (filter_kernel; the
// arithmetic: filter.h).  A part of misc_kernels.hip's unit.
#include "kernels.h"
#include "filter.h"

namespace zv
{

// ---------------------------------------------------------------------------------------------------
// Waveform filter (kernels.h: launch_filter; the rule: filter.h).  Grid (tiles of FILTER_TILE outputs, segments).  Workgroup (t, u)
// owns the outputs [t * FILTER_TILE, (t + 1) * FILTER_TILE) of segment u's capacity.
//   n_taps == 0: the tile is copied, bit for bit.
//   else:        with R = FILTER_LANE_OUTPUTS: the taps go to LDS as f64, padded with +0.0 to Lp, the next multiple of R (a step with a
//                +0.0 tap leaves a chain as it is: filter.h); the samples x'[t0 - (Lp - 1 - c) .. t0 + FILTER_TILE + c) go to LDS as
//                f64, the finite test and the span test [0, S) applied there, so nothing past the segment's own samples is ever
//                loaded.  Lane l owns the R outputs t0 + R l + r and walks the taps in ascending order; output r at tap k needs
//                staged element R l + r + q, q = Lp - 1 - k.  The R elements a step needs live in R registers, element e in register
//                e mod R: a step reads ONE new element from LDS (e = R l + q - 1, into the register the step's last chain has just
//                let go) and feeds R independent chains.  Unrolled by R, every register index is a constant.
// LDS: element i lies at i + (i >> log2 R) doubles: lanes then read at a stride of R + 1 doubles, an odd count, which is conflict free for the
// 32 lanes of a ds_read_b64 group (2 (R + 1) l mod 64 takes 32 distinct even values), where the plain stride would be R-way.
// Nothing depends on the deal: every output is its own chain in tap order.
constexpr int FILTER_R = FILTER_LANE_OUTPUTS;
static_assert((FILTER_R & (FILTER_R - 1)) == 0 && FILTER_R >= 4 && FILTER_R <= 16, "register indices are taken mod R; the stores move float4s");
constexpr int FILTER_LP_MAX = ((int)FILTER_MAX_TAPS + FILTER_R - 1) & ~(FILTER_R - 1);      // 512
constexpr int FILTER_STAGE = FILTER_TILE + FILTER_LP_MAX;                      // elements staged at most: FILTER_TILE + Lp - 1
constexpr int FILTER_STAGE_LDS = FILTER_STAGE + FILTER_STAGE / FILTER_R + 1;    // with the padding

// (a shift, not a division: the compiler then folds a lane's R l + constant into one base address and constant offsets)
constexpr int FILTER_R_LOG2 = __builtin_ctz((unsigned)FILTER_R);
__device__ __forceinline__ int filter_lds_at(int i) { return i + (i >> FILTER_R_LOG2); }

__global__ __launch_bounds__(256) void filter_kernel(const float *__restrict__ in, float *__restrict__ out, const uint32_t *__restrict__ par,
                                                     const Segs frames, const Segs live, int hop)
{
    __shared__ double s_x[FILTER_STAGE_LDS];
    __shared__ double s_h[FILTER_LP_MAX];
    const int u = blockIdx.y;
    const Seg cap = seg_at(frames, u), lv = seg_at(live, u);
    const long total = (long)cap.rows * hop;
    const long t0 = (long)blockIdx.x * FILTER_TILE;
    if (t0 >= total) return;
    const int lrows = lv.rows < 0 ? 0 : (lv.rows < cap.rows ? lv.rows : cap.rows);
    const long S = (long)lrows * hop;
    const float *xs = in + (size_t)cap.row0 * hop;
    float *ys = out + (size_t)cap.row0 * hop;
    const uint32_t *row = par + (size_t)u * FILTER_PARAM_STRIDE;
    int L = __builtin_amdgcn_readfirstlane((int)row[0]);
    const int len = (int)(total - t0 < FILTER_TILE ? total - t0 : FILTER_TILE);
    const int n0 = (int)threadIdx.x * FILTER_LANE_OUTPUTS;
    float *yo = ys + t0 + n0;
    const bool vec = ((uintptr_t)yo & 15) == 0 && n0 + FILTER_LANE_OUTPUTS <= len;
    if (L <= 0 || L > (int)FILTER_MAX_TAPS)
    {
        // no filter on this segment: its capacity as it is (bit patterns, so a NaN's payload and a -0.0 come through)
        const uint32_t *xi = (const uint32_t *)(xs + t0);
        uint32_t *yi = (uint32_t *)(ys + t0);
        for (int i = threadIdx.x; i < len; i += 256) yi[i] = xi[i];
        return;
    }
    if (t0 >= S)
    {
        // behind the span: silence
        for (int i = threadIdx.x; i < len; i += 256) ys[t0 + i] = 0.0f;
        return;
    }
    constexpr int R = FILTER_R;
    const int c = (L - 1) >> 1, Lp = (L + R - 1) & ~(R - 1), nb = Lp / R;
    for (int k = threadIdx.x; k < Lp; k += 256) s_h[k] = k < L ? (double)level_from_bits(row[1 + k]) : 0.0;
    // staged element i is x'[g0 + i], g0 = t0 - (Lp - 1 - c); i < FILTER_TILE + Lp - 1
    const long g0 = t0 - (Lp - 1 - c);
    const int nst = FILTER_TILE + Lp - 1;
    for (int i = threadIdx.x; i < nst; i += 256)
    {
        const long g = g0 + i;
        double v = 0.0;
        if (g >= 0 && g < S) v = filter_sample(xs[g]);
        s_x[filter_lds_at(i)] = v;
    }
    __syncthreads();
    double acc[R], reg[R];
#pragma unroll
    for (int r = 0; r < R; r++) acc[r] = 0.0;
    // q = Lp - 1 = R (nb - 1) + R - 1: elements R l + q .. R l + q + R - 1, element e in register e mod R
    {
        const int e0 = n0 + R * (nb - 1);
        reg[R - 1] = s_x[filter_lds_at(e0 + R - 1)];
#pragma unroll
        for (int j = 0; j < R - 1; j++) reg[j] = s_x[filter_lds_at(e0 + R + j)];
    }
    for (int qb = nb - 1; qb >= 0; qb--)
    {
        const double *hk = s_h + R * (nb - 1 - qb);
        const int eb = n0 + R * qb;                                 // element R l + q at step s is eb + R - 1 - s
#pragma unroll
        for (int s = 0; s < R; s++)
        {
            const double h = hk[s];
#pragma unroll
            for (int r = 0; r < R; r++) acc[r] = __builtin_fma(h, reg[(r + R - 1 - s) & (R - 1)], acc[r]);
            // the element of the next step, R l + q - 1 = eb + R - 2 - s (the last step of the last block has none)
            if (s < R - 1 || qb > 0) reg[(R - 2 - s) & (R - 1)] = s_x[filter_lds_at(eb + R - 2 - s)];
        }
    }
    if (vec)
    {
#pragma unroll
        for (int r = 0; r < R; r += 4)
        {
            float y[4];
#pragma unroll
            for (int j = 0; j < 4; j++) y[j] = t0 + n0 + r + j < S ? (float)acc[r + j] : 0.0f;
            *(float4 *)(yo + r) = make_float4(y[0], y[1], y[2], y[3]);
        }
    }
    else
    {
#pragma unroll
        for (int r = 0; r < R; r++)
            if (n0 + r < len) yo[r] = t0 + n0 + r < S ? (float)acc[r] : 0.0f;
    }
}

hipError_t launch_filter(hipStream_t s, const float *in, float *out, const uint32_t *par, const Segs &frames, const Segs &live, int hop)
{
    if (frames.nseg < 1 || frames.max_rows < 1 || live.nseg != frames.nseg || hop < 1 || !in || !out || in == out || !par ||
        (!frames.tab && frames.nseg != 1) || (!live.tab && live.nseg != 1))
        return hipErrorInvalidValue;
    const FilterPlan p = filter_plan(frames.max_rows, hop);
    hipLaunchKernelGGL(filter_kernel, dim3(p.tiles, frames.nseg), dim3(256), 0, s, in, out, par, frames, live, hop);
    return hipGetLastError();
}

}  // namespace zv
