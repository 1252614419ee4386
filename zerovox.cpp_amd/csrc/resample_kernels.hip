// resample_kernels.hip — sample-rate conversion and PCM16 delivery (resample_kernel, resample_reduce_kernel; the arithmetic: resample.h).
// A part of misc_kernels.hip's unit.
#include "kernels.h"
#include "resample.h"

namespace zv
{

// ---------------------------------------------------------------------------------------------------
// Resampling (kernels.h: launch_resample; the rule and the deal: resample.h).  Grid (tiles, utterances).  Workgroup (t, u) owns the
// R * S consecutive outputs from n0 = t R S of utterance u (resample_tile).  Their input bases run from i_first = (n0 M) div L to
// ((n_last M) div L), so the samples x'[i_first - half + 1 .. i_last + half] go to LDS once, as f64, the finite test and the span test
// [0, S_in) applied there: nothing outside the utterance's own samples is ever loaded.  Slot s (thread s, s + 256, ...) owns the outputs
// n0 + s + r S, r < R: S is a multiple of L, so they share the phase p = ((n0 M) mod L + s M) mod L and their bases lie D = S M / L
// apart.  The slot walks its row of the table once, two taps per 8-byte load, in ascending order, and every tap feeds R independent
// chains: the per-lane fetch of a table row, which neighbouring slots cannot share (they are M mod L phases apart), is paid once for R
// multiply-adds.  Neighbouring slots store neighbouring samples.  An output past n_out reads the staged span's first samples and is
// dropped.  The PCM16 conversion, the peak and the clip count are part of the pass; a workgroup leaves one (peak, clips) pair.
// Nothing depends on the deal: every output is its own chain in tap order.
template <int R> __global__ __launch_bounds__(RESAMPLE_THREADS) void resample_kernel(const ResampleJob job, const int S, const int D)
{
    __shared__ double s_x[RESAMPLE_STAGE];
    __shared__ uint32_t s_red[2 * (RESAMPLE_THREADS / 64)];
    const int u = blockIdx.y, tid = threadIdx.x;
    const ResampleSeg sg = job.segs[u];
    const int tile = R * S;
    const int64_t n0 = (int64_t)blockIdx.x * tile;
    if (n0 >= sg.n_out) return;
    const int len = (int)(sg.n_out - n0 < tile ? sg.n_out - n0 : tile);
    const uint32_t L = job.L, M = job.M, P = job.P;
    const int half = (int)(P >> 1);
    const uint64_t t0 = (uint64_t)n0 * M;
    const int64_t i_first = (int64_t)(t0 / L);
    const uint32_t rem0 = (uint32_t)(t0 - (uint64_t)i_first * L);
    const int reach = (int)((rem0 + (uint32_t)(len - 1) * M) / L);      // i_last - i_first
    const int nst = reach + (int)P;
    if (nst > RESAMPLE_STAGE) return;                                   // (resample_tile picks no R that gets here)
    const float *xs = job.wav + sg.x0;
    const int64_t g0 = i_first - half + 1;
    for (int i = tid; i < nst; i += RESAMPLE_THREADS)
    {
        const int64_t g = g0 + i;
        double v = 0.0;
        if (g >= 0 && g < sg.S_in) v = loud_sample(xs[g]);
        s_x[i] = v;
    }
    __syncthreads();
    uint32_t peak = 0, clips = 0;
    for (int s = tid; s < S && s < len; s += RESAMPLE_THREADS)
    {
        const uint32_t q = rem0 + (uint32_t)s * M, io = q / L, p = q - io * L;
        const float2 *row = (const float2 *)(job.table + (size_t)p * P);
        int at[R];                                                      // x'[i0 - half + 1 + k] of output r at s_x[at[r] + k]
#pragma unroll
        for (int r = 0; r < R; r++) at[r] = s + r * S < len ? (int)io + r * D : 0;
        double acc[R];
#pragma unroll
        for (int r = 0; r < R; r++) acc[r] = 0.0;
        for (int k = 0; k < half; k++)
        {
            const float2 h = row[k];
            const double h0 = (double)h.x, h1 = (double)h.y;
#pragma unroll
            for (int r = 0; r < R; r++)
            {
                acc[r] = __builtin_fma(h0, s_x[at[r] + 2 * k], acc[r]);
                acc[r] = __builtin_fma(h1, s_x[at[r] + 2 * k + 1], acc[r]);
            }
        }
#pragma unroll
        for (int r = 0; r < R; r++)
        {
            if (s + r * S >= len) continue;
            const float y = (float)acc[r];
            const uint32_t a = level_abs_bits(y);
            peak = a > peak ? a : peak;
            const int64_t n = n0 + s + r * S;
            if (job.out) job.out[sg.y0 + n] = y;
            if (job.pcm) job.pcm[sg.y0 + n] = resample_pcm(y, job.flags, sg.seed, (uint64_t)n, &clips);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
    {
        const uint32_t v = (uint32_t)__shfl_xor((int)peak, o, 64);
        peak = v > peak ? v : peak;
        clips += (uint32_t)__shfl_xor((int)clips, o, 64);
    }
    const int w = tid >> 6;
    if ((tid & 63) == 0) s_red[2 * w] = peak, s_red[2 * w + 1] = clips;
    __syncthreads();
    if (tid == 0)
    {
        for (int k = 1; k < RESAMPLE_THREADS / 64; k++)
        {
            peak = s_red[2 * k] > peak ? s_red[2 * k] : peak;
            clips += s_red[2 * k + 1];
        }
        uint32_t *st = job.stats + 2 * ((size_t)sg.tile0 + blockIdx.x);
        st[0] = peak;
        st[1] = clips;
    }
}

// The reduction: one wave per utterance over its tiles' (peak, clips) pairs.
__global__ __launch_bounds__(64) void resample_reduce_kernel(const ResampleJob job)
{
    const int u = blockIdx.x, lane = threadIdx.x;
    const ResampleSeg sg = job.segs[u];
    const int64_t tiles = resample_tiles(sg.n_out, resample_tile_outputs(resample_tile(job.L, job.M, job.P)));
    const uint32_t *st = job.stats + 2 * (size_t)sg.tile0;
    uint32_t peak = 0;
    unsigned long long clips = 0;
    for (int64_t t = lane; t < tiles; t += 64)
    {
        peak = st[2 * t] > peak ? st[2 * t] : peak;
        clips += st[2 * t + 1];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
    {
        const uint32_t v = (uint32_t)__shfl_xor((int)peak, o, 64);
        peak = v > peak ? v : peak;
        clips += (unsigned long long)__shfl_xor((long long)clips, o, 64);
    }
    if (lane == 0)
    {
        ResampleRow r;
        r.n_out = (uint64_t)sg.n_out;
        r.clipped = job.pcm ? clips : 0;
        r.sample_peak = level_from_bits(peak);
        job.rows[u] = r;
    }
}

static bool resample_job_ok(const ResampleJob &j)
{
    return j.wav && (j.out || j.pcm) && j.table && j.stats && j.rows && j.segs && !((uintptr_t)j.wav & 15) && !((uintptr_t)j.out & 15) &&
           !((uintptr_t)j.pcm & 15) && !((uintptr_t)j.table & 7) && !(j.flags & ~RESAMPLE_FLAG_DITHER) &&
           resample_plan(j.max_n_out, j.nseg, j.L, j.M, j.P).ok;
}

hipError_t launch_resample(hipStream_t s, const ResampleJob &j)
{
    if (!resample_job_ok(j)) return hipErrorInvalidValue;
    const ResamplePlan p = resample_plan(j.max_n_out, j.nseg, j.L, j.M, j.P);
    const dim3 grid(p.gx, p.gy), block(RESAMPLE_THREADS);
    switch (p.tile.R)
    {
    case 8: hipLaunchKernelGGL(resample_kernel<8>, grid, block, 0, s, j, p.tile.S, p.tile.D); break;
    case 4: hipLaunchKernelGGL(resample_kernel<4>, grid, block, 0, s, j, p.tile.S, p.tile.D); break;
    case 2: hipLaunchKernelGGL(resample_kernel<2>, grid, block, 0, s, j, p.tile.S, p.tile.D); break;
    default: hipLaunchKernelGGL(resample_kernel<1>, grid, block, 0, s, j, p.tile.S, p.tile.D); break;
    }
    return hipGetLastError();
}

hipError_t launch_resample_reduce(hipStream_t s, const ResampleJob &j)
{
    if (!resample_job_ok(j)) return hipErrorInvalidValue;
    const ResamplePlan p = resample_plan(j.max_n_out, j.nseg, j.L, j.M, j.P);
    hipLaunchKernelGGL(resample_reduce_kernel, dim3(p.gy), dim3(64), 0, s, j);
    return hipGetLastError();
}

}  // namespace zv
