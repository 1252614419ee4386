// loudness_kernels.hip — loudness: K-weighting in chunks (phases A, B, C), the true peak, the gates with the gain, the apply pass
// (the arithmetic: loudness.h).  A part of misc_kernels.hip's unit.
#include "kernels.h"
#include "loudness.h"
#include "stage_plan.h"

namespace zv
{

// ---------------------------------------------------------------------------------------------------
// Loudness (kernels.h: launch_loud_*; the rule: loudness.h).  Six launches over ONE launch group of utterances (LoudJob), whatever the
// group; utterance u is blockIdx.y of the passes over samples and finds its arrays through segs[u].
//   chunks<false> (phase A): lane = chunk k of utterance u, run from the zero state; state[chunk0 + k] = z_k
//   states        (phase B): lane = utterance; s_0 = 0, s_(k+1) = M s_k + z_k in k; state[chunk0 + k] = s_k in place of z_k
//   chunks<true>  (phase C): lane = chunk k again, run from s_k; runs[chunk0 + k] = its two run sums
//   peak:         workgroup = LOUD_TP_TILE outputs of the three interpolated phases; peaks[tile0 + t] = {max |v| as f64 bits, max |x| as f32 bits}
//   gate:         one wave per utterance: phase D, blocks, short-term sums, the maxima, the two gated sums, report and gain; rows[u]
//   apply:        wav[i] *= rows[u].gain over the utterance's capacity
// No atomics, nothing to zero: every entry a pass reads was stored by a pass before it in the same run.
//
// The two chunk passes.  A lane walks its chunk sample by sample (the recursion leaves no other way), so 64 lanes read 64 addresses 1 KB
// apart: straight from HBM that is a cache line per lane and load.  A workgroup (one wave, LOUD_WG_CHUNKS = 64 chunks) stages
// LOUD_SLICE = 64 samples of each of its chunks through LDS instead: 16 lanes fetch the 256 contiguous bytes of a chunk's slice as
// float4s, four chunks per load instruction.  A row of the LDS tile is LOUD_SLICE + 1 floats: lane l reads word 65 l + i, bank
// (l + i) mod 64 — 64 lanes, 64 banks; the staging stores of one instruction go to rows r .. r + 3 and columns 4 c + j: banks
// r + 4 c + j (+ 65 r'), 64 distinct ones again.  The span test (n < N) and the finite test are applied at staging, so nothing past
// the span reaches a chain; every utterance's region is padded to whole chunks, so no load leaves it.  16.6 KB of LDS and one wave per
// workgroup: nine workgroups fit a CU, and 32 x 1 024 frames of hop 256 are 512 workgroups on 256 CUs — the pass is bound by the
// dependent f64 chain (three operations per sample and stage), not by occupancy.
constexpr int LOUD_ROW = LOUD_SLICE + 1;
static_assert(LOUD_WG_CHUNKS == 64 && LOUD_SLICE == 64 && LOUD_CHUNK % LOUD_SLICE == 0, "a lane per chunk, 16 lanes per slice row");

template <bool PHASE_C>
__global__ __launch_bounds__(LOUD_WG_CHUNKS) void loud_chunks_kernel(const LoudJob job)
{
    __shared__ float s_x[LOUD_WG_CHUNKS * LOUD_ROW];
    const int u = blockIdx.y, lane = threadIdx.x;
    const LoudSeg sg = job.segs[u];
    const int64_t nch = loud_chunks(sg.N);
    const int64_t k0 = (int64_t)blockIdx.x * LOUD_WG_CHUNKS;
    if (k0 >= nch) return;
    const int64_t k = k0 + lane;
    const LoudFilter F = *job.filter;
    const float *xs = job.wav + sg.x0;
    double s[4] = {0.0, 0.0, 0.0, 0.0}, run[2] = {0.0, 0.0};
    if (PHASE_C && k < nch)
    {
        const double2 a = *(const double2 *)(job.state + 4 * ((size_t)sg.chunk0 + k)), b = *(const double2 *)(job.state + 4 * ((size_t)sg.chunk0 + k) + 2);
        s[0] = a.x, s[1] = a.y, s[2] = b.x, s[3] = b.y;
    }
    const int64_t edge = loud_edge(k, job.step);
    const int col = (lane & 15) * 4, row0 = lane >> 4;
    for (int sl = 0; sl < LOUD_CHUNK / LOUD_SLICE; sl++)
    {
        __syncthreads();
#pragma unroll 4
        for (int it = 0; it < LOUD_WG_CHUNKS / 4; it++)
        {
            const int r = it * 4 + row0;
            const int64_t n = (k0 + r) * LOUD_CHUNK + sl * LOUD_SLICE + col;      // < the padded capacity wherever k0 + r < nch
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (k0 + r < nch) v = *(const float4 *)(xs + n);
            float *d = s_x + r * LOUD_ROW + col;
            d[0] = n < sg.N && loud_finite(v.x) ? v.x : 0.0f;
            d[1] = n + 1 < sg.N && loud_finite(v.y) ? v.y : 0.0f;
            d[2] = n + 2 < sg.N && loud_finite(v.z) ? v.z : 0.0f;
            d[3] = n + 3 < sg.N && loud_finite(v.w) ? v.w : 0.0f;
        }
        __syncthreads();
        const float *mine = s_x + lane * LOUD_ROW;
        const int64_t n0 = k * LOUD_CHUNK + sl * LOUD_SLICE;
#pragma unroll 8
        for (int i = 0; i < LOUD_SLICE; i++)
        {
            const double w = loud_kweight(F, s, (double)mine[i]);
            if (PHASE_C) loud_run_add(run, w, n0 + i >= edge);
        }
    }
    if (k >= nch) return;
    if (PHASE_C)
        *(double2 *)(job.runs + 2 * ((size_t)sg.chunk0 + k)) = make_double2(run[0], run[1]);
    else
    {
        double *st = job.state + 4 * ((size_t)sg.chunk0 + k);
        *(double2 *)st = make_double2(s[0], s[1]);
        *(double2 *)(st + 2) = make_double2(s[2], s[3]);
    }
}

// Phase B: small and serial.  A lane per utterance keeps s and M in registers; the z_k of LOUD_B_AHEAD steps are loaded before the
// first of them is used, so the chain waits for memory once per LOUD_B_AHEAD steps.
constexpr int LOUD_B_AHEAD = 8;
__global__ __launch_bounds__(64) void loud_states_kernel(const LoudJob job)
{
    const int u = blockIdx.x * 64 + threadIdx.x;
    if (u >= job.nseg) return;
    const LoudSeg sg = job.segs[u];
    const int64_t nch = loud_chunks(sg.N);
    double M[16];
#pragma unroll
    for (int i = 0; i < 16; i++) M[i] = job.filter->M[i];
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    double *st = job.state + 4 * (size_t)sg.chunk0;
    for (int64_t k = 0; k < nch; k += LOUD_B_AHEAD)
    {
        double z[LOUD_B_AHEAD][4];
#pragma unroll
        for (int j = 0; j < LOUD_B_AHEAD; j++)
            if (k + j < nch)
            {
                const double2 a = *(const double2 *)(st + 4 * (k + j)), b = *(const double2 *)(st + 4 * (k + j) + 2);
                z[j][0] = a.x, z[j][1] = a.y, z[j][2] = b.x, z[j][3] = b.y;
            }
#pragma unroll
        for (int j = 0; j < LOUD_B_AHEAD; j++)
            if (k + j < nch)
            {
                *(double2 *)(st + 4 * (k + j)) = make_double2(s[0], s[1]);
                *(double2 *)(st + 4 * (k + j) + 2) = make_double2(s[2], s[3]);
                loud_advance(M, s, z[j]);
            }
    }
}

// ---------------------------------------------------------------------------------------------------
// True peak, in the manner of filter_kernel: workgroup (t, u) owns the outputs n = t0 .. t0 + LOUD_TP_TILE of utterance u, t0 = t *
// LOUD_TP_TILE, lane l the 8 outputs t0 + 8 l + r.  The samples x'[t0 - 11 .. t0 + LOUD_TP_TILE) go to LDS as f64, the span test [0, N)
// and the finite test applied there; staged element i lies at i + (i >> 3) doubles, so lanes read at a stride of 9 doubles, an odd
// count (filter_kernels.hip).  A lane holds the 19 elements its outputs need in registers and runs 3 x 8 chains of 12 steps in tap
// order.  Outputs behind N + 11 see zeros only and give +0.0, so the last tile needs no mask.  The maxima are maxima of bit patterns
// of non-negative values, which no order changes.
constexpr int LOUD_TP_R = 8;
constexpr int LOUD_TP_STAGE = LOUD_TP_TILE + LOUD_TP_TAIL;
__device__ __forceinline__ int loud_tp_at(int i) { return i + (i >> 3); }

__global__ __launch_bounds__(256) void loud_peak_kernel(const LoudJob job)
{
    __shared__ double s_x[LOUD_TP_STAGE + LOUD_TP_STAGE / LOUD_TP_R + 1];
    __shared__ float s_c[LOUD_TAPS];
    __shared__ unsigned long long red_t[4];
    __shared__ uint32_t red_p[4];
    const int u = blockIdx.y;
    const LoudSeg sg = job.segs[u];
    const int64_t t0 = (int64_t)blockIdx.x * LOUD_TP_TILE;
    if (t0 >= sg.N + LOUD_TP_TAIL) return;
    const float *xs = job.wav + sg.x0;
    if (threadIdx.x < LOUD_TAPS) s_c[threadIdx.x] = job.filter->c[threadIdx.x];
    uint32_t sp = 0;
    for (int i = threadIdx.x; i < LOUD_TP_STAGE; i += 256)
    {
        const int64_t g = t0 - LOUD_TP_TAIL + i;
        double v = 0.0;
        if (g >= 0 && g < sg.N)
        {
            const float x = xs[g];
            v = loud_sample(x);
            const uint32_t a = level_abs_bits(x);
            sp = a > sp ? a : sp;
        }
        s_x[loud_tp_at(i)] = v;
    }
    __syncthreads();
    // output 8 l + r at tap k reads x'[n - k] = staged element 8 l + r + 11 - k: e[r + 11 - k]
    double e[LOUD_TP_R + LOUD_TP_TAIL];
    const int base = (int)threadIdx.x * LOUD_TP_R;
#pragma unroll
    for (int j = 0; j < LOUD_TP_R + LOUD_TP_TAIL; j++) e[j] = s_x[loud_tp_at(base + j)];
    unsigned long long tp = 0;
#pragma unroll
    for (int f = 1; f < 4; f++)
    {
        double acc[LOUD_TP_R];
#pragma unroll
        for (int r = 0; r < LOUD_TP_R; r++) acc[r] = 0.0;
#pragma unroll
        for (int k = 0; k < LOUD_PHASE_TAPS; k++)
        {
            const float c = s_c[f + 4 * k];
#pragma unroll
            for (int r = 0; r < LOUD_TP_R; r++) acc[r] = loud_tp_step(acc[r], c, e[r + LOUD_TP_TAIL - k]);
        }
#pragma unroll
        for (int r = 0; r < LOUD_TP_R; r++)
        {
            const unsigned long long b = loud_dbits(fabs(acc[r]));
            tp = b > tp ? b : tp;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
    {
        const unsigned long long t = (unsigned long long)__shfl_xor((long long)tp, o, 64);
        tp = t > tp ? t : tp;
        const uint32_t p = (uint32_t)__shfl_xor((int)sp, o, 64);
        sp = p > sp ? p : sp;
    }
    if ((threadIdx.x & 63) == 0)
    {
        red_t[threadIdx.x >> 6] = tp;
        red_p[threadIdx.x >> 6] = sp;
    }
    __syncthreads();
    if (threadIdx.x == 0)
    {
        for (int w = 1; w < 4; w++)
        {
            tp = red_t[w] > tp ? red_t[w] : tp;
            sp = red_p[w] > sp ? red_p[w] : sp;
        }
        unsigned long long *o = (unsigned long long *)job.peaks + 2 * ((size_t)sg.tile0 + blockIdx.x);
        o[0] = tp;
        o[1] = sp;
    }
}

// ---------------------------------------------------------------------------------------------------
// The gates: one wave per utterance.  The step energies, the momentary blocks, the short-term sums and the maxima are independent
// values, a lane each; the two gated sums are ONE chain in block order: a wave loads 64 blocks at a time, a lane each, and every lane
// adds them in order from the shuffled values — 64 copies of the same chain, the rule's.
__device__ __forceinline__ double loud_wave_max(double v)
{
    unsigned long long b = loud_dbits(v);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
    {
        const unsigned long long t = (unsigned long long)__shfl_xor((long long)b, o, 64);
        b = t > b ? t : b;
    }
    return mel_from_bits(b);
}

__global__ __launch_bounds__(64) void loud_gate_kernel(const LoudJob job)
{
    const int u = blockIdx.x, lane = threadIdx.x;
    const LoudSeg sg = job.segs[u];
    const uint32_t step = job.step;
    const int64_t J = sg.N / step, nb = J >= 4 ? J - 3 : 0;
    const double *runs = job.runs + 2 * (size_t)sg.chunk0;
    double *E = job.energy + sg.step0, *z = job.blocks + sg.step0;
    for (int64_t j = lane; j < J; j += 64) E[j] = loud_step_energy(runs, j, step);
    __syncthreads();
    double mom = 0.0, sht = 0.0;
    for (int64_t i = lane; i < nb; i += 64)
    {
        const double v = loud_momentary(E, i, step);
        z[i] = v;
        mom = v > mom ? v : mom;
    }
    for (int64_t i = lane; i + 30 <= J; i += 64)
    {
        const double v = loud_short_term(E, i, step);
        sht = v > sht ? v : sht;
    }
    unsigned long long tpb = 0;
    uint32_t spb = 0;
    const unsigned long long *pk = (const unsigned long long *)job.peaks + 2 * (size_t)sg.tile0;
    const int64_t tiles = loud_tp_tiles(sg.N);
    for (int64_t t = lane; t < tiles && sg.N > 0; t += 64)
    {
        tpb = pk[2 * t] > tpb ? pk[2 * t] : tpb;
        spb = (uint32_t)pk[2 * t + 1] > spb ? (uint32_t)pk[2 * t + 1] : spb;
    }
    mom = loud_wave_max(mom);
    sht = loud_wave_max(sht);
    const float sp = (float)loud_wave_max((double)level_from_bits(spb));      // (f32 -> f64 -> f32 is the identity)
    double tp = loud_wave_max(mel_from_bits(tpb));
    tp = (double)sp > tp ? (double)sp : tp;
    __syncthreads();
    const double ga = loud_gate_abs();
    double sum = 0.0;
    uint32_t na = 0, ng = 0;
    for (int64_t b0 = 0; b0 < nb; b0 += 64)
    {
        const double mine = b0 + lane < nb ? z[b0 + lane] : 0.0;
        const int cnt = (int)(nb - b0 < 64 ? nb - b0 : 64);
        for (int t = 0; t < cnt; t++)
        {
            const double v = __shfl(mine, t, 64);
            if (v > ga)
            {
                sum = sum + v;
                na++;
            }
        }
    }
    double z_int = 0.0;
    if (na)
    {
        const double gr = loud_gate_rel(sum, na);
        sum = 0.0;
        for (int64_t b0 = 0; b0 < nb; b0 += 64)
        {
            const double mine = b0 + lane < nb ? z[b0 + lane] : 0.0;
            const int cnt = (int)(nb - b0 < 64 ? nb - b0 : 64);
            for (int t = 0; t < cnt; t++)
            {
                const double v = __shfl(mine, t, 64);
                if (v > ga && v > gr)
                {
                    sum = sum + v;
                    ng++;
                }
            }
        }
        if (ng) z_int = sum / (double)ng;
    }
    if (lane == 0) job.rows[u] = loud_finish(z_int, mom, sht, (uint32_t)nb, na, ng, tp, sp, job.asks[u]);
}

// The apply pass: workgroup (t, u) scales LOUD_APPLY_TILE samples of utterance u's capacity by the gain the gate kernel stored.
__global__ __launch_bounds__(256) void loud_apply_kernel(const LoudJob job)
{
    const int u = blockIdx.y;
    const LoudSeg sg = job.segs[u];
    const int64_t t0 = (int64_t)blockIdx.x * LOUD_APPLY_TILE;
    if (t0 >= sg.total) return;
    const float g = job.rows[u].gain;
    float *xs = job.wav + sg.x0;
#pragma unroll
    for (int k = 0; k < LOUD_APPLY_TILE / 1024; k++)
    {
        const int64_t i = t0 + k * 1024 + (int64_t)threadIdx.x * 4;
        if (i + 4 <= sg.total)
        {
            const float4 v = *(const float4 *)(xs + i);
            *(float4 *)(xs + i) = make_float4(v.x * g, v.y * g, v.z * g, v.w * g);
        }
        else
            for (int64_t j = i; j < sg.total; j++) xs[j] = xs[j] * g;
    }
}

static bool loud_job_ok(const LoudJob &j)
{
    return j.wav && j.state && j.runs && j.energy && j.blocks && j.peaks && j.rows && j.segs && j.asks && j.filter && !((uintptr_t)j.wav & 15) &&
           !((uintptr_t)j.state & 15) && !((uintptr_t)j.runs & 15) && loud_plan(j.max_N, j.max_total, j.nseg, j.step).ok;
}

hipError_t launch_loud_chunks(hipStream_t s, const LoudJob &j, bool phase_c)
{
    if (!loud_job_ok(j)) return hipErrorInvalidValue;
    const LoudPlan p = loud_plan(j.max_N, j.max_total, j.nseg, j.step);
    if (!p.chunk_gx) return hipSuccess;
    if (phase_c) hipLaunchKernelGGL(loud_chunks_kernel<true>, dim3(p.chunk_gx, p.gy), dim3(LOUD_WG_CHUNKS), 0, s, j);
    else hipLaunchKernelGGL(loud_chunks_kernel<false>, dim3(p.chunk_gx, p.gy), dim3(LOUD_WG_CHUNKS), 0, s, j);
    return hipGetLastError();
}

hipError_t launch_loud_states(hipStream_t s, const LoudJob &j)
{
    if (!loud_job_ok(j)) return hipErrorInvalidValue;
    const LoudPlan p = loud_plan(j.max_N, j.max_total, j.nseg, j.step);
    if (!p.chunk_gx) return hipSuccess;
    hipLaunchKernelGGL(loud_states_kernel, dim3(p.states_gx), dim3(64), 0, s, j);
    return hipGetLastError();
}

hipError_t launch_loud_peak(hipStream_t s, const LoudJob &j)
{
    if (!loud_job_ok(j)) return hipErrorInvalidValue;
    const LoudPlan p = loud_plan(j.max_N, j.max_total, j.nseg, j.step);
    if (!p.chunk_gx) return hipSuccess;
    hipLaunchKernelGGL(loud_peak_kernel, dim3(p.tp_gx, p.gy), dim3(256), 0, s, j);
    return hipGetLastError();
}

hipError_t launch_loud_gate(hipStream_t s, const LoudJob &j)
{
    if (!loud_job_ok(j)) return hipErrorInvalidValue;
    const LoudPlan p = loud_plan(j.max_N, j.max_total, j.nseg, j.step);
    hipLaunchKernelGGL(loud_gate_kernel, dim3(p.gy), dim3(64), 0, s, j);
    return hipGetLastError();
}

hipError_t launch_loud_apply(hipStream_t s, const LoudJob &j)
{
    if (!loud_job_ok(j)) return hipErrorInvalidValue;
    const LoudPlan p = loud_plan(j.max_N, j.max_total, j.nseg, j.step);
    hipLaunchKernelGGL(loud_apply_kernel, dim3(p.apply_gx, p.gy), dim3(256), 0, s, j);
    return hipGetLastError();
}

}  // namespace zv
