// runs_kernels.hip — the run tables of the run-shortened schedules: the vocoder's (voc_run_*) and the decoder's (dec_runs,
// dec_pack_rows, dec_run_expand; the rule: dec_runs.h).  A part of misc_kernels.hip's unit.
#include "kernels.h"
#include "dec_runs.h"

namespace zv
{

// ---------------------------------------------------------------------------------------------------
// Run-shortened vocoding (kernels.h: launch_voc_runs).  Behind an utterance's end the decoder's mel rows are bit-identical, and
// the vocoder is shift-invariant with a reach of H frames, so the waveform over such a run is one frame, repeated.  Three steps,
// all on the device so that the schedule stays one graph: (1) eq[row] = "this mel row has the bits of the row above it",
// (2) per segment the first longest run [a, b) of equal rows -> the table entry, (3) the compacted mel.
//   taken (b - a >= 2H + 1 + VOC_RUN_MARGIN): runs[u] = {row0, T - (b - a - (2H + 1)), split = a + H, shift = b - a - (2H + 1)}
//   otherwise:                                runs[u] = {row0, T, split = T, shift = 0}
// Rows are compared as 32-bit integers: -0 and +0 differ, equal NaN patterns are equal.
__global__ __launch_bounds__(256) void voc_run_flags_kernel(const uint32_t *__restrict__ mel, int M, int32_t *__restrict__ eq, const Segs frames)
{
    const Seg sg = seg_at(frames, blockIdx.y);
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (t >= sg.rows) return;
    int same = t > 0;
    if (t > 0)
    {
        const uint32_t *r = mel + (size_t)(sg.row0 + t) * M;
        for (int c = lane; c < M; c += 64) same &= r[c] == r[c - M];
    }
    same = __all(same);
    if (lane == 0) eq[sg.row0 + t] = same;
}

__global__ __launch_bounds__(256) void voc_run_scan_kernel(const int32_t *__restrict__ eq, Seg *__restrict__ runs, const Segs frames, int H)
{
    // per thread one contiguous chunk of the segment's flags: leading ones, trailing ones, the first longest run of ones inside
    __shared__ int s_pre[256], s_suf[256], s_len[256], s_pos[256];
    const Seg sg = seg_at(frames, blockIdx.x);
    const int T = sg.rows, tid = threadIdx.x;
    const int per = (T + 255) / 256;
    const int p0 = tid * per < T ? tid * per : T, p1 = p0 + per < T ? p0 + per : T;
    int pre = 0, cur = 0, best = 0, pos = p0;
    bool lead = true;
    for (int t = p0; t < p1; t++)
    {
        if (eq[sg.row0 + t])
        {
            cur++;
            if (lead) pre = cur;
            if (cur > best) { best = cur; pos = t - cur + 1; }
        }
        else
        {
            cur = 0;
            lead = false;
        }
    }
    s_pre[tid] = pre;
    s_suf[tid] = cur;
    s_len[tid] = best;
    s_pos[tid] = pos;
    __syncthreads();
    if (tid != 0) return;
    // the chunks in order: `run` ones end at the current chunk boundary and began at run_pos; strict > keeps the first longest
    int run = 0, run_pos = 0, len = 0, at = 0;
    for (int k = 0; k < 256; k++)
    {
        const int q0 = k * per < T ? k * per : T, n = (q0 + per < T ? q0 + per : T) - q0;
        if (n <= 0) break;
        if (run == 0) run_pos = q0;
        if (s_pre[k] == n)
            run += n;
        else
        {
            if (run + s_pre[k] > len) { len = run + s_pre[k]; at = run_pos; }
            if (s_len[k] > len) { len = s_len[k]; at = s_pos[k]; }
            run = s_suf[k];
            run_pos = q0 + n - run;
        }
        if (run > len) { len = run; at = run_pos; }
    }
    // `len` flags from `at` on = the rows [at - 1, at + len) are equal
    const int a = at - 1, b = at + len, Rmin = 2 * H + 1;
    const bool take = len > 0 && b - a >= Rmin + VOC_RUN_MARGIN;
    const int shift = take ? b - a - Rmin : 0;
    *(int4 *)(runs + blockIdx.x) = make_int4(sg.row0, T - shift, take ? a + H : T, shift);
}

// dst rows [0, split + H + 1) = the segment's own, dst rows behind them = the source rows `shift` further on
__global__ __launch_bounds__(256) void voc_run_compact_kernel(const uint32_t *__restrict__ mel, uint32_t *__restrict__ dst, int M, const Seg *__restrict__ runs, int H)
{
    const int4 e = *(const int4 *)(runs + blockIdx.y);
    const int row0 = __builtin_amdgcn_readfirstlane(e.x), rows = __builtin_amdgcn_readfirstlane(e.y);
    const int split = __builtin_amdgcn_readfirstlane(e.z), shift = __builtin_amdgcn_readfirstlane(e.w);
    const long n = (long)rows * M, keep = (long)(split + H + 1) * M;
    const size_t base = (size_t)row0 * M;
#pragma unroll
    for (int k = 0; k < 4; k++)
    {
        const long i = (long)blockIdx.x * 1024 + k * 256 + threadIdx.x;
        if (i < n) dst[base + i] = mel[base + i + (i >= keep ? (long)shift * M : 0)];
    }
}

hipError_t launch_voc_runs(hipStream_t s, const float *mel, int M, float *mel_c, int32_t *eq, Seg *runs, const Segs &frames, int H)
{
    if (frames.nseg < 1 || frames.max_rows < 1 || M < 1 || H < 0 || !mel || !mel_c || !eq || !runs) return hipErrorInvalidValue;
    hipLaunchKernelGGL(voc_run_flags_kernel, dim3((frames.max_rows + 3) / 4, frames.nseg), dim3(256), 0, s, (const uint32_t *)mel, M, eq, frames);
    hipLaunchKernelGGL(voc_run_scan_kernel, dim3(frames.nseg), dim3(256), 0, s, eq, runs, frames, H);
    const long per_seg = (long)frames.max_rows * M;
    hipLaunchKernelGGL(voc_run_compact_kernel, dim3((unsigned)((per_seg + 1023) / 1024), frames.nseg), dim3(256), 0, s,
                       (const uint32_t *)mel, (uint32_t *)mel_c, M, runs, H);
    return hipGetLastError();
}

// wav frames (split, split + shift] of every segment = copies of frame `split` (x: `rate` samples per frame): the frames the
// run-shortened schedule did not vocode.  grid.x walks the longest possible fill in chunks of 1 024 samples.
__global__ __launch_bounds__(256) void voc_run_fill_kernel(float *__restrict__ x, const Seg *__restrict__ runs, int rate)
{
    const int4 e = *(const int4 *)(runs + blockIdx.y);
    const int row0 = __builtin_amdgcn_readfirstlane(e.x), split = __builtin_amdgcn_readfirstlane(e.z);
    const int shift = __builtin_amdgcn_readfirstlane(e.w);
    const long n = (long)shift * rate, i0 = (long)blockIdx.x * 1024;
    if (i0 >= n) return;
    const float *src = x + (size_t)(row0 + split) * rate;
    float *dst = x + (size_t)(row0 + split + 1) * rate;
#pragma unroll
    for (int k = 0; k < 4; k++)
    {
        const long i = i0 + k * 256 + threadIdx.x;
        if (i < n) dst[i] = src[i % rate];
    }
}

hipError_t launch_voc_run_fill(hipStream_t s, float *x, const Segs &runs, int rate)
{
    if (runs.nseg < 1 || runs.max_rows < 1 || rate < 1 || !runs.tab || !x) return hipErrorInvalidValue;
    const long per_seg = (long)runs.max_rows * rate;
    hipLaunchKernelGGL(voc_run_fill_kernel, dim3((unsigned)((per_seg + 1023) / 1024), runs.nseg), dim3(256), 0, s, x, runs.tab, rate);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------
// Run-shortened decoding (kernels.h: launch_dec_runs, dec_runs.h).  The table: one thread per segment, from the regulator's counts.
// ONE wave walks the segments 64 at a time.  packed (dec_runs.h "densely packed decoding"): row0 is the start of the segment's slot
// in the packed row space — the wave's running sum of the slots in front of it — and entry nseg is the packed space as one segment
__global__ __launch_bounds__(64) void dec_runs_kernel(const int32_t *__restrict__ n_frames, Seg *__restrict__ runs, const Segs frames, int R,
                                                      int packed)
{
    const int lane = threadIdx.x;
    int done = 0;                                   // packed rows in front of this round's segments (the same in every lane)
    for (int u0 = 0; u0 < frames.nseg; u0 += 64)
    {
        const int u = u0 + lane;
        const bool live = u < frames.nseg;
        const Seg cap = frames.tab ? frames.tab[live ? u : 0] : frames.one;
        const DecRun r = dec_run(live ? n_frames[u] : 0, cap.rows, R);
        const int slot = live && packed ? dec_pack_slot(r.rows_c) : 0;
        int incl = slot;                            // inclusive scan of the slots over the wave
#pragma unroll
        for (int o = 1; o < 64; o <<= 1)
        {
            const int v = __shfl_up(incl, o, 64);
            if (lane >= o) incl += v;
        }
        if (live) *(int4 *)(runs + u) = make_int4(packed ? done + incl - slot : cap.row0, r.rows_c, r.gap_at, r.G);
        done += __shfl(incl, 63, 64);
    }
    if (packed && lane == 0) *(int4 *)(runs + frames.nseg) = make_int4(0, done, 0, 0);
}

hipError_t launch_dec_runs(hipStream_t s, const int32_t *n_frames, Seg *runs, const Segs &frames, int R, int packed)
{
    if (frames.nseg < 1 || !n_frames || !runs || R < 0 || (!frames.tab && frames.nseg != 1)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(dec_runs_kernel, dim3(1), dim3(64), 0, s, n_frames, runs, frames, R, packed);
    return hipGetLastError();
}

// densely packed decoding: rows [0, rows_c) of every segment from the capacity layout (`frames`) into the segment's slot of the
// packed layout (`runs`: row0 = the slot's first row), zeros in the slot's guard rows.  C floats per row, a multiple of 4; grid.x
// walks a slot in chunks of 1 024 float4
__global__ __launch_bounds__(256) void dec_pack_rows_kernel(const float4 *__restrict__ src, float4 *__restrict__ dst, int C4,
                                                            const Seg *__restrict__ runs, const Segs frames)
{
    const Seg cap = seg_at(frames, blockIdx.y);
    const int4 e = *(const int4 *)(runs + blockIdx.y);
    const int row0_p = __builtin_amdgcn_readfirstlane(e.x), rows_c = __builtin_amdgcn_readfirstlane(e.y);
    const long n = (long)dec_pack_slot(rows_c) * C4, live = (long)rows_c * C4;
    const float4 *sp = src + (size_t)cap.row0 * C4;
    float4 *dp = dst + (size_t)row0_p * C4;
#pragma unroll
    for (int k = 0; k < 4; k++)
    {
        const long i = (long)blockIdx.x * 1024 + k * 256 + threadIdx.x;
        if (i >= n) continue;
        dp[i] = i < live ? sp[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

hipError_t launch_dec_pack_rows(hipStream_t s, const float *x, float *xp, int C, const Segs &runs, const Segs &frames)
{
    if (frames.nseg < 1 || frames.nseg != runs.nseg || frames.max_rows < 1 || C < 4 || (C & 3) || !runs.tab || !x || !xp) return hipErrorInvalidValue;
    const long per_slot = (long)dec_pack_slot(frames.max_rows) * (C / 4);
    hipLaunchKernelGGL(dec_pack_rows_kernel, dim3((unsigned)((per_slot + 1023) / 1024), frames.nseg), dim3(256), 0, s, (const float4 *)x,
                       (float4 *)xp, C / 4, runs.tab, frames);
    return hipGetLastError();
}

// every row of a segment's capacity from the compact row that holds its value; grid.x walks the capacity in chunks of 1 024 elements
__global__ __launch_bounds__(256) void dec_run_expand_kernel(const float *__restrict__ src, float *__restrict__ dst, int M,
                                                             const Seg *__restrict__ runs, const Segs frames)
{
    const Seg cap = seg_at(frames, blockIdx.y);
    const int4 e = *(const int4 *)(runs + blockIdx.y);
    const int rows_c = __builtin_amdgcn_readfirstlane(e.y), gap_at = __builtin_amdgcn_readfirstlane(e.z), G = __builtin_amdgcn_readfirstlane(e.w);
    const long n = (long)cap.rows * M;
    // (the compact rows begin where the run table says: at the capacity's own row0, or at the slot of densely packed decoding)
    const size_t base = (size_t)cap.row0 * M, cbase = (size_t)__builtin_amdgcn_readfirstlane(e.x) * M;
#pragma unroll
    for (int k = 0; k < 4; k++)
    {
        const long i = (long)blockIdx.x * 1024 + k * 256 + threadIdx.x;
        if (i >= n) continue;
        const int t = (int)(i / M), c = (int)(i - (long)t * M);
        const int tc = dec_run_compact_row(t, gap_at, G);
        if (tc < rows_c) dst[base + i] = src[cbase + (size_t)tc * M + c];
    }
}

hipError_t launch_dec_run_expand(hipStream_t s, const float *mel_c, float *mel, int M, const Segs &runs, const Segs &frames)
{
    if (frames.nseg < 1 || frames.nseg != runs.nseg || frames.max_rows < 1 || M < 1 || !runs.tab || !mel_c || !mel) return hipErrorInvalidValue;
    const long per_seg = (long)frames.max_rows * M;
    hipLaunchKernelGGL(dec_run_expand_kernel, dim3((unsigned)((per_seg + 1023) / 1024), frames.nseg), dim3(256), 0, s, mel_c, mel, M,
                       runs.tab, frames);
    return hipGetLastError();
}

}  // namespace zv
