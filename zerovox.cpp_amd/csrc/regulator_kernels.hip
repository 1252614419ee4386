// regulator_kernels.hip — the length regulator on the device (lr_scan, lr_gather, lr_gather16, lr_fused16: launch_length_regulator
// launches what stage_plan.h plans), target durations (fit_durations) and fitted mode's frame table (live_frames, zero_tail).
// A part of misc_kernels.hip's unit.
#include "kernels.h"
#include "fit_durations.h"
#include "stage_plan.h"

namespace zv
{

// ---------------------------------------------------------------------------------------------------
// Length regulator on the device (the reference does it on the host, src/fs2encoder.cpp:611-654):
//   dur_i = (int)((float)(exp(logdur_i) - 1.0) + 0.5) for the first num_phonemes (= aux) tokens of the utterance;
//   frame f belongs to the token whose cumulative duration first exceeds f; frames past the total (or past T) are zero.
//   ctl (or null): the (float) duration is multiplied by ctl[seg][CTL_DURATION] before it is rounded (prosody control).
//   pctl (or null): then by pctl[row][PCTL_DURATION]; after rounding and clamping, pctl[row][PCTL_FRAMES] >= 0 replaces the
//   duration by min(frames, T) (per-phoneme control; row = the token's absolute row).
__global__ __launch_bounds__(1024) void lr_scan_kernel(const float *__restrict__ logdur, int32_t *__restrict__ cum,
                                                       int32_t *__restrict__ n_frames, const Segs tokens, const Segs frames,
                                                       const float *__restrict__ ctl, const float *__restrict__ pctl)
{
    __shared__ int buf[1024];
    const Seg tk = seg_at(tokens, blockIdx.x), fr = seg_at(frames, blockIdx.x);
    const int n = tk.rows, T = fr.rows;
    if (n <= 0) return;
    const int nwalk = tk.aux < n ? tk.aux : n;
    const float *ld_ = logdur + tk.row0;
    int32_t *cm = cum + tk.row0;
    const int tid = threadIdx.x;
    const float dscale = ctl ? ctl[(size_t)blockIdx.x * CTL_STRIDE + CTL_DURATION] : 1.f;
    int carry = 0;
    for (int base = 0; base < n; base += 1024)
    {
        const int i = base + tid;
        int d = 0;
        if (i < nwalk)
        {
            float dur = (float)(exp((double)ld_[i]) - 1.0);
            if (ctl) dur = dur * dscale;
            const float *pr = pctl ? pctl + ((size_t)tk.row0 + i) * PCTL_STRIDE : nullptr;
            if (pctl) dur = dur * pr[PCTL_DURATION];
            d = (int)((double)dur + 0.5);
            if (d < 0) d = 0;
            if (d > T) d = T;          // keeps the running sum far from int overflow; frames stop at T anyway
            if (pctl && pr[PCTL_FRAMES] >= 0.f)
            {
                const int forced = (int)pr[PCTL_FRAMES];
                d = forced < T ? forced : T;
            }
        }
        buf[tid] = d;
        __syncthreads();
        for (int o = 1; o < 1024; o <<= 1)
        {
            const int v = (tid >= o) ? buf[tid - o] : 0;
            __syncthreads();
            buf[tid] += v;
            __syncthreads();
        }
        if (i < n) cm[i] = carry + buf[tid];
        carry += buf[1023];
        __syncthreads();
    }
    if (tid == 0) n_frames[blockIdx.x] = carry < T ? carry : T;
}

__global__ void lr_gather_kernel(const float *__restrict__ feat, int ld, const int32_t *__restrict__ cum, int C,
                                 float *__restrict__ hidden, int ldh, const Segs tokens, const Segs frames)
{
    const Seg tk = seg_at(tokens, blockIdx.y), fr = seg_at(frames, blockIdx.y);
    const int f = blockIdx.x;
    if (f >= fr.rows) return;
    const int n = tk.rows;
    const int32_t *cm = cum + tk.row0;
    // first token i with cum[i] > f
    int lo = 0, hi = n;
    while (lo < hi)
    {
        const int mid = (lo + hi) >> 1;
        if (cm[mid] > f) hi = mid; else lo = mid + 1;
    }
    const bool live = lo < n;
    const float *src = feat + ((size_t)tk.row0 + lo) * ld;
    float *dst = hidden + ((size_t)fr.row0 + f) * ldh;
    for (int c = threadIdx.x; c < C; c += blockDim.x) dst[c] = live ? src[c] : 0.f;
}

// the same gather, 16 frames per workgroup: the utterance's cumulative durations are read into LDS once (coalesced) and searched
// there — the kernel above walks them in global memory, eight dependent round trips per frame — and the rows move in 16-byte pieces
__global__ __launch_bounds__(256) void lr_gather16_kernel(const float *__restrict__ feat, int ld, const int32_t *__restrict__ cum, int C,
                                                          float *__restrict__ hidden, int ldh, const Segs tokens, const Segs frames)
{
    extern __shared__ int32_t lr_cs[];
    const Seg tk = seg_at(tokens, blockIdx.y), fr = seg_at(frames, blockIdx.y);
    const int f0 = blockIdx.x * 16;
    if (f0 >= fr.rows) return;
    const int n = tk.rows;
    for (int i = threadIdx.x; i < n; i += 256) lr_cs[i] = cum[tk.row0 + i];
    __syncthreads();
    const int f = f0 + (threadIdx.x >> 4), l16 = threadIdx.x & 15;
    if (f >= fr.rows) return;
    int lo = 0, hi = n;                  // first token i with cum[i] > f
    while (lo < hi)
    {
        const int mid = (lo + hi) >> 1;
        if (lr_cs[mid] > f) hi = mid; else lo = mid + 1;
    }
    const bool live = lo < n;
    const float4 *src = (const float4 *)(feat + ((size_t)tk.row0 + (live ? lo : 0)) * ld);
    float4 *dst = (float4 *)(hidden + ((size_t)fr.row0 + f) * ldh);
    for (int c4 = l16; c4 < (C >> 2); c4 += 16)
    {
        const float4 v = src[c4];
        dst[c4] = live ? v : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

// Scan and gather in ONE launch for utterances of at most 1 024 tokens: every workgroup (16 frames) recomputes its utterance's
// rounded durations and their inclusive scan in LDS — a few hundred integer operations against a launch boundary — and the first
// workgroup of a segment also stores the scan (the `cum` tap) and the frame count, even for a segment without frames (the phoneme
// timings are read from `cum`).  Integer sums: any scan order, the same values.  ctl / pctl: lr_scan_kernel's controls.
__global__ __launch_bounds__(256) void lr_fused16_kernel(const float *__restrict__ feat, int ld, const float *__restrict__ logdur, int C,
                                                         float *__restrict__ hidden, int ldh, int32_t *__restrict__ cum,
                                                         int32_t *__restrict__ n_frames, const Segs tokens, const Segs frames,
                                                         const float *__restrict__ ctl, const float *__restrict__ pctl)
{
    __shared__ int32_t lr_cs[1024];
    __shared__ int32_t lr_part[256];
    const Seg tk = seg_at(tokens, blockIdx.y), fr = seg_at(frames, blockIdx.y);
    const int f0 = blockIdx.x * 16;
    const int n = tk.rows, T = fr.rows;
    if (f0 >= T && blockIdx.x != 0) return;      // workgroup 0 stores cum / n_frames whatever T is
    const int nwalk = tk.aux < n ? tk.aux : n;
    const int tid = threadIdx.x;
    const float dscale = ctl ? ctl[(size_t)blockIdx.y * CTL_STRIDE + CTL_DURATION] : 1.f;
    // four consecutive tokens per thread: durations (lr_scan_kernel's arithmetic), their running sums, the thread's total
    int d[4], tot = 0;
#pragma unroll
    for (int j = 0; j < 4; j++)
    {
        const int i = tid * 4 + j;
        int v = 0;
        if (i < nwalk)
        {
            float dur = (float)(exp((double)logdur[tk.row0 + i]) - 1.0);
            if (ctl) dur = dur * dscale;
            const float *pr = pctl ? pctl + ((size_t)tk.row0 + i) * PCTL_STRIDE : nullptr;
            if (pctl) dur = dur * pr[PCTL_DURATION];
            v = (int)((double)dur + 0.5);
            if (v < 0) v = 0;
            if (v > T) v = T;
            if (pctl && pr[PCTL_FRAMES] >= 0.f)
            {
                const int forced = (int)pr[PCTL_FRAMES];
                v = forced < T ? forced : T;
            }
        }
        tot += v;
        d[j] = tot;
    }
    lr_part[tid] = tot;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1)
    {
        const int v = tid >= o ? lr_part[tid - o] : 0;
        __syncthreads();
        lr_part[tid] += v;
        __syncthreads();
    }
    const int base = tid ? lr_part[tid - 1] : 0;
#pragma unroll
    for (int j = 0; j < 4; j++) lr_cs[tid * 4 + j] = base + d[j];
    __syncthreads();
    if (blockIdx.x == 0)
    {
        for (int i = tid; i < n; i += 256) cum[tk.row0 + i] = lr_cs[i];
        if (tid == 0)
        {
            const int total = lr_part[255];
            n_frames[blockIdx.y] = total < T ? total : T;
        }
    }
    const int f = f0 + (tid >> 4), l16 = tid & 15;
    if (f >= T) return;
    int lo = 0, hi = n;                  // first token i with cum[i] > f
    while (lo < hi)
    {
        const int mid = (lo + hi) >> 1;
        if (lr_cs[mid] > f) hi = mid; else lo = mid + 1;
    }
    const bool live = lo < n;
    const float4 *src = (const float4 *)(feat + ((size_t)tk.row0 + (live ? lo : 0)) * ld);
    float4 *dst = (float4 *)(hidden + ((size_t)fr.row0 + f) * ldh);
    for (int c4 = l16; c4 < (C >> 2); c4 += 16)
    {
        const float4 v = src[c4];
        dst[c4] = live ? v : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

hipError_t launch_length_regulator(hipStream_t s, const float *feat, int ld, const float *logdur, int C, float *hidden,
                                   int ldh, int32_t *cum, int32_t *n_frames, const Segs &tokens, const Segs &frames, const float *ctl,
                                   const float *pctl)
{
    if (tokens.nseg != frames.nseg || tokens.nseg < 1) return hipErrorInvalidValue;
    const LrPlan p = lr_plan(C, ld, ldh, tokens.max_rows, frames.max_rows, frames.nseg);
    const dim3 grid(p.gx, p.gy);
    if (p.form == LR_FUSED)
    {
        hipLaunchKernelGGL(lr_fused16_kernel, grid, dim3(256), 0, s, feat, ld, logdur, C, hidden, ldh, cum, n_frames, tokens, frames, ctl, pctl);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(lr_scan_kernel, dim3(p.scan_gx), dim3(1024), 0, s, logdur, cum, n_frames, tokens, frames, ctl, pctl);
    if (p.form == LR_SCAN_GATHER16)
        hipLaunchKernelGGL(lr_gather16_kernel, grid, dim3(256), p.lds, s, feat, ld, cum, C, hidden, ldh, tokens, frames);
    else
        hipLaunchKernelGGL(lr_gather_kernel, grid, dim3(256), 0, s, feat, ld, cum, C, hidden, ldh, tokens, frames);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------
// Target durations (include/zerovox_amd.h "target durations", the rule: fit_durations.h): between the duration predictor and the
// length regulator.  One workgroup per utterance; a segment whose ctl row holds no target (CTL_TARGET <= 0) returns at once and
// leaves its rows alone.  Otherwise the durations d_i that sum to the target are stored as FORCED frame counts in the PCTL_FRAMES
// column of the utterance's pctl rows, where the regulator kernels read them as they read a caller's duration_frames: those
// kernels do not change.  The rows are uploaded at the head of every run, so a replay starts from the caller's values again.
//   pass 1: forced phonemes add min(frames, T) to Fs, free ones get their weight q (lr_scan_kernel's f32 duration, fit_weight)
//   pass 2: share and remainder of every free phoneme (64-bit integers from here on); L = R - sum of the shares
//   pass 3: free phoneme i gets one frame more when fewer than L free phonemes come before it (largest remainder, then lower
//           index): counted over the LDS-resident remainders, broadcast reads, n^2 compares (2.3 M at 1 501 phonemes)
// Sums are integer sums over the workgroup: any order, the same values.  Tokens at or past num_phonemes (aux) are left alone: the
// regulator gives them 0 whatever their row says.
__device__ __forceinline__ long long fit_block_sum(long long v, long long *red)
{
    const int tid = threadIdx.x;
    __syncthreads();                         // the previous sum's red[0] has been read by everyone
    red[tid] = v;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1)
    {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    return red[0];
}

__global__ __launch_bounds__(1024) void fit_durations_kernel(const float *__restrict__ logdur, const float *__restrict__ ctl,
                                                             float *__restrict__ pctl, const Segs tokens, const Segs frames)
{
    extern __shared__ long long fit_lds[];   // [max_rows] weight, then share (-1: not free), [max_rows] remainder (-1: not free)
    __shared__ long long red[1024];
    const Seg tk = seg_at(tokens, blockIdx.x), fr = seg_at(frames, blockIdx.x);
    const float *cv = ctl + (size_t)blockIdx.x * CTL_STRIDE;
    const int target = (int)cv[CTL_TARGET];
    const int n = tk.rows < tokens.max_rows ? tk.rows : tokens.max_rows, T = fr.rows;      // (the LDS arrays hold max_rows entries)
    if (target <= 0 || n <= 0) return;
    const int nwalk = tk.aux < n ? tk.aux : n;
    const int tid = threadIdx.x;
    long long *qs = fit_lds, *rs = fit_lds + tokens.max_rows;
    float *rows = pctl + (size_t)tk.row0 * PCTL_STRIDE;
    const float *ld_ = logdur + tk.row0;
    const float dscale = cv[CTL_DURATION];
    long long Fs = 0, Q = 0, n_free = 0;
    for (int i = tid; i < nwalk; i += 1024)
    {
        const float *pr = rows + (size_t)i * PCTL_STRIDE;
        const float f = pr[PCTL_FRAMES];
        long long q = -1;
        if (f >= 0.f)
        {
            const int forced = (int)f;
            Fs += forced < T ? forced : T;
        }
        else
        {
            float dur = (float)(exp((double)ld_[i]) - 1.0);
            dur = dur * dscale;
            dur = dur * pr[PCTL_DURATION];
            q = fit_weight(dur);
            Q += q;
            n_free++;
        }
        qs[i] = q;
    }
    Fs = fit_block_sum(Fs, red);
    Q = fit_block_sum(Q, red);
    n_free = fit_block_sum(n_free, red);
    const long long R = (long long)target - Fs;
    if (R <= 0 || n_free == 0)               // forced durations win: every free phoneme gets 0
    {
        for (int i = tid; i < nwalk; i += 1024)
            if (qs[i] >= 0) rows[(size_t)i * PCTL_STRIDE + PCTL_FRAMES] = 0.f;
        return;
    }
    const bool equal = Q == 0;               // no weight at all: equal shares
    if (equal) Q = n_free;
    long long shares = 0;
    for (int i = tid; i < nwalk; i += 1024)
    {
        const long long q = equal ? 1 : qs[i];
        const bool is_free = qs[i] >= 0;
        const long long base = is_free ? fit_share(q, R, Q) : -1;
        rs[i] = is_free ? fit_remainder(q, R, Q) : -1;
        qs[i] = base;
        if (is_free) shares += base;
    }
    const long long L = R - fit_block_sum(shares, red);       // (its barriers also publish rs[])
    for (int i = tid; i < nwalk; i += 1024)
    {
        const long long ri = rs[i];
        if (ri < 0) continue;
        long long before = 0;
        if (L > 0)
            for (int j = 0; j < nwalk; j++) before += fit_before(rs[j], j, ri, i) ? 1 : 0;      // (a forced j holds -1: never before)
        const long long d = qs[i] + (before < L ? 1 : 0);
        rows[(size_t)i * PCTL_STRIDE + PCTL_FRAMES] = (float)d;
    }
}

hipError_t launch_fit_durations(hipStream_t s, const float *logdur, const float *ctl, const float *pctl, const Segs &tokens,
                                const Segs &frames)
{
    if (!logdur || !ctl || !pctl || tokens.nseg != frames.nseg || tokens.nseg < 1 || tokens.max_rows < 1) return hipErrorInvalidValue;
    if (tokens.max_rows > FIT_MAX_TOKENS) return hipErrorInvalidValue;
    const size_t lds = (size_t)tokens.max_rows * 2 * sizeof(long long);
    // the rows are the caller's controls and read-only to every other kernel; this one rewrites their PCTL_FRAMES column in place
    hipLaunchKernelGGL(fit_durations_kernel, dim3(tokens.nseg), dim3(1024), lds, s, logdur, ctl, const_cast<float *>(pctl), tokens, frames);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------
// Fitted mode: the frame table the decoder and the vocoder read, written on the device from the length regulator's frame counts.
//   live[u] = {frames[u].row0, min(n_frames[u], frames[u].rows), 0, 0}
// row0 stays the capacity table's (buffers are laid out by capacity, so every output stays where the host expects it); a segment
// whose regulator produced no frame gets rows = 0, and every frame-rate kernel then leaves it alone (its workgroups exit on
// `t0 >= L`, the statistics kernels on `L <= 0`).  One thread per segment, HBM tables in and out.
__global__ __launch_bounds__(64) void live_frames_kernel(const int32_t *__restrict__ n_frames, Seg *__restrict__ live, const Segs frames)
{
    const int u = blockIdx.x * 64 + threadIdx.x;
    if (u >= frames.nseg) return;
    const Seg cap = frames.tab ? frames.tab[u] : frames.one;
    int nf = n_frames[u];
    nf = nf < 0 ? 0 : (nf < cap.rows ? nf : cap.rows);
    *(int4 *)(live + u) = make_int4(cap.row0, nf, 0, 0);
}

hipError_t launch_live_frames(hipStream_t s, const int32_t *n_frames, Seg *live, const Segs &frames)
{
    if (frames.nseg < 1 || !n_frames || !live || (!frames.tab && frames.nseg != 1)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(live_frames_kernel, dim3((frames.nseg + 63) / 64), dim3(64), 0, s, n_frames, live, frames);
    return hipGetLastError();
}

// Fitted mode: x[(row0 + t) * C + c] = 0 for the rows t in [live.rows * rate, frames.rows * rate) of every segment — the part of a
// segment's capacity that the fitted schedule never writes (the waveform behind an utterance's last frame).  grid.x walks a
// segment's capacity in chunks of 1 024 elements; a chunk that lies inside the live part exits at once.
__global__ __launch_bounds__(256) void zero_tail_kernel(float *__restrict__ x, int C, const Segs frames, const Segs live, int rate)
{
    const Seg cap = seg_at(frames, blockIdx.y), lv = seg_at(live, blockIdx.y);
    const long end = (long)cap.rows * rate * C;
    long lo = (long)(lv.rows < cap.rows ? lv.rows : cap.rows) * rate * C;
    if (lo < 0) lo = 0;
    const long i0 = (long)blockIdx.x * 1024;
    if (i0 + 1024 <= lo || i0 >= end) return;
    float *xs = x + (size_t)cap.row0 * rate * C;
#pragma unroll
    for (int k = 0; k < 4; k++)
    {
        const long i = i0 + k * 256 + threadIdx.x;
        if (i >= lo && i < end) xs[i] = 0.f;
    }
}

hipError_t launch_zero_tail(hipStream_t s, float *x, int C, const Segs &frames, const Segs &live, int rate)
{
    if (frames.nseg < 1 || frames.nseg != live.nseg || frames.max_rows < 1 || C < 1 || rate < 1 || !live.tab) return hipErrorInvalidValue;
    const long per_seg = (long)frames.max_rows * rate * C;
    hipLaunchKernelGGL(zero_tail_kernel, dim3((unsigned)((per_seg + 1023) / 1024), frames.nseg), dim3(256), 0, s, x, C, frames, live, rate);
    return hipGetLastError();
}

}  // namespace zv
