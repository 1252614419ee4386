// level_kernels.hip — volume controls: the level meter's two passes over a finished waveform (level_measure, level_apply; the
// arithmetic: level.h).  A part of misc_kernels.hip's unit.
#include "kernels.h"
#include "level.h"
#include "wave_sum.h"

namespace zv
{

// ---------------------------------------------------------------------------------------------------
// Volume controls (kernels.h: launch_level_measure / launch_level_apply; the rule: level.h).  Two passes over the finished waveform,
// grid (chunks of LEVEL_CHUNK_SAMPLES samples, segments):
//   measure: workgroup (c, u) adds the squared 1.19 magnitudes and takes the peak of the SPEECH samples of its chunk (i < nf * hop,
//            nf from the device frame counts) and stores {S, peak bits, 0} into slab[u][c] with one 16-byte store; a chunk behind the
//            speech stores nothing
//   apply:   workgroup (c, u) adds slab[u][0 .. chunks of the speech) — integers, so every workgroup of a segment gets the same
//            totals — computes the gain (level_report) and scales chunk c of the segment's CAPACITY; workgroup (0, u) stores the
//            segment's LevelRow
// No atomics and nothing to zero: every slab entry apply reads was stored by measure in the same run, so a graph replay on
// poisoned buffers changes nothing.  A segment's first sample sits at row0 * hop floats behind a 256-byte aligned base, a chunk at a
// multiple of 4 samples behind it: 16-byte loads whenever row0 * hop is a multiple of 4 (any row0 at a hop that is one); the
// workgroup falls back to 4-byte accesses otherwise and for the last samples of a length that is no multiple of 4.
constexpr int LEVEL_SWEEPS = (LEVEL_CHUNK_SAMPLES + 1023) / 1024;      // 16-byte loads a lane issues for a whole chunk

__device__ __forceinline__ void level_block_totals(unsigned long long &S, uint32_t &peak, unsigned long long *red_s, uint32_t *red_p)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
    {
        S += (unsigned long long)__shfl_xor((long long)S, o, 64);
        const uint32_t p = (uint32_t)__shfl_xor((int)peak, o, 64);
        peak = p > peak ? p : peak;
    }
    if ((threadIdx.x & 63) == 0)
    {
        red_s[threadIdx.x >> 6] = S;
        red_p[threadIdx.x >> 6] = peak;
    }
    __syncthreads();
    S = (red_s[0] + red_s[1]) + (red_s[2] + red_s[3]);
    const uint32_t pa = red_p[0] > red_p[1] ? red_p[0] : red_p[1], pb = red_p[2] > red_p[3] ? red_p[2] : red_p[3];
    peak = pa > pb ? pa : pb;
}

// the frames of segment u that hold speech: the regulator's count, inside [0, capacity]
__device__ __forceinline__ int level_speech_frames(const int32_t *__restrict__ n_frames, int u, int cap_rows)
{
    const int nf = __builtin_amdgcn_readfirstlane(n_frames[u]);
    return nf < 0 ? 0 : (nf < cap_rows ? nf : cap_rows);
}

__global__ __launch_bounds__(256) void level_measure_kernel(const float *__restrict__ wav, const int32_t *__restrict__ n_frames,
                                                            uint4 *__restrict__ slab, int slab_seg, const Segs frames, int hop)
{
    __shared__ unsigned long long red_s[4];
    __shared__ uint32_t red_p[4];
    const int u = blockIdx.y;
    const Seg cap = seg_at(frames, u);
    const long n = (long)level_speech_frames(n_frames, u, cap.rows) * hop;
    const long i0 = (long)blockIdx.x * LEVEL_CHUNK_SAMPLES;
    if (i0 >= n) return;
    const float *xs = wav + (size_t)cap.row0 * hop + i0;
    const int len = (int)(n - i0 < LEVEL_CHUNK_SAMPLES ? n - i0 : LEVEL_CHUNK_SAMPLES);
    const bool vec = ((uintptr_t)xs & 15) == 0;
    unsigned long long S = 0;
    uint32_t peak = 0;
    auto take = [&](float v) {
        const unsigned long long q = level_quant(v);
        S += q * q;
        const uint32_t a = level_abs_bits(v);
        peak = a > peak ? a : peak;
    };
    if (vec)
    {
        // all of a lane's 16-byte loads are issued before the first is used (a zero adds nothing to either total)
        float4 q[LEVEL_SWEEPS];
#pragma unroll
        for (int k = 0; k < LEVEL_SWEEPS; k++)
        {
            const int i = k * 1024 + threadIdx.x * 4;
            q[k] = i + 4 <= len ? *(const float4 *)(xs + i) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int k = 0; k < LEVEL_SWEEPS; k++)
        {
            take(q[k].x);
            take(q[k].y);
            take(q[k].z);
            take(q[k].w);
        }
        const int i = (len & ~3) + threadIdx.x;          // the last samples of a length that is no multiple of 4
        if (threadIdx.x < 3 && i < len) take(xs[i]);
    }
    else
        for (int i = threadIdx.x; i < len; i += 256) take(xs[i]);
    level_block_totals(S, peak, red_s, red_p);
    if (threadIdx.x == 0) slab[(size_t)u * slab_seg + blockIdx.x] = make_uint4((uint32_t)S, (uint32_t)(S >> 32), peak, 0u);
}

__global__ __launch_bounds__(256) void level_apply_kernel(float *__restrict__ wav, const int32_t *__restrict__ n_frames,
                                                          const uint4 *__restrict__ slab, int slab_seg, const float *__restrict__ vol,
                                                          LevelRow *__restrict__ levels, const Segs frames, int hop)
{
    __shared__ unsigned long long red_s[4];
    __shared__ uint32_t red_p[4];
    const int u = blockIdx.y;
    const Seg cap = seg_at(frames, u);
    const long total = (long)cap.rows * hop;
    const long i0 = (long)blockIdx.x * LEVEL_CHUNK_SAMPLES;
    if (i0 >= total) return;
    // the chunk's 16-byte loads are issued first: they travel while the segment's totals are added up and the gain is computed
    float *xs = wav + (size_t)cap.row0 * hop + i0;
    const int len = (int)(total - i0 < LEVEL_CHUNK_SAMPLES ? total - i0 : LEVEL_CHUNK_SAMPLES);
    const bool vec = ((uintptr_t)xs & 15) == 0;
    float4 q[LEVEL_SWEEPS];
#pragma unroll
    for (int k = 0; k < LEVEL_SWEEPS; k++)
    {
        const int i = k * 1024 + threadIdx.x * 4;
        if (vec && i + 4 <= len) q[k] = *(const float4 *)(xs + i);
    }
    const long n = (long)level_speech_frames(n_frames, u, cap.rows) * hop;
    long nch = (n + LEVEL_CHUNK_SAMPLES - 1) / LEVEL_CHUNK_SAMPLES;
    nch = nch < slab_seg ? nch : slab_seg;
    unsigned long long S = 0;
    uint32_t peak = 0;
    for (int c = threadIdx.x; c < (int)nch; c += 256)
    {
        const uint4 e = slab[(size_t)u * slab_seg + c];
        S += (unsigned long long)e.x | ((unsigned long long)e.y << 32);
        peak = e.z > peak ? e.z : peak;
    }
    level_block_totals(S, peak, red_s, red_p);
    const float *vr = vol + (size_t)u * LEVEL_VOL_STRIDE;
    const LevelRow r = level_report(S, (uint64_t)n, peak, vr[0], vr[1], vr[2]);
    if (blockIdx.x == 0 && threadIdx.x == 0) *(uint4 *)(levels + u) = make_uint4(level_bits(r.rms), level_bits(r.peak), level_bits(r.gain), 0u);
    const float g = r.gain;
    if (vec)
    {
#pragma unroll
        for (int k = 0; k < LEVEL_SWEEPS; k++)
        {
            const int i = k * 1024 + threadIdx.x * 4;
            if (i + 4 <= len) *(float4 *)(xs + i) = make_float4(q[k].x * g, q[k].y * g, q[k].z * g, q[k].w * g);
        }
        const int i = (len & ~3) + threadIdx.x;
        if (threadIdx.x < 3 && i < len) xs[i] = xs[i] * g;
    }
    else
        for (int i = threadIdx.x; i < len; i += 256) xs[i] = xs[i] * g;
}

int level_chunks(int max_rows, int hop) { return (int)(((long)max_rows * hop + LEVEL_CHUNK_SAMPLES - 1) / LEVEL_CHUNK_SAMPLES); }

hipError_t launch_level_measure(hipStream_t s, const float *wav, const int32_t *n_frames, void *slab, const Segs &frames, int hop)
{
    if (frames.nseg < 1 || frames.max_rows < 1 || hop < 1 || !wav || !n_frames || !slab || ((uintptr_t)slab & 15) || (!frames.tab && frames.nseg != 1))
        return hipErrorInvalidValue;
    const int chunks = level_chunks(frames.max_rows, hop);
    hipLaunchKernelGGL(level_measure_kernel, dim3(chunks, frames.nseg), dim3(256), 0, s, wav, n_frames, (uint4 *)slab, chunks, frames, hop);
    return hipGetLastError();
}

hipError_t launch_level_apply(hipStream_t s, float *wav, const int32_t *n_frames, const void *slab, const float *vol, LevelRow *levels,
                              const Segs &frames, int hop)
{
    if (frames.nseg < 1 || frames.max_rows < 1 || hop < 1 || !wav || !n_frames || !slab || ((uintptr_t)slab & 15) || !vol || !levels ||
        ((uintptr_t)levels & 15) || (!frames.tab && frames.nseg != 1))
        return hipErrorInvalidValue;
    const int chunks = level_chunks(frames.max_rows, hop);
    hipLaunchKernelGGL(level_apply_kernel, dim3(chunks, frames.nseg), dim3(256), 0, s, wav, n_frames, (const uint4 *)slab, chunks, vol, levels,
                       frames, hop);
    return hipGetLastError();
}

}  // namespace zv
