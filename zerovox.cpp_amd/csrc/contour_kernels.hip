// contour_kernels.hip — level contour: the level meter per frame and per phoneme, two passes behind the volume passes over the
// waveform the caller receives (contour_frames, contour_phonemes; the arithmetic: contour.h, level.h).  A part of misc_kernels.hip's unit.
#include "kernels.h"
#include "contour.h"
#include "level.h"

namespace zv
{

// ---------------------------------------------------------------------------------------------------
// Level contour (kernels.h: launch_contour_frames / launch_contour_phonemes; the rule: contour.h).
//   frames:   grid (chunks of CONTOUR_CHUNK_FRAMES whole frames, segments) over the CAPACITY table.  A workgroup's four waves take eight
//             frames each, a QUARTER wave per frame and two frames after each other: at hop 300 a frame is 75 16-byte loads, which fill
//             five sweeps of 16 lanes to 94 % where two sweeps of 64 lanes would be filled to 59 % — and the pass is bound by the
//             quantisation's arithmetic (level_quant: four f64 steps and a 64-bit multiply-add per sample), which empty lanes pay too.
//             The lanes add the squared 1.19 magnitudes and take the peak of their frame's samples, a butterfly over the 16 lanes makes
//             the frame's totals, one lane per frame stores slab[row0 + f] = {S lo, S hi, peak bits, 0} and, where the call downloads
//             frame rows, rows[row0 + f] = {rms, peak}.  One pass over the waveform: a lane issues the loads of both its frames before
//             it uses the first (hops up to CONTOUR_REG_HOP; a longer hop goes frame by frame over the whole wave).
//   phonemes: grid (groups of four tokens, segments), one wave per token row.  The wave takes the phoneme's frames from the regulator's
//             scan clipped to the capacity (contour_extent), adds and maximises their slab entries strided over the lanes — a forced
//             duration makes a phoneme up to 32 768 frames long — and after a shuffle reduction lane 0 stores rows[token row].  Every
//             token row of the segment is stored, a phoneme of no frames as {0, 0}.
// Both index by ABSOLUTE frame row / token row, so the segments of consecutive tail groups touch disjoint entries.  No atomics and
// nothing to zero: every slab entry the second pass reads and every row a download reads was stored in the same run, so a graph
// replay on poisoned buffers changes nothing.  Integer totals: the split over lanes cannot show in a row.
// A segment's first sample sits row0 * hop floats behind a 256-byte aligned base: with a hop that is a multiple of 4 every frame
// starts on a 16-byte boundary and holds whole 16-byte loads.  The launcher refuses any other hop (no loadable checkpoint has one).
constexpr int CONTOUR_WAVE_FRAMES = CONTOUR_CHUNK_FRAMES / 4;      // frames of one wave
constexpr int CONTOUR_FRAME_LANES = 16;                            // lanes that share a frame on the register path
constexpr int CONTOUR_ROUNDS = CONTOUR_WAVE_FRAMES / (64 / CONTOUR_FRAME_LANES);      // frames a quarter wave takes, one after the other
constexpr int CONTOUR_FRAME_LOADS = 5;                             // 16-byte loads of a lane per frame that are kept in registers
constexpr int CONTOUR_REG_HOP = CONTOUR_FRAME_LOADS * CONTOUR_FRAME_LANES * 4;      // the longest hop of the register path: 320 samples

__device__ __forceinline__ void contour_take(float4 v, unsigned long long &S, uint32_t &peak)
{
    const float x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int t = 0; t < 4; t++)
    {
        const unsigned long long q = level_quant(x[t]);
        S += q * q;
        const uint32_t a = level_abs_bits(x[t]);
        peak = a > peak ? a : peak;
    }
}

// the totals of every aligned group of W lanes, in all of its lanes
template <int W> __device__ __forceinline__ void contour_totals(unsigned long long &S, uint32_t &peak)
{
#pragma unroll
    for (int o = W / 2; o > 0; o >>= 1)
    {
        S += (unsigned long long)__shfl_xor((long long)S, o, 64);
        const uint32_t p = (uint32_t)__shfl_xor((int)peak, o, 64);
        peak = p > peak ? p : peak;
    }
}

__device__ __forceinline__ void contour_store_frame(uint4 *__restrict__ slab, ContourRow *__restrict__ rows, size_t row, unsigned long long S,
                                                    uint32_t peak, int hop)
{
    slab[row] = make_uint4((uint32_t)S, (uint32_t)(S >> 32), peak, 0u);
    if (rows)
    {
        const ContourRow r = contour_row(S, (uint64_t)hop, peak);
        *(float2 *)(rows + row) = make_float2(r.rms, r.peak);
    }
}

template <bool REG>
__global__ __launch_bounds__(256) void contour_frames_kernel(const float *__restrict__ wav, uint4 *__restrict__ slab, ContourRow *__restrict__ rows,
                                                             const Segs frames, int hop)
{
    const int u = blockIdx.y;
    const Seg cap = seg_at(frames, u);
    const int lane = threadIdx.x & 63;
    const int f0 = __builtin_amdgcn_readfirstlane(blockIdx.x * CONTOUR_CHUNK_FRAMES + (int)(threadIdx.x >> 6) * CONTOUR_WAVE_FRAMES);
    if (f0 >= cap.rows) return;                                    // the whole wave
    const int nfr = cap.rows - f0 < CONTOUR_WAVE_FRAMES ? cap.rows - f0 : CONTOUR_WAVE_FRAMES;
    const float *xs = wav + ((size_t)cap.row0 + f0) * hop;
    const int h4 = hop >> 2;                                       // 16-byte loads of a frame
    if (REG)
    {
        // quarter wave `sub` takes frames sub, 4 + sub of the wave's eight; all of a lane's 16-byte loads are issued before the first is
        // used (a zero adds nothing to either total)
        const int sub = lane / CONTOUR_FRAME_LANES, l = lane % CONTOUR_FRAME_LANES;
        float4 q[CONTOUR_ROUNDS][CONTOUR_FRAME_LOADS];
#pragma unroll
        for (int r = 0; r < CONTOUR_ROUNDS; r++)
#pragma unroll
            for (int t = 0; t < CONTOUR_FRAME_LOADS; t++)
            {
                const int k = r * (64 / CONTOUR_FRAME_LANES) + sub, j = t * CONTOUR_FRAME_LANES + l;
                q[r][t] = k < nfr && j < h4 ? *(const float4 *)(xs + (size_t)k * hop + j * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        unsigned long long S[CONTOUR_ROUNDS];
        uint32_t P[CONTOUR_ROUNDS];
#pragma unroll
        for (int r = 0; r < CONTOUR_ROUNDS; r++)
        {
            S[r] = 0;
            P[r] = 0;
#pragma unroll
            for (int t = 0; t < CONTOUR_FRAME_LOADS; t++) contour_take(q[r][t], S[r], P[r]);
        }
#pragma unroll
        for (int r = 0; r < CONTOUR_ROUNDS; r++) contour_totals<CONTOUR_FRAME_LANES>(S[r], P[r]);
        // every lane of a quarter holds both frames' totals: lane r of it stores frame r
#pragma unroll
        for (int r = 0; r < CONTOUR_ROUNDS; r++)
        {
            const int k = r * (64 / CONTOUR_FRAME_LANES) + sub;
            if (l == r && k < nfr) contour_store_frame(slab, rows, (size_t)cap.row0 + f0 + k, S[r], P[r], hop);
        }
    }
    else
        for (int k = 0; k < nfr; k++)
        {
            unsigned long long S = 0;
            uint32_t P = 0;
            for (int j = lane; j < h4; j += 64) contour_take(*(const float4 *)(xs + (size_t)k * hop + j * 4), S, P);
            contour_totals<64>(S, P);
            if (lane == 0) contour_store_frame(slab, rows, (size_t)cap.row0 + f0 + k, S, P, hop);
        }
}

__global__ __launch_bounds__(256) void contour_phonemes_kernel(const int32_t *__restrict__ cum, const uint4 *__restrict__ slab,
                                                               ContourRow *__restrict__ rows, const Segs tokens, const Segs frames, int hop)
{
    const int u = blockIdx.y;
    const Seg tk = seg_at(tokens, u), cap = seg_at(frames, u);
    const int lane = threadIdx.x & 63;
    const int i = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (int)(threadIdx.x >> 6));
    if (i >= tk.rows) return;                                      // the whole wave
    int start, d;
    contour_extent(cum + tk.row0, i, cap.rows, start, d);
    start = __builtin_amdgcn_readfirstlane(start);
    d = __builtin_amdgcn_readfirstlane(d);
    d = d > 0 ? d : 0;
    unsigned long long S = 0;
    uint32_t P = 0;
    const uint4 *sl = slab + (size_t)cap.row0 + start;             // start + d <= cap.rows (contour_extent clips both ends)
    for (int f = lane; f < d; f += 64)
    {
        const uint4 e = sl[f];
        S += (unsigned long long)e.x | ((unsigned long long)e.y << 32);
        P = e.z > P ? e.z : P;
    }
    contour_totals<64>(S, P);
    if (lane == 0)
    {
        const ContourRow r = contour_row(S, (uint64_t)d * (uint64_t)hop, P);
        *(float2 *)(rows + (size_t)tk.row0 + i) = make_float2(r.rms, r.peak);
    }
}

bool contour_hop_supported(int hop) { return hop >= 4 && (hop & 3) == 0; }

hipError_t launch_contour_frames(hipStream_t s, const float *wav, void *slab, ContourRow *rows, const Segs &frames, int hop)
{
    if (frames.nseg < 1 || frames.max_rows < 1 || !contour_hop_supported(hop) || !wav || ((uintptr_t)wav & 15) || !slab ||
        ((uintptr_t)slab & 15) || ((uintptr_t)rows & 7) || (!frames.tab && frames.nseg != 1))
        return hipErrorInvalidValue;
    const dim3 grid((frames.max_rows + CONTOUR_CHUNK_FRAMES - 1) / CONTOUR_CHUNK_FRAMES, frames.nseg);
    if (hop <= CONTOUR_REG_HOP) hipLaunchKernelGGL(contour_frames_kernel<true>, grid, dim3(256), 0, s, wav, (uint4 *)slab, rows, frames, hop);
    else hipLaunchKernelGGL(contour_frames_kernel<false>, grid, dim3(256), 0, s, wav, (uint4 *)slab, rows, frames, hop);
    return hipGetLastError();
}

hipError_t launch_contour_phonemes(hipStream_t s, const int32_t *cum, const void *slab, ContourRow *rows, const Segs &tokens,
                                   const Segs &frames, int hop)
{
    if (frames.nseg < 1 || tokens.nseg != frames.nseg || tokens.max_rows < 1 || hop < 1 || !cum || !slab || ((uintptr_t)slab & 15) || !rows ||
        ((uintptr_t)rows & 7) || (!frames.tab && frames.nseg != 1) || (!tokens.tab && tokens.nseg != 1))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(contour_phonemes_kernel, dim3((tokens.max_rows + 3) / 4, frames.nseg), dim3(256), 0, s, cum, (const uint4 *)slab, rows,
                       tokens, frames, hop);
    return hipGetLastError();
}

}  // namespace zv
