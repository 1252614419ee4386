// envelope_kernels.hip — amplitude envelope: the knots pass and the apply pass over a finished waveform (env_knots, env_apply; the
// arithmetic: envelope.h).  A part of misc_kernels.hip's unit.
#include "kernels.h"
#include "envelope.h"
#include "level.h"

namespace zv
{

// ---------------------------------------------------------------------------------------------------
// Amplitude envelope (kernels.h: launch_env_knots / launch_env_apply; the rule: envelope.h).
//   knots: workgroup (c, u) writes the knots B[c * 256 .. c * 256 + 256) of segment u, f <= nf, into knots[row0 + u + f] (a segment of
//          `rows` frames has up to rows + 1 knots, hence the + u).  It stages the frame gains F[f0 - r - 1 .. f0 + 255 + r] in LDS — the
//          owner of a frame from a search in the regulator's scan — and every thread adds its two windows.  Integer sums: any split,
//          the same table.  A segment without speech writes nothing.
//   apply: grid (chunks of LEVEL_CHUNK_SAMPLES samples, segments) like level_apply_kernel.  Workgroup (c, u) stages the knots of its
//          chunk's frames in LDS and, per frame, the gain of a frame whose two knots are equal (one f64 quotient per FRAME, computed
//          while the chunk's 16-byte loads travel); a sample of such a frame outside the fades takes that value, every other sample
//          the whole rule (env_sample_gain).  Scales the segment's CAPACITY in place.
// No atomics and nothing to zero: every knot apply reads was stored by knots in the same run.
constexpr int ENV_KNOT_TILE = 256;
constexpr int ENV_STAGE = ENV_KNOT_TILE + 2 * ENV_MAX_RAMP + 1;          // frame gains a knots workgroup stages
constexpr int ENV_LDS_KNOTS = 1024;                                     // knots an apply workgroup stages: chunk / hop + 3 at most
constexpr int ENV_SWEEPS = (LEVEL_CHUNK_SAMPLES + 1023) / 1024;

__device__ __forceinline__ int env_speech_frames(const int32_t *__restrict__ n_frames, int u, int cap_rows)
{
    const int nf = __builtin_amdgcn_readfirstlane(n_frames[u]);
    return nf < 0 ? 0 : (nf < cap_rows ? nf : cap_rows);
}

__global__ __launch_bounds__(ENV_KNOT_TILE) void env_knots_kernel(const int32_t *__restrict__ cum, const float *__restrict__ gain,
                                                                  const int32_t *__restrict__ env, const int32_t *__restrict__ n_frames,
                                                                  uint32_t *__restrict__ knots, const Segs tokens, const Segs frames)
{
    __shared__ uint32_t F[ENV_STAGE];
    const int u = blockIdx.y;
    const Seg tk = seg_at(tokens, u), cap = seg_at(frames, u);
    const int nf = env_speech_frames(n_frames, u, cap.rows);
    const int f0 = blockIdx.x * ENV_KNOT_TILE;
    if (nf <= 0 || f0 > nf) return;
    int r = __builtin_amdgcn_readfirstlane(env[(size_t)u * ENV_CTL_STRIDE]);
    r = r < 0 ? 0 : (r < ENV_MAX_RAMP ? r : ENV_MAX_RAMP);
    // F[k] = the gain of frame f0 - r - 1 + k, k < 256 + 2r + 1
    const int nstage = ENV_KNOT_TILE + 2 * r + 1;
    for (int k = threadIdx.x; k < nstage; k += ENV_KNOT_TILE)
        F[k] = env_frame_gain(cum + tk.row0, gain + tk.row0, tk.rows, nf, f0 - r - 1 + k);
    __syncthreads();
    const int f = f0 + threadIdx.x;
    if (f > nf) return;
    // B[f] = A[f - 1] + A[f]: frames f - 1 - r .. f - 1 + r and f - r .. f + r, staged at threadIdx.x + (0 .. 2r) and + (1 .. 2r + 1)
    uint32_t b = 0;
    for (int k = 0; k <= 2 * r; k++) b += F[threadIdx.x + k] + F[threadIdx.x + 1 + k];
    knots[(size_t)cap.row0 + u + f] = b;
}

__global__ __launch_bounds__(256) void env_apply_kernel(float *__restrict__ wav, const int32_t *__restrict__ n_frames,
                                                        const uint32_t *__restrict__ knots, const int32_t *__restrict__ env,
                                                        const Segs frames, int hop)
{
    __shared__ uint32_t s_b[ENV_LDS_KNOTS];
    __shared__ float s_e[ENV_LDS_KNOTS];
    const int u = blockIdx.y;
    const Seg cap = seg_at(frames, u);
    const long total = (long)cap.rows * hop;
    const long i0 = (long)blockIdx.x * LEVEL_CHUNK_SAMPLES;
    if (i0 >= total) return;
    // the chunk's 16-byte loads are issued first: they travel while the knots are staged and the flat frames' gains are computed
    float *xs = wav + (size_t)cap.row0 * hop + i0;
    const int len = (int)(total - i0 < LEVEL_CHUNK_SAMPLES ? total - i0 : LEVEL_CHUNK_SAMPLES);
    const bool vec = ((uintptr_t)xs & 15) == 0;
    float4 q[ENV_SWEEPS];
#pragma unroll
    for (int k = 0; k < ENV_SWEEPS; k++)
    {
        const int i = k * 1024 + threadIdx.x * 4;
        if (vec && i + 4 <= len) q[k] = *(const float4 *)(xs + i);
    }
    const int nf = env_speech_frames(n_frames, u, cap.rows);
    const int32_t *ec = env + (size_t)u * ENV_CTL_STRIDE;
    int r = __builtin_amdgcn_readfirstlane(ec[0]);
    r = r < 0 ? 0 : (r < ENV_MAX_RAMP ? r : ENV_MAX_RAMP);
    const uint32_t Fi = (uint32_t)__builtin_amdgcn_readfirstlane(ec[1]), Fo = (uint32_t)__builtin_amdgcn_readfirstlane(ec[2]);
    const long n = (long)nf * hop;
    const int64_t den = env_den(r, hop);
    // samples [flat0, flat1) of the segment are outside both fades
    const long flat0 = (long)Fi, flat1 = Fo > 0 ? n - (long)Fo : total;
    const int f_lo = (int)(i0 / hop);
    const int nk = (int)((i0 + len - 1) / hop) - f_lo + 2;          // knots f_lo .. the end of the chunk's last frame; <= ENV_LDS_KNOTS (launcher)
    if (nf > 0)
    {
        const uint32_t *kn = knots + (size_t)cap.row0 + u;
        for (int k = threadIdx.x; k < nk; k += 256)
        {
            const int f = f_lo + k;
            const uint32_t b0 = kn[f < nf ? f : nf], b1 = kn[f + 1 < nf ? f + 1 : nf];
            s_b[k] = b0;
            // a frame between equal knots: num = b0 * hop at every j
            s_e[k] = b0 == b1 ? env_sample_gain(b0, b0, hop, 0, den, 0, n, 0u, 0u) : 0.0f;
        }
    }
    __syncthreads();
    const float e0 = env_empty_gain(Fo);
    // the gain of sample i of the chunk, in frame f_lo + k at offset j
    auto gain_at = [&](int i, int k, int j) -> float {
        if (nf <= 0) return e0;
        const uint32_t b0 = s_b[k], b1 = s_b[k + 1];
        const long s = i0 + i;
        if (b0 == b1 && s >= flat0 && s < flat1) return s_e[k];
        return env_sample_gain(b0, b1, hop, j, den, s, n, Fi, Fo);
    };
    const int j_lo = (int)(i0 - (long)f_lo * hop);                  // offset of the chunk's first sample in frame f_lo
    if (vec)
    {
#pragma unroll
        for (int kk = 0; kk < ENV_SWEEPS; kk++)
        {
            const int i = kk * 1024 + threadIdx.x * 4;
            if (i + 4 <= len)
            {
                const unsigned p = (unsigned)(j_lo + i);
                int k = (int)(p / (unsigned)hop), j = (int)(p - (unsigned)k * (unsigned)hop);
                float e[4];
#pragma unroll
                for (int t = 0; t < 4; t++)
                {
                    e[t] = gain_at(i + t, k, j);
                    if (++j == hop) { j = 0; k++; }
                }
                *(float4 *)(xs + i) = make_float4(q[kk].x * e[0], q[kk].y * e[1], q[kk].z * e[2], q[kk].w * e[3]);
            }
        }
        const int i = (len & ~3) + threadIdx.x;                     // the last samples of a length that is no multiple of 4
        if (threadIdx.x < 3 && i < len)
        {
            const unsigned p = (unsigned)(j_lo + i);
            const int k = (int)(p / (unsigned)hop), j = (int)(p - (unsigned)k * (unsigned)hop);
            xs[i] = xs[i] * gain_at(i, k, j);
        }
    }
    else
        for (int i = threadIdx.x; i < len; i += 256)
        {
            const unsigned p = (unsigned)(j_lo + i);
            const int k = (int)(p / (unsigned)hop), j = (int)(p - (unsigned)k * (unsigned)hop);
            xs[i] = xs[i] * gain_at(i, k, j);
        }
}

// the smallest hop the apply pass takes: a chunk's frames, and the knot behind the last, must fit its LDS table
bool env_hop_supported(int hop) { return hop >= 1 && LEVEL_CHUNK_SAMPLES / hop + 3 <= ENV_LDS_KNOTS; }

hipError_t launch_env_knots(hipStream_t s, const int32_t *cum, const float *gain, const int32_t *env, const int32_t *n_frames,
                            uint32_t *knots, const Segs &tokens, const Segs &frames)
{
    if (frames.nseg < 1 || frames.max_rows < 1 || tokens.nseg != frames.nseg || !cum || !gain || !env || !n_frames || !knots ||
        (!frames.tab && frames.nseg != 1) || (!tokens.tab && tokens.nseg != 1))
        return hipErrorInvalidValue;
    const int tiles = frames.max_rows / ENV_KNOT_TILE + 1;          // knots 0 .. max_rows
    hipLaunchKernelGGL(env_knots_kernel, dim3(tiles, frames.nseg), dim3(ENV_KNOT_TILE), 0, s, cum, gain, env, n_frames, knots, tokens, frames);
    return hipGetLastError();
}

hipError_t launch_env_apply(hipStream_t s, float *wav, const int32_t *n_frames, const uint32_t *knots, const int32_t *env,
                            const Segs &frames, int hop)
{
    if (frames.nseg < 1 || frames.max_rows < 1 || !env_hop_supported(hop) || !wav || !n_frames || !knots || !env ||
        (!frames.tab && frames.nseg != 1))
        return hipErrorInvalidValue;
    const int chunks = level_chunks(frames.max_rows, hop);
    hipLaunchKernelGGL(env_apply_kernel, dim3(chunks, frames.nseg), dim3(256), 0, s, wav, n_frames, knots, env, frames, hop);
    return hipGetLastError();
}

}  // namespace zv
