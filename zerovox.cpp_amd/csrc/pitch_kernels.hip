// pitch_kernels.hip — pitch track: the fundamental frequency and the voicing per frame and per phoneme, two passes behind the level
// contour's over the waveform the caller receives (pitch_frames, pitch_phonemes; the arithmetic: pitch.h).  A part of
// misc_kernels.hip's unit.
#include "kernels.h"
#include "pitch.h"

#include <type_traits>

namespace zv
{

// ---------------------------------------------------------------------------------------------------
// Pitch track (kernels.h: launch_pitch_frames / launch_pitch_phonemes; the rule: pitch.h).
//   frames:   grid (chunks of PITCH_CHUNK_FRAMES whole frames, segments) over the CAPACITY table.  A workgroup's four waves take
//             PITCH_WAVE_FRAMES frames each, ONE WAVE PER FRAME at a time and nothing shared between waves (no workgroup barrier).
//             Per frame the wave
//               1. loads the span (<= 1 537 samples, 25 coalesced loads of a lane at most), masked to the utterance's own [0, T * hop)
//                  and to finite samples, and reduces the peak's bit pattern over the wave;
//               2. block-scales it (pitch_quant) to 16-bit integers a[] in LDS, zeros behind the span;
//               3. makes the prefix sums of a[]^2 in LDS (a lane adds 26 consecutive samples, a wave scan joins them): E(L) is the
//                  difference of two entries, so the energies cost two reads per lag, not a multiply-add per sample and lag;
//               4. correlates: with R = ceil(lags / 64), lane l owns the R CONSECUTIVE lags min_lag - 1 + R * l + r.  Over a block
//                  of 8 samples t it needs a[t .. t + 8), the same dwords in every lane (a broadcast read), and the R + 7 samples
//                  a[t + L .. t + L + R + 7) — 8 R multiply-adds from R + 7 samples, where lags dealt round robin (lane + 64 j)
//                  would need 8 samples per 8 multiply-adds and be bound by LDS issue.  The window slides: 4 new dwords per block.
//                  Two samples sit in a dword, so c(L) grows by v_dot2_i32_i16: two multiply-adds per instruction.  A lane whose
//                  window starts at an odd sample shifts it by 16 bits (v_alignbit, the shift in a register), and the pairs at odd
//                  offsets inside the window are one more v_alignbit each.  Exact integers below 2^30: same bits as any other order;
//               5. turns its sums into r(L) (pitch_corr, f64) in LDS, over the prefix sums, which are dead by then;
//               6. picks: rmax by a butterfly, L0 and L* as wave minima of the lanes' smallest candidates (ties go to the lower lag
//                  by construction), lanes strided over the lags; lane 0 refines (pitch_refine) and makes the row (pitch_frame_row).
//             Lane 0 stores slab[row0 + f] = {Fq, voiced} and rows[row0 + f] = {f0_hz, strength}.
//             The parameters come from par[segment][PITCH_PARAM_STRIDE] in HBM (resolved on the host, uploaded with the call's input
//             block): a replayed graph picks up new lags, window and threshold; grid and LDS do not depend on them.
//   phonemes: grid (groups of four tokens, segments), one wave per token row, as contour_phonemes_kernel: the extent from the
//             regulator's scan (contour_extent), Fq and the voiced flags added strided over the lanes, lane 0 stores the row.
// Both index by ABSOLUTE frame row / token row.  No atomics and nothing to zero: every entry that is read was stored in the same run.
constexpr int PITCH_WAVE_FRAMES = PITCH_CHUNK_FRAMES / 4;          // frames of one wave
constexpr int PITCH_LANE_SAMPLES = 26;                             // consecutive samples of a lane in the prefix pass
constexpr int PITCH_LDS_SAMPLES = 64 * PITCH_LANE_SAMPLES;         // a[] of one wave: the span and zeros behind it
constexpr int PITCH_SPAN_LOADS = (PITCH_MAX_SPAN + 63) / 64;       // loads of a lane per span: 25
// the furthest dword a window touches, the prefetch behind the last block included: d0 + t / 2 + 4 + k < (513 + 63) / 2 + 1016 / 2 + 4 + 10 = 810
static_assert(((int)PITCH_LAG_HI + 1 + 63) / 2 + ((int)PITCH_WINDOW_HI - 8) / 2 + 4 + 10 <= PITCH_LDS_SAMPLES / 2, "a[] holds every sample a window may touch");
static_assert(PITCH_SPAN_LOADS * 64 <= PITCH_LDS_SAMPLES && PITCH_MAX_LAGS <= 64 * 8, "the span fits a[]; eight lags per lane cover every range");
static_assert(PITCH_MAX_LAGS * 8 <= PITCH_LDS_SAMPLES * 4, "r(L) fits over the prefix sums");

typedef short pitch_s2 __attribute__((ext_vector_type(2)));
// a[] is written as 16-bit samples and read as dwords; r(L) lies over the prefix sums
// (the LDS address space is part of the type: a pointer handed to pitch_correlate as a generic one would turn every read into a flat load)
typedef __attribute__((address_space(3))) uint32_t __attribute__((may_alias)) pitch_u32;
typedef __attribute__((address_space(3))) double __attribute__((may_alias)) pitch_f64;

__device__ __forceinline__ void pitch_wave_sync()
{
    // LDS written by one lane is read by another of the SAME wave: order the accesses, no other wave takes part
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

__device__ __forceinline__ int pitch_dot2(uint32_t a, uint32_t b, int c)
{
    pitch_s2 x, y;
    __builtin_memcpy(&x, &a, 4);
    __builtin_memcpy(&y, &b, 4);
    return __builtin_amdgcn_sdot2(x, y, c, false);
}

// step 4 and 5 for R lags per lane: r(L) of the lags lo .. hi1 (= max_lag + 1) into rr[L - lo]
template <int R>
__device__ __attribute__((noinline)) void pitch_correlate(const pitch_u32 *a32, const pitch_u32 *psq, pitch_f64 *rr, int lane, int lo,
                                                int hi1, int W)
{
    constexpr int NW = (R + 8) / 2 + 1;       // dwords of the aligned window (the last one only feeds a shift)
    constexpr int ND = NW + 1;                // dwords read: one more, for a window that starts at an odd sample
    const int Lb = lo + R * lane;
    // the energies first: the prefix sums are overwritten by r(L) below
    int64_t E[R];
#pragma unroll
    for (int r = 0; r < R; r++)
    {
        const int L = Lb + r < hi1 ? Lb + r : hi1;
        E[r] = (int64_t)(psq[L + W] - psq[L]);
    }
    const int64_t E0 = (int64_t)psq[W];
    const int d0 = Lb >> 1;
    const uint32_t sh = (uint32_t)(Lb & 1) * 16u;
    int c[R];
#pragma unroll
    for (int r = 0; r < R; r++) c[r] = 0;
    // the window of the block at hand in registers, and the next block's 4 new dwords and its 8 samples a[t + 8 .. t + 16) on their way
    // while this block is added up: the LDS latency hides behind the dot products.  (Reads behind the last block stay inside a[].)
    uint32_t raw[ND], b[4];
#pragma unroll
    for (int k = 0; k < ND; k++) raw[k] = a32[d0 + k];
#pragma unroll
    for (int p = 0; p < 4; p++) b[p] = a32[p];
    // one block of 8 samples; MASKED: the window's last, partial block, whose samples at or behind W take no part
    auto block = [&](int t, auto masked) {
        const int tn = (t >> 1) + 4;
        uint32_t nraw[4], nb[4];
#pragma unroll
        for (int k = 0; k < 4; k++) nraw[k] = a32[d0 + tn + ND - 4 + k];
#pragma unroll
        for (int p = 0; p < 4; p++) nb[p] = a32[tn + p];
        uint32_t win[NW], odd[NW - 1];
#pragma unroll
        for (int k = 0; k < NW; k++) win[k] = __builtin_amdgcn_alignbit(raw[k + 1], raw[k], sh);
#pragma unroll
        for (int k = 0; k < NW - 1; k++) odd[k] = __builtin_amdgcn_alignbit(win[k + 1], win[k], 16u);
#pragma unroll
        for (int p = 0; p < 4; p++)
        {
            // a[t + 2p], a[t + 2p + 1]: the same dword in every lane
            uint32_t bp = b[p];
            if (decltype(masked)::value)
            {
                const int left = W - (t + 2 * p);
                bp = left >= 2 ? bp : (left == 1 ? (bp & 0xffffu) : 0u);
            }
#pragma unroll
            for (int r = 0; r < R; r++)
            {
                const int o = 2 * p + r;
                c[r] = pitch_dot2(bp, (o & 1) ? odd[o >> 1] : win[o >> 1], c[r]);
            }
        }
#pragma unroll
        for (int k = 0; k < ND - 4; k++) raw[k] = raw[k + 4];
#pragma unroll
        for (int k = 0; k < 4; k++)
        {
            raw[ND - 4 + k] = nraw[k];
            b[k] = nb[k];
        }
    };
    const int Wfull = W & ~7;
    for (int t = 0; t < Wfull; t += 8) block(t, std::false_type{});
    if (Wfull < W) block(Wfull, std::true_type{});
    pitch_wave_sync();                        // every lane has its energies: the prefix sums are dead
#pragma unroll
    for (int r = 0; r < R; r++)
        if (Lb + r <= hi1) rr[Lb + r - lo] = pitch_corr((int64_t)c[r], E0, E[r]);
    pitch_wave_sync();
}

__global__ __launch_bounds__(256) void pitch_frames_kernel(const float *__restrict__ wav, uint2 *__restrict__ slab, PitchFrameRow *__restrict__ rows,
                                                           const uint32_t *__restrict__ par, const Segs frames, int hop, int sr)
{
    __shared__ __attribute__((aligned(16))) short s_a[4][PITCH_LDS_SAMPLES];
    __shared__ __attribute__((aligned(16))) uint32_t s_p[4][PITCH_LDS_SAMPLES];
    const int u = blockIdx.y;
    const Seg cap = seg_at(frames, u);
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int f0 = __builtin_amdgcn_readfirstlane(blockIdx.x * PITCH_CHUNK_FRAMES + wv * PITCH_WAVE_FRAMES);
    if (f0 >= cap.rows) return;                                    // the whole wave
    const int nfr = cap.rows - f0 < PITCH_WAVE_FRAMES ? cap.rows - f0 : PITCH_WAVE_FRAMES;
    PitchParams p;
    p.min_lag = __builtin_amdgcn_readfirstlane(par[(size_t)u * PITCH_PARAM_STRIDE + 0]);
    p.max_lag = __builtin_amdgcn_readfirstlane(par[(size_t)u * PITCH_PARAM_STRIDE + 1]);
    p.window = __builtin_amdgcn_readfirstlane(par[(size_t)u * PITCH_PARAM_STRIDE + 2]);
    p.voiced_threshold = level_from_bits(__builtin_amdgcn_readfirstlane(par[(size_t)u * PITCH_PARAM_STRIDE + 3]));
    // the host resolves and checks the rows (pitch_params_resolve); a row outside the bounds would index past the LDS arrays
    if (!(p.min_lag >= PITCH_LAG_LO && p.max_lag > p.min_lag && p.max_lag <= PITCH_LAG_HI && p.max_lag <= PITCH_LAG_RATIO * p.min_lag &&
          p.window >= PITCH_WINDOW_LO && p.window <= PITCH_WINDOW_HI))
        return;
    const int W = (int)p.window, lo = (int)p.min_lag - 1, hi1 = (int)p.max_lag + 1, M = W + (int)p.max_lag + 1;
    const int R = (hi1 - lo + 1 + 63) >> 6;                        // lags per lane, 1 .. 8
    const long long n = (long long)cap.rows * hop;                 // the utterance's own samples
    const float *xs = wav + (size_t)cap.row0 * hop;
    short *a = s_a[wv];
    pitch_u32 *psq = (pitch_u32 *)s_p[wv];
    pitch_f64 *rr = (pitch_f64 *)psq;
    for (int k = 0; k < nfr; k++)
    {
        const int f = f0 + k;
        const size_t row = (size_t)cap.row0 + f;
        const long long s0 = pitch_span((uint32_t)f, (uint32_t)hop, (uint32_t)M);
        // 1. the span and its peak
        float y[PITCH_SPAN_LOADS];
        uint32_t pk = 0;
#pragma unroll
        for (int i = 0; i < PITCH_SPAN_LOADS; i++)
        {
            const int t = i * 64 + lane;
            const long long s = s0 + t;
            const float x = t < M && s >= 0 && s < n ? xs[s] : 0.0f;
            const uint32_t ab = pitch_abs_bits(x);
            y[i] = ab == (level_bits(x) & 0x7fffffffu) ? x : 0.0f;
            pk = ab > pk ? ab : pk;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1)
        {
            const uint32_t q = (uint32_t)__shfl_xor((int)pk, o, 64);
            pk = q > pk ? q : pk;
        }
        PitchSlabRow sl;
        PitchFrameRow out;
        if (pk < PITCH_SILENT_BITS)
            out = pitch_frame_none(sl);
        else
        {
            // 2. block scale
            const double scale = pitch_scale(pk);
#pragma unroll
            for (int i = 0; i < PITCH_SPAN_LOADS; i++) a[i * 64 + lane] = (short)pitch_quant(y[i], scale);
            a[PITCH_SPAN_LOADS * 64 + lane] = 0;
            static_assert((PITCH_SPAN_LOADS + 1) * 64 == PITCH_LDS_SAMPLES, "the zero fill ends a[]");
            pitch_wave_sync();
            // 3. prefix sums of the squares: psq[i] = sum of a[t]^2 over t < i
            uint32_t sq[PITCH_LANE_SAMPLES], tot = 0;
#pragma unroll
            for (int j = 0; j < PITCH_LANE_SAMPLES; j++)
            {
                const int v = a[lane * PITCH_LANE_SAMPLES + j];
                sq[j] = tot;
                tot += (uint32_t)(v * v);
            }
            uint32_t inc = tot;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1)
            {
                const uint32_t q = (uint32_t)__shfl_up((int)inc, o, 64);
                inc += lane >= o ? q : 0u;
            }
            const uint32_t before = inc - tot;
#pragma unroll
            for (int j = 0; j < PITCH_LANE_SAMPLES; j++) psq[lane * PITCH_LANE_SAMPLES + j] = before + sq[j];
            pitch_wave_sync();
            // 4., 5. the correlations
            const pitch_u32 *a32 = (const pitch_u32 *)a;
            switch (R)
            {
            case 1: pitch_correlate<1>(a32, psq, rr, lane, lo, hi1, W); break;
            case 2: pitch_correlate<2>(a32, psq, rr, lane, lo, hi1, W); break;
            case 3: pitch_correlate<3>(a32, psq, rr, lane, lo, hi1, W); break;
            case 4: pitch_correlate<4>(a32, psq, rr, lane, lo, hi1, W); break;
            case 5: pitch_correlate<5>(a32, psq, rr, lane, lo, hi1, W); break;
            case 6: pitch_correlate<6>(a32, psq, rr, lane, lo, hi1, W); break;
            case 7: pitch_correlate<7>(a32, psq, rr, lane, lo, hi1, W); break;
            default: pitch_correlate<8>(a32, psq, rr, lane, lo, hi1, W); break;
            }
            // 6. the pick, lanes strided over the lags min_lag .. max_lag
            const int Lmin = (int)p.min_lag, Lmax = (int)p.max_lag;
            double rmax = 0.0;
            for (int L = Lmin + lane; L <= Lmax; L += 64) rmax = rr[L - lo] > rmax ? rr[L - lo] : rmax;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1)
            {
                const double q = __shfl_xor(rmax, o, 64);
                rmax = q > rmax ? q : rmax;
            }
            if (rmax == 0.0)
                out = pitch_frame_none(sl);
            else
            {
                const double gate = PITCH_PICK_SHARE * rmax;
                int L0 = Lmax;
                for (int L = Lmin + lane; L <= Lmax; L += 64)
                    if (rr[L - lo] >= gate)
                    {
                        L0 = L;
                        break;
                    }
#pragma unroll
                for (int o = 32; o > 0; o >>= 1)
                {
                    const int q = __shfl_xor(L0, o, 64);
                    L0 = q < L0 ? q : L0;
                }
                int Ls = Lmax;
                for (int L = L0 + lane; L < Lmax; L += 64)
                    if (rr[L + 1 - lo] <= rr[L - lo])
                    {
                        Ls = L;
                        break;
                    }
#pragma unroll
                for (int o = 32; o > 0; o >>= 1)
                {
                    const int q = __shfl_xor(Ls, o, 64);
                    Ls = q < Ls ? q : Ls;
                }
                const double f0hz = pitch_refine(rr[Ls - 1 - lo], rr[Ls - lo], rr[Ls + 1 - lo], (uint32_t)Ls, (uint32_t)sr);
                out = pitch_frame_row(f0hz, rr[Ls - lo], p.voiced_threshold, sl);
            }
            pitch_wave_sync();                // the next frame overwrites a[] and the prefix sums
        }
        if (lane == 0)
        {
            slab[row] = make_uint2(sl.fq, sl.voiced);
            if (rows) *(float2 *)(rows + row) = make_float2(out.f0_hz, out.strength);
        }
    }
}

__global__ __launch_bounds__(256) void pitch_phonemes_kernel(const int32_t *__restrict__ cum, const uint2 *__restrict__ slab,
                                                             PitchPhonemeRow *__restrict__ rows, const Segs tokens, const Segs frames)
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
    unsigned long long SF = 0;
    uint32_t nv = 0;
    const uint2 *sl = slab + (size_t)cap.row0 + start;             // start + d <= cap.rows (contour_extent clips both ends)
    for (int f = lane; f < d; f += 64)
    {
        const uint2 e = sl[f];
        SF += e.x;
        nv += e.y;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
    {
        SF += (unsigned long long)__shfl_xor((long long)SF, o, 64);
        nv += (uint32_t)__shfl_xor((int)nv, o, 64);
    }
    if (lane == 0)
    {
        const PitchPhonemeRow r = pitch_phoneme_row(SF, nv, (uint64_t)d);
        *(float2 *)(rows + (size_t)tk.row0 + i) = make_float2(r.f0_hz, r.voiced);
    }
}

hipError_t launch_pitch_frames(hipStream_t s, const float *wav, void *slab, PitchFrameRow *rows, const uint32_t *par, const Segs &frames, int hop,
                               int sr)
{
    if (frames.nseg < 1 || frames.max_rows < 1 || hop < 1 || sr < 1 || !wav || !slab || ((uintptr_t)slab & 7) || ((uintptr_t)rows & 7) || !par ||
        (!frames.tab && frames.nseg != 1))
        return hipErrorInvalidValue;
    const dim3 grid((frames.max_rows + PITCH_CHUNK_FRAMES - 1) / PITCH_CHUNK_FRAMES, frames.nseg);
    hipLaunchKernelGGL(pitch_frames_kernel, grid, dim3(256), 0, s, wav, (uint2 *)slab, rows, par, frames, hop, sr);
    return hipGetLastError();
}

hipError_t launch_pitch_phonemes(hipStream_t s, const int32_t *cum, const void *slab, PitchPhonemeRow *rows, const Segs &tokens, const Segs &frames)
{
    if (frames.nseg < 1 || tokens.nseg != frames.nseg || tokens.max_rows < 1 || !cum || !slab || ((uintptr_t)slab & 7) || !rows ||
        ((uintptr_t)rows & 7) || (!frames.tab && frames.nseg != 1) || (!tokens.tab && tokens.nseg != 1))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(pitch_phonemes_kernel, dim3((tokens.max_rows + 3) / 4, frames.nseg), dim3(256), 0, s, cum, (const uint2 *)slab, rows, tokens,
                       frames);
    return hipGetLastError();
}

}  // namespace zv
