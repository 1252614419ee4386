// bands_kernels.hip — band levels: the energy per frequency band, per frame and per phoneme, two passes behind the pitch track's over
// the waveform the caller receives (bands_frames, bands_phonemes; the arithmetic: bands.h).  A part of misc_kernels.hip's unit.
#include "kernels.h"
#include "bands.h"

namespace zv
{

// ---------------------------------------------------------------------------------------------------
// Band levels (kernels.h: launch_bands_frames / launch_bands_phonemes; the rule: bands.h).
//   frames:   grid (tiles of BANDS_TILE_FRAMES whole frames, segments) over the CAPACITY table: an integer GEMM
//             [32 frames x 1024 samples] . [1024 samples x (cos | sin) of 513 bins] on v_mfma_i32_16x16x64_i8.
//               1. Quantise: each of the four waves takes eight frames, one at a time.  A lane loads 16 samples of the frame's span as
//                  four pairs of aligned 8-byte loads (the hop is a multiple of 4, so a span starts at an even sample; at hop 300 it
//                  starts at 2 mod 4, so there is no 16-byte load), masked to the utterance's own [0, T * hop); the NEXT frame's loads
//                  are issued before this frame is reduced and quantised.  The spans of a tile overlap 3.4 times at hop 300 and the
//                  re-reads hit the vector cache.  Non-finite samples count as +0.0, the wave reduces the peak, and the block-scaled
//                  samples (bands_quant) go to LDS as two signed 8-bit digit planes, a = 128 * hi + lo (bands_digits), four samples to
//                  a dword.  A plane's row is 1 040 bytes: the 16 rows a 128-bit fragment read touches then start 4 banks apart and
//                  cover the 64 banks once.
//               2. Multiply: wave w takes the PAIRS of 16-bin blocks w, w + 4, ...: the workgroup streams the table ONCE from L2 for its
//                  32 frames.  Per k step of 64 samples a lane loads four table fragments (cos and sin of both blocks, 16 bytes each,
//                  stored in fragment order: bands_table_index) and four frame fragments (two row tiles x two digit planes) from LDS,
//                  and issues 16 MFMAs into 16 accumulators (64 registers).  A frame fragment is the A operand (rows = frames), a table
//                  fragment the B operand (columns = bins): lane l holds row / column l & 15 and the 16 samples 64 * step + 16 * (l >> 4)
//                  + j of it.  Both operands take their samples from the same places, so the sum over k is the same whatever order the
//                  hardware gives the 64 products.  C/D: column = lane & 15, row = 4 * (lane >> 4) + register: the cos and the sin
//                  accumulator of one (frame, bin) sit in the same lane and register, Re = 128 * acc_hi + acc_lo exactly, and
//                  Q = (Re^2 + Im^2) >> 6 is formed in place.
//               3. Band sums: Q goes to S[frame][band] in LDS by a 64-bit integer atomic add (order cannot show).  Where the block's 16
//                  bins lie in one band, which is most of the default bands' bins, the 16 lanes of a frame add up by butterflies first.
//               4. Rows: a thread per (frame, band) turns S into the row entry and the kept power (bands_row, f64).
//             The parameters come from par[segment][BANDS_PARAM_STRIDE] in HBM (resolved on the host, uploaded with the call's input
//             block): a replayed graph picks up new edges and a new band count; grid and LDS do not depend on them.  n_bands == 0 marks
//             a segment that asked for nothing: its workgroups return at once.
//   phonemes: grid (groups of four tokens, segments), one wave per token row, a lane per band: the extent from the regulator's scan
//             (contour_extent), the kept powers added frame after frame (a frame's 64 entries are one 512-byte line).
// Both index by ABSOLUTE frame row / token row.  Nothing in HBM to zero: every entry that is read was stored in the same run.
constexpr int BANDS_LDS_ROW = BANDS_N + 16;                        // bytes of a frame in a digit plane
constexpr int BANDS_WAVE_FRAMES = BANDS_TILE_FRAMES / 4;           // frames a wave quantises
constexpr int BANDS_PREFETCH = 4;                                  // k steps of table fragments in flight (64 registers)
constexpr int BANDS_SILENT = -1000;                                // s_k of a silent frame or one behind the capacity
static_assert(BANDS_TILE_FRAMES == 32 && BANDS_BIN_BLOCKS % 2 == 0 && BANDS_BIN_BLOCKS * 16 >= BANDS_BINS, "two row tiles; pairs of bin blocks cover the bins");

typedef int bands_i4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void bands_frames_kernel(const float *__restrict__ wav, const int8_t *__restrict__ tab,
                                                           unsigned long long *__restrict__ slab, float *__restrict__ rows,
                                                           const uint32_t *__restrict__ par, const Segs frames, int hop)
{
    __shared__ __attribute__((aligned(16))) int8_t s_a[2][BANDS_TILE_FRAMES][BANDS_LDS_ROW];
    __shared__ unsigned long long s_sum[BANDS_TILE_FRAMES][BANDS_MAX];
    __shared__ uint8_t s_band[BANDS_BIN_BLOCKS * 16];
    __shared__ int s_k[BANDS_TILE_FRAMES];
    const int u = blockIdx.y;
    const Seg cap = seg_at(frames, u);
    const int f0 = blockIdx.x * BANDS_TILE_FRAMES;
    if (f0 >= cap.rows) return;                                    // the whole workgroup
    const uint32_t *pr = par + (size_t)u * BANDS_PARAM_STRIDE;
    const int nb = __builtin_amdgcn_readfirstlane((int)pr[0]);
    // the host resolves and checks the rows (bands_resolve); 0: the segment asked for no table
    if (nb < 1 || nb > (int)BANDS_MAX) return;
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int i = tid; i < BANDS_TILE_FRAMES * (int)BANDS_MAX; i += 256) (&s_sum[0][0])[i] = 0ull;
    for (int bin = tid; bin < BANDS_BIN_BLOCKS * 16; bin += 256)
    {
        uint32_t band = 0xffu;
        for (int b = 0; b < nb; b++)
            if (pr[1 + b] <= (uint32_t)bin && (uint32_t)bin < pr[2 + b]) band = (uint32_t)b;
        s_band[bin] = (uint8_t)(bin < BANDS_BINS ? band : 0xffu);
    }
    // 1. quantise
    const long long n = (long long)cap.rows * hop;                 // the utterance's own samples
    const float *xs = wav + (size_t)cap.row0 * hop;
    // a frame's 16 samples of this lane as 8 pairs, out of bounds +0.0; a frame behind the capacity is all zeros (and so silent).  The
    // hop is a multiple of 4 (launch_bands_frames), so s0 and n are even and xs is 16-byte aligned: every pair is an aligned 8-byte
    // load that lies wholly inside or wholly outside the utterance
    auto span = [&](int f, float2 (&x)[8]) {
        const long long s0 = bands_span((uint32_t)f, (uint32_t)hop);
#pragma unroll
        for (int q = 0; q < 4; q++)
#pragma unroll
            for (int h = 0; h < 2; h++)
            {
                const long long s = s0 + q * 256 + lane * 4 + 2 * h;
                x[q * 2 + h] = f < cap.rows && s >= 0 && s < n ? *(const float2 *)(xs + s) : make_float2(0.0f, 0.0f);
            }
    };
    float2 next[8];
    span(f0 + wv * BANDS_WAVE_FRAMES, next);
    for (int i = 0; i < BANDS_WAVE_FRAMES; i++)
    {
        const int fl = wv * BANDS_WAVE_FRAMES + i;
        float y[16];
        uint32_t pk = 0;
#pragma unroll
        for (int j = 0; j < 16; j++)
        {
            const float x = (j & 1) ? next[j >> 1].y : next[j >> 1].x;
            const uint32_t ab = level_abs_bits(x);
            y[j] = ab == (level_bits(x) & 0x7fffffffu) ? x : 0.0f;
            pk = ab > pk ? ab : pk;
        }
        // the next frame's loads are on their way while this one is reduced and quantised
        if (i + 1 < BANDS_WAVE_FRAMES) span(f0 + fl + 1, next);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1)
        {
            const uint32_t q = (uint32_t)__shfl_xor((int)pk, o, 64);
            pk = q > pk ? q : pk;
        }
        const bool live = pk >= BANDS_SILENT_BITS;                 // wave uniform
        const int k = live ? bands_exponent(pk) : BANDS_SILENT;
        const double scale = bands_pow2(live ? k : 0);
#pragma unroll
        for (int q = 0; q < 4; q++)
        {
            uint32_t whi = 0, wlo = 0;
#pragma unroll
            for (int j = 0; j < 4; j++)
            {
                int32_t hi = 0, lo = 0;
                if (live) bands_digits(bands_quant(y[q * 4 + j], scale), hi, lo);
                whi |= ((uint32_t)hi & 0xffu) << (8 * j);
                wlo |= ((uint32_t)lo & 0xffu) << (8 * j);
            }
            *(uint32_t *)&s_a[0][fl][q * 256 + lane * 4] = whi;
            *(uint32_t *)&s_a[1][fl][q * 256 + lane * 4] = wlo;
        }
        if (lane == 0) s_k[fl] = k;
    }
    __syncthreads();
    // 2., 3. multiply and add up the bands
    const int r16 = lane & 15, g4 = lane >> 4;
    for (int pair = wv; pair < BANDS_BIN_BLOCKS / 2; pair += 4)
    {
        bands_i4 acc[2][2][2][2];                                  // [bin block][row tile][digit plane][cos, sin]
#pragma unroll
        for (int i = 0; i < 16; i++) (&acc[0][0][0][0])[i] = bands_i4{0, 0, 0, 0};
        const int8_t *tb = tab + (size_t)lane * 16;
        // the table fragments of k step ks, [bin block][cos, sin]
        auto table = [&](int ks, bands_i4 (&B)[2][2]) {
#pragma unroll
            for (int nbk = 0; nbk < 2; nbk++)
#pragma unroll
                for (int trig = 0; trig < 2; trig++)
                    B[nbk][trig] = *(const bands_i4 *)(tb + (((size_t)trig * BANDS_BIN_BLOCKS + (2 * pair + nbk)) * BANDS_K_STEPS + ks) * 1024);
        };
        // a ring of BANDS_PREFETCH k steps of table fragments in registers: a step's loads are issued BANDS_PREFETCH steps ahead of the
        // MFMAs that take them, and the scheduling barriers keep that order (left alone, the compiler waits for every load where it is
        // issued: one L2 latency per load and one wave per SIMD to hide it)
        bands_i4 ring[BANDS_PREFETCH][2][2];
#pragma unroll
        for (int ks = 0; ks < BANDS_PREFETCH; ks++) table(ks, ring[ks]);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int ks = 0; ks < BANDS_K_STEPS; ks++)
        {
            bands_i4 A[2][2];
#pragma unroll
            for (int mt = 0; mt < 2; mt++)
#pragma unroll
                for (int pl = 0; pl < 2; pl++) A[mt][pl] = *(const bands_i4 *)&s_a[pl][mt * 16 + r16][ks * 64 + 16 * g4];
#pragma unroll
            for (int nbk = 0; nbk < 2; nbk++)
#pragma unroll
                for (int mt = 0; mt < 2; mt++)
#pragma unroll
                    for (int pl = 0; pl < 2; pl++)
#pragma unroll
                        for (int trig = 0; trig < 2; trig++)
                            acc[nbk][mt][pl][trig] =
                                __builtin_amdgcn_mfma_i32_16x16x64_i8(A[mt][pl], ring[ks % BANDS_PREFETCH][nbk][trig], acc[nbk][mt][pl][trig], 0, 0, 0);
            if (ks + BANDS_PREFETCH < BANDS_K_STEPS) table(ks + BANDS_PREFETCH, ring[ks % BANDS_PREFETCH]);
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int nbk = 0; nbk < 2; nbk++)
        {
            const int blk = 2 * pair + nbk;
            const uint32_t band = s_band[blk * 16 + r16];
            const uint32_t b_lo = s_band[blk * 16], b_hi = s_band[blk * 16 + 15];
            // wave uniform.  Bands are runs of consecutive bins, so a block whose first and last bin lie in the SAME BAND lies in it
            // whole.  That does not hold for "no band" (0xff): bins between two unassigned ends may still belong to bands, so such
            // a block goes bin by bin, and is skipped only when none of its 16 bins has a band (every group of 16 lanes holds the
            // same 16 bins, so the ballot is the same question in all four)
            const bool one_band = b_lo == b_hi && b_lo != 0xffu;
            if (__ballot(band != 0xffu) == 0) continue;
#pragma unroll
            for (int mt = 0; mt < 2; mt++)
#pragma unroll
                for (int reg = 0; reg < 4; reg++)
                {
                    const int fl = mt * 16 + g4 * 4 + reg;
                    const int32_t re = 128 * acc[nbk][mt][0][0][reg] + acc[nbk][mt][1][0][reg];
                    const int32_t im = 128 * acc[nbk][mt][0][1][reg] + acc[nbk][mt][1][1][reg];
                    unsigned long long q = bands_power(re, im);
                    if (one_band)
                    {
#pragma unroll
                        for (int o = 8; o > 0; o >>= 1) q += (unsigned long long)__shfl_xor((long long)q, o, 64);
                        if (r16 == 0) atomicAdd(&s_sum[fl][b_lo], q);
                    }
                    else if (band != 0xffu)
                        atomicAdd(&s_sum[fl][band], q);
                }
        }
    }
    __syncthreads();
    // 4. rows
    for (int i = tid; i < BANDS_TILE_FRAMES * (int)BANDS_MAX; i += 256)
    {
        const int fl = i >> 6, b = i & 63, f = f0 + fl;
        if (f >= cap.rows || b >= nb) continue;
        const int k = s_k[fl];
        unsigned long long eq = 0;
        float r = 0.0f;
        if (k != BANDS_SILENT)
        {
            uint64_t e;
            r = bands_row((uint64_t)s_sum[fl][b], k, e);
            eq = e;
        }
        const size_t at = ((size_t)cap.row0 + f) * BANDS_ROW_STRIDE + b;
        slab[at] = eq;
        if (rows) rows[at] = r;
    }
}

__global__ __launch_bounds__(256) void bands_phonemes_kernel(const int32_t *__restrict__ cum, const unsigned long long *__restrict__ slab,
                                                             float *__restrict__ rows, const uint32_t *__restrict__ par, const Segs tokens,
                                                             const Segs frames)
{
    const int u = blockIdx.y;
    const Seg tk = seg_at(tokens, u), cap = seg_at(frames, u);
    const int lane = threadIdx.x & 63;
    const int i = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (int)(threadIdx.x >> 6));
    if (i >= tk.rows) return;                                      // the whole wave
    const int nb = __builtin_amdgcn_readfirstlane((int)par[(size_t)u * BANDS_PARAM_STRIDE]);
    if (nb < 1 || nb > (int)BANDS_MAX) return;
    int start, d;
    contour_extent(cum + tk.row0, i, cap.rows, start, d);
    start = __builtin_amdgcn_readfirstlane(start);
    d = __builtin_amdgcn_readfirstlane(d);
    d = d > 0 ? d : 0;
    if (lane >= nb) return;
    const unsigned long long *sl = slab + ((size_t)cap.row0 + start) * BANDS_ROW_STRIDE + lane;      // start + d <= cap.rows
    unsigned long long sum = 0;
    for (int f = 0; f < d; f++) sum += sl[(size_t)f * BANDS_ROW_STRIDE];
    rows[((size_t)tk.row0 + i) * BANDS_ROW_STRIDE + lane] = bands_phoneme_row((uint64_t)sum, (uint64_t)d);
}

hipError_t launch_bands_frames(hipStream_t s, const float *wav, const void *table, void *slab, float *rows, const uint32_t *par, const Segs &frames,
                               int hop)
{
    if (frames.nseg < 1 || frames.max_rows < 1 || !contour_hop_supported(hop) || !wav || ((uintptr_t)wav & 15) || !table || ((uintptr_t)table & 15) || !slab || ((uintptr_t)slab & 7) ||
        ((uintptr_t)rows & 3) || !par || (!frames.tab && frames.nseg != 1))
        return hipErrorInvalidValue;
    const dim3 grid((frames.max_rows + BANDS_TILE_FRAMES - 1) / BANDS_TILE_FRAMES, frames.nseg);
    hipLaunchKernelGGL(bands_frames_kernel, grid, dim3(256), 0, s, wav, (const int8_t *)table, (unsigned long long *)slab, rows, par, frames, hop);
    return hipGetLastError();
}

hipError_t launch_bands_phonemes(hipStream_t s, const int32_t *cum, const void *slab, float *rows, const uint32_t *par, const Segs &tokens,
                                 const Segs &frames)
{
    if (frames.nseg < 1 || tokens.nseg != frames.nseg || tokens.max_rows < 1 || !cum || !slab || ((uintptr_t)slab & 7) || !rows ||
        ((uintptr_t)rows & 3) || !par || (!frames.tab && frames.nseg != 1) || (!tokens.tab && tokens.nseg != 1))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(bands_phonemes_kernel, dim3((tokens.max_rows + 3) / 4, frames.nseg), dim3(256), 0, s, cum, (const unsigned long long *)slab,
                       rows, par, tokens, frames);
    return hipGetLastError();
}

}  // namespace zv
