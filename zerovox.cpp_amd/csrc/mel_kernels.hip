// mel_kernels.hip — mel analysis: a waveform's log-mel rows, two passes over a host waveform's copy on the device (mel_frames, mel_rows;
// the arithmetic: mel.h).  A part of misc_kernels.hip's unit.
#include "kernels.h"
#include "mel.h"

namespace zv
{

// ---------------------------------------------------------------------------------------------------
// Mel analysis (kernels.h: launch_mel_frames / launch_mel_rows; the rule: mel.h).
//   frames: grid (tiles of MEL_TILE_FRAMES whole frames, segments): the band levels' frames kernel (bands_kernels.hip) with two digits on
//           the table as well, an integer GEMM [32 frames x 1024 samples] . [1024 samples x (cos | sin) of 513 bins] in four digit-plane
//           products on v_mfma_i32_16x16x64_i8.
//             1. Quantise: each of the four waves takes eight frames, one at a time.  A lane loads the 16 samples 256 q + 4 lane + j of
//                the frame's span one by one: centre is any sample of a hop and a reflected index runs backwards, so there is no aligned
//                pair as in the band levels.  Every index goes through mel_sample_index, which keeps it inside the utterance's own
//                [0, T * hop) or reads +0.0.  The next frame's loads are issued before this frame is reduced and quantised.  The two
//                digit planes of the block-scaled samples go to LDS exactly as in bands_frames_kernel (rows of 1 040 bytes).
//             2. Multiply: wave w takes the 16-bin blocks w, w + 4, ... of the 33 that hold a bin.  Per k step of 64 samples a lane loads
//                four table fragments (cos and sin of the high and the low digit plane, 16 bytes each, in fragment order:
//                mel_table_index) through a register ring and four frame fragments (two row tiles x two digit planes) from LDS, and
//                issues 16 MFMAs into 12 accumulators: per (row tile, cos / sin) hi.Chi, hi.Clo + lo.Chi (two MFMAs into one
//                accumulator) and lo.Clo.  Operand and result layouts are the band levels' (lane l: row / column l & 15, samples
//                64 step + 16 (l >> 4) + j; C/D: column = lane & 15, row = 4 (lane >> 4) + register), so cos and sin of one (frame, bin)
//                sit in the same lane and register and the magnitude (mel_magnitude, f64) is formed in place.
//             3. The 513 magnitudes of a frame go to slab[frame row][MEL_SLAB_STRIDE] in HBM (f64): 32 frames of them are 131 KB, which
//                LDS does not hold next to the planes the other waves still read.
//   rows:   grid (groups of MEL_ROWS_FRAMES frames, segments): the frames' magnitudes are staged in LDS, a thread per (frame, channel)
//           walks its channel's non-zero bins in ascending order (mel_channel) and writes the row entry (mel_level).
// Both index by ABSOLUTE frame row.  Nothing in HBM to zero: every entry that is read was stored in the same run.
constexpr int MEL_LDS_ROW = BANDS_N + 16;                          // bytes of a frame in a digit plane
constexpr int MEL_WAVE_FRAMES = MEL_TILE_FRAMES / 4;               // frames a wave quantises
constexpr int MEL_PREFETCH = 4;                                    // k steps of table fragments in flight (64 registers)
constexpr int MEL_BLOCKS = (BANDS_BINS + 15) / 16;                 // 16-bin blocks that hold a bin: 33 of the table's 34
static_assert(MEL_TILE_FRAMES == 32 && MEL_BLOCKS <= BANDS_BIN_BLOCKS, "two row tiles; the table covers the blocks");

typedef int mel_i4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void mel_frames_kernel(const float *__restrict__ wav, const int8_t *__restrict__ tab, double *__restrict__ slab,
                                                         const uint32_t *__restrict__ par, const Segs frames, int hop)
{
    __shared__ __attribute__((aligned(16))) int8_t s_a[2][MEL_TILE_FRAMES][MEL_LDS_ROW];
    __shared__ int s_k[MEL_TILE_FRAMES];
    const int u = blockIdx.y;
    const Seg cap = seg_at(frames, u);
    const int f0 = blockIdx.x * MEL_TILE_FRAMES;
    if (f0 >= cap.rows) return;                                    // the whole workgroup
    const uint32_t centre = (uint32_t)__builtin_amdgcn_readfirstlane((int)par[0]), pad = (uint32_t)__builtin_amdgcn_readfirstlane((int)par[1]);
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    // 1. quantise
    const long long n = (long long)cap.rows * hop;                 // the utterance's own samples
    const float *xs = wav + (size_t)cap.row0 * hop;
    // a frame's 16 samples of this lane; a frame behind the capacity is all zeros (and so silent)
    auto span = [&](int f, float (&x)[16]) {
        const long long s0 = mel_span((uint32_t)f, (uint32_t)hop, centre);
#pragma unroll
        for (int q = 0; q < 4; q++)
#pragma unroll
            for (int j = 0; j < 4; j++)
            {
                const long long s = mel_sample_index(s0 + q * 256 + lane * 4 + j, n, pad);
                x[q * 4 + j] = f < cap.rows && s >= 0 ? xs[s] : 0.0f;
            }
    };
    float next[16];
    span(f0 + wv * MEL_WAVE_FRAMES, next);
    for (int i = 0; i < MEL_WAVE_FRAMES; i++)
    {
        const int fl = wv * MEL_WAVE_FRAMES + i;
        float y[16];
        uint32_t pk = 0;
#pragma unroll
        for (int j = 0; j < 16; j++)
        {
            const float x = next[j];
            const uint32_t ab = level_abs_bits(x);
            y[j] = ab == (level_bits(x) & 0x7fffffffu) ? x : 0.0f;
            pk = ab > pk ? ab : pk;
        }
        // the next frame's loads are on their way while this one is reduced and quantised
        if (i + 1 < MEL_WAVE_FRAMES) span(f0 + fl + 1, next);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1)
        {
            const uint32_t q = (uint32_t)__shfl_xor((int)pk, o, 64);
            pk = q > pk ? q : pk;
        }
        const bool live = pk >= BANDS_SILENT_BITS;                 // wave uniform
        const int k = live ? bands_exponent(pk) : 0;               // a silent frame: zero planes, so every magnitude is +0.0 at any k
        const double scale = bands_pow2(k);
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
    // 2., 3. multiply, form the magnitudes and store them
    const int r16 = lane & 15, g4 = lane >> 4;
    for (int blk = wv; blk < MEL_BLOCKS; blk += 4)
    {
        mel_i4 acc[2][2][3];                                       // [row tile][cos, sin][hi.Chi | hi.Clo + lo.Chi | lo.Clo]
#pragma unroll
        for (int i = 0; i < 12; i++) (&acc[0][0][0])[i] = mel_i4{0, 0, 0, 0};
        const int8_t *tb = tab + (size_t)lane * 16;
        // the table fragments of k step ks, [digit plane][cos, sin]
        auto table = [&](int ks, mel_i4 (&B)[2][2]) {
#pragma unroll
            for (int pl = 0; pl < 2; pl++)
#pragma unroll
                for (int trig = 0; trig < 2; trig++)
                    B[pl][trig] = *(const mel_i4 *)(tb + (size_t)pl * BANDS_TABLE_BYTES + (((size_t)trig * BANDS_BIN_BLOCKS + blk) * BANDS_K_STEPS + ks) * 1024);
        };
        // a ring of MEL_PREFETCH k steps of table fragments in registers, as in bands_frames_kernel
        mel_i4 ring[MEL_PREFETCH][2][2];
#pragma unroll
        for (int ks = 0; ks < MEL_PREFETCH; ks++) table(ks, ring[ks]);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int ks = 0; ks < BANDS_K_STEPS; ks++)
        {
            mel_i4 A[2][2];
#pragma unroll
            for (int mt = 0; mt < 2; mt++)
#pragma unroll
                for (int pl = 0; pl < 2; pl++) A[mt][pl] = *(const mel_i4 *)&s_a[pl][mt * 16 + r16][ks * 64 + 16 * g4];
            mel_i4(&B)[2][2] = ring[ks % MEL_PREFETCH];
#pragma unroll
            for (int mt = 0; mt < 2; mt++)
#pragma unroll
                for (int trig = 0; trig < 2; trig++)
                {
                    acc[mt][trig][0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[mt][0], B[0][trig], acc[mt][trig][0], 0, 0, 0);
                    acc[mt][trig][1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[mt][0], B[1][trig], acc[mt][trig][1], 0, 0, 0);
                    acc[mt][trig][1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[mt][1], B[0][trig], acc[mt][trig][1], 0, 0, 0);
                    acc[mt][trig][2] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[mt][1], B[1][trig], acc[mt][trig][2], 0, 0, 0);
                }
            if (ks + MEL_PREFETCH < BANDS_K_STEPS) table(ks + MEL_PREFETCH, ring[ks % MEL_PREFETCH]);
            __builtin_amdgcn_sched_barrier(0);
        }
        const int bin = blk * 16 + r16;
#pragma unroll
        for (int mt = 0; mt < 2; mt++)
#pragma unroll
            for (int reg = 0; reg < 4; reg++)
            {
                const int fl = mt * 16 + g4 * 4 + reg, f = f0 + fl;
                const int64_t re = mel_combine(acc[mt][0][0][reg], acc[mt][0][1][reg], acc[mt][0][2][reg]);
                const int64_t im = mel_combine(acc[mt][1][0][reg], acc[mt][1][1][reg], acc[mt][1][2][reg]);
                const double g = mel_magnitude(re, im, s_k[fl]);
                if (f < cap.rows && bin < BANDS_BINS) slab[((size_t)cap.row0 + f) * MEL_SLAB_STRIDE + bin] = g;
            }
    }
}

__global__ __launch_bounds__(256) void mel_rows_kernel(const double *__restrict__ slab, float *__restrict__ rows, const uint32_t *__restrict__ par,
                                                       const Segs frames)
{
    __shared__ double s_g[MEL_ROWS_FRAMES][MEL_SLAB_STRIDE];
    const Seg cap = seg_at(frames, blockIdx.y);
    const int f0 = blockIdx.x * MEL_ROWS_FRAMES;
    if (f0 >= cap.rows) return;                                    // the whole workgroup
    const int nf = cap.rows - f0 < MEL_ROWS_FRAMES ? cap.rows - f0 : MEL_ROWS_FRAMES;
    const int M = __builtin_amdgcn_readfirstlane((int)par[4]);
    if (M < 1 || M > (int)MEL_MAX_MELS) return;                    // the host resolves and checks the block (mel_resolve)
    const uint32_t log = par[2];
    const float floor = level_from_bits(par[3]);
    const double *src = slab + ((size_t)cap.row0 + f0) * MEL_SLAB_STRIDE;      // the group's frames are consecutive rows
    for (int i = threadIdx.x; i < nf * MEL_SLAB_STRIDE; i += 256) (&s_g[0][0])[i] = src[i];
    __syncthreads();
    const float *w = (const float *)(par + MEL_PAR_WEIGHTS);
    for (int i = threadIdx.x; i < nf * M; i += 256)
    {
        const int fl = i / M, c = i - fl * M;
        uint32_t lo = par[MEL_PAR_HEAD + 2 * c], hi = par[MEL_PAR_HEAD + 2 * c + 1];
        hi = hi < (uint32_t)BANDS_BINS ? hi : (uint32_t)BANDS_BINS;
        lo = lo < hi ? lo : hi;
        const double acc = mel_channel(w + (size_t)c * BANDS_BINS, s_g[fl], lo, hi);
        rows[((size_t)cap.row0 + f0 + fl) * M + c] = mel_level(acc, floor, log);
    }
}

hipError_t launch_mel_frames(hipStream_t s, const float *wav, const void *table, double *slab, const uint32_t *par, const Segs &frames, int hop,
                             int num_mels)
{
    const MelPlan p = mel_plan(frames.max_rows, frames.nseg, hop, num_mels);
    if (!p.ok || !wav || ((uintptr_t)wav & 3) || !table || ((uintptr_t)table & 15) || !slab || ((uintptr_t)slab & 7) || !par ||
        (!frames.tab && frames.nseg != 1))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(mel_frames_kernel, dim3(p.frames_gx, p.gy), dim3(256), 0, s, wav, (const int8_t *)table, slab, par, frames, hop);
    return hipGetLastError();
}

hipError_t launch_mel_rows(hipStream_t s, const double *slab, float *rows, const uint32_t *par, const Segs &frames, int hop, int num_mels)
{
    const MelPlan p = mel_plan(frames.max_rows, frames.nseg, hop, num_mels);
    if (!p.ok || !slab || ((uintptr_t)slab & 7) || !rows || ((uintptr_t)rows & 3) || !par || (!frames.tab && frames.nseg != 1))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(mel_rows_kernel, dim3(p.rows_gx, p.gy), dim3(256), 0, s, slab, rows, par, frames);
    return hipGetLastError();
}

}  // namespace zv
