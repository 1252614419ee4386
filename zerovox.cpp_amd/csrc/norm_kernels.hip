// norm_kernels.hip — InstanceNorm over time: the f64 statistics in two steps (stats_partial, stats_finalize), norm_apply, and the
// passes that write a conv's f16 operand (norm_act_f16, act_f16), with their launchers.  A part of misc_kernels.hip's unit.
#include "kernels.h"
#include "dec_runs.h"
#include "wave_sum.h"

namespace zv
{

// ---------------------------------------------------------------------------------------------------
// InstanceNorm1d statistics over time (ggml_norm: mean and biased variance accumulated in f64, scale =
// 1/sqrtf(var + eps); reference ggml-cpu.c:6906-6923), in two steps so that no kernel ever has to walk a whole
// sequence: (1) per 32-row block and channel the f64 pair (sum x, sum x^2) — written by the conv epilogue that
// produced the tensor (conv1d_mfma.hip: tile_stats_store), by stats_partial_kernel below for tensors that come from
// elsewhere, or by norm_apply_kernel for its own output; (2) stats_finalize_kernel adds a segment's blocks in block
// order.  The reference subtracts the f32 mean before squaring (two passes); sum x^2 - (sum x)^2 / L in f64 is the
// same quantity to ~1e-12 relative, far inside the f32 rounding of the reference's own terms.
// first block of segment useg in `part`: its own run of nblk blocks, or — densely packed decoding (dec_runs.h), where the conv
// epilogues store by the block of the ONE packed segment — the global block its slot begins at
__device__ __forceinline__ size_t part_block0(const Seg &sg, int useg, int nblk, int packed)
{
    return packed ? (size_t)(sg.row0 / DEC_RUN_BLOCK) : (size_t)useg * nblk;
}

__global__ __launch_bounds__(256) void stats_partial_kernel(const float *__restrict__ x, int ldx, int C,
                                                            double *__restrict__ part, int nblk, const Segs segs, int rate, int packed)
{
    __shared__ double red[2][4][64];
    const int useg = blockIdx.z, blk = blockIdx.y;
    const Seg sg = seg_at(segs, useg);
    const int L = sg.rows * rate;
    if (blk * 32 >= L) return;
    const size_t blk0 = part_block0(sg, useg, nblk, packed);
    const int cl = threadIdx.x & 63, rg = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + cl;
    const float *xs = x + (size_t)sg.row0 * rate * ldx;
    double s1 = 0.0, s2 = 0.0;
    if (c < C)
#pragma unroll
        for (int i = 0; i < 8; i++)
        {
            const int t = blk * 32 + rg * 8 + i;
            const double v = (t < L) ? (double)xs[(size_t)t * ldx + c] : 0.0;
            s1 += v;
            s2 += v * v;
        }
    red[0][rg][cl] = s1;
    red[1][rg][cl] = s2;
    __syncthreads();
    if (rg == 0 && c < C)
    {
        const double a = (red[0][0][cl] + red[0][1][cl]) + (red[0][2][cl] + red[0][3][cl]);
        const double b = (red[1][0][cl] + red[1][1][cl]) + (red[1][2][cl] + red[1][3][cl]);
        *(double2 *)(part + ((blk0 + blk) * C + c) * 2) = make_double2(a, b);
    }
}

hipError_t launch_stats_partial(hipStream_t s, const float *x, int ldx, int C, double *part, int nblk, const Segs &segs, int rate, int packed)
{
    const int nb = (segs.max_rows * rate + 31) / 32;
    if (nb > nblk || segs.nseg < 1 || (packed && (!segs.tab || rate != 1))) return hipErrorInvalidValue;
    hipLaunchKernelGGL(stats_partial_kernel, dim3((C + 63) / 64, nb, segs.nseg), dim3(256), 0, s, x, ldx, C, part, nblk, segs, rate, packed);
    return hipGetLastError();
}

// (mean, rstd) of one channel of one segment from its blocks' partial sums, added in block order.  A decoder run table's segment
// (gap_at, G: dec_runs.h) stands for L rows, 32 G more than its nb blocks hold: the G blocks behind block gap_at - 1 were not
// computed and hold that block's pair, added where they stood.  G = 0: the plain sum.
// xtail (packed decoding, the partial sums stored by a conv over the packed rows): the segment's last block also holds guard rows
// when its nb blocks are not all whole, so that block's pair is summed from the `tail` rows of x that count, in the conv epilogue's
// order (dec_pack_tail_pair), and added where the stored pair would be: last, behind the whole blocks and the gap.
__device__ __forceinline__ float2 stats_from_partials(const double *__restrict__ p, int C, int nb, int L, float eps, int gap_at = 0, int G = 0,
                                                      const float *__restrict__ xtail = nullptr, size_t ldx = 0, int tail = 0)
{
    double s1, s2;
    if (xtail && tail > 0)
    {
        double t1, t2;
        dec_run_block_sum(p, (size_t)C * 2, nb - 1, gap_at, G, &s1, &s2);
        dec_pack_tail_pair(xtail, ldx, tail, &t1, &t2);
        s1 += t1;
        s2 += t2;
    }
    else
        dec_run_block_sum(p, (size_t)C * 2, nb, gap_at, G, &s1, &s2);
    const double mean = s1 / (double)L;
    double var = s2 / (double)L - mean * mean;
    var = var > 0.0 ? var : 0.0;
    return make_float2((float)mean, 1.0f / sqrtf((float)var + eps));
}

// the gap of segment useg when segs is a decoder run table: (blocks in front of it, blocks dropped), else (0, 0)
__device__ __forceinline__ int2 dec_run_gap(const Segs &segs, int useg, int dec_runs)
{
    if (!(dec_runs & DEC_TAB_RUNS) || !segs.tab) return make_int2(0, 0);
    return make_int2(__builtin_amdgcn_readfirstlane(segs.tab[useg].aux), __builtin_amdgcn_readfirstlane(segs.tab[useg].pad));
}

__global__ __launch_bounds__(64) void stats_finalize_kernel(const double *__restrict__ part, int nblk, int C, float eps,
                                                            float *__restrict__ stat, int stat_seg, int c_off,
                                                            const Segs segs, int rate, int dec_runs, const float *__restrict__ x, int ldx)
{
    const int useg = blockIdx.y;
    const Seg sg = seg_at(segs, useg);
    const int L = sg.rows * rate;
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= C || L <= 0) return;
    const int2 gap = dec_run_gap(segs, useg, dec_runs);
    const bool tail = (dec_runs & DEC_TAB_CONV_TAIL) && (L & 31);
    const float2 mr = stats_from_partials(part + (part_block0(sg, useg, nblk, dec_runs & DEC_TAB_PACKED) * C + c) * 2, C, (L + 31) >> 5,
                                          L + DEC_RUN_BLOCK * gap.y, eps, gap.x, gap.y,
                                          tail ? x + ((size_t)sg.row0 + (L & ~31)) * ldx + c : nullptr, (size_t)ldx, L & 31);
    float *o = stat + (size_t)useg * stat_seg + 2 * (c_off + c);
    o[0] = mr.x;
    o[1] = mr.y;
}

hipError_t launch_stats_finalize(hipStream_t s, const double *part, int nblk, int C, float eps, float *stat, int stat_seg,
                                 int c_off, const Segs &segs, int rate, int dec_runs, const float *x, int ldx)
{
    if (segs.nseg < 1 || (dec_runs && (!segs.tab || rate != 1))) return hipErrorInvalidValue;
    if ((dec_runs & DEC_TAB_CONV_TAIL) && (!(dec_runs & DEC_TAB_PACKED) || !x)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(stats_finalize_kernel, dim3((C + 63) / 64, segs.nseg), dim3(64), 0, s, part, nblk, C, eps, stat, stat_seg,
                       c_off, segs, rate, dec_runs, x, ldx);
    return hipGetLastError();
}

// y = ((x - mean) * rstd) * g + b  (affine InstanceNorm written out: the decoder's asr_res branch, reference
// src/stylettsdec.cpp:382-404) + the partial sums of y for the InstanceNorm that follows
__global__ __launch_bounds__(256) void norm_apply_kernel(const float *__restrict__ x, int ldx, int C,
                                                         const float *__restrict__ stat, int stat_seg,
                                                         const float *__restrict__ g, const float *__restrict__ b,
                                                         float *__restrict__ y, int ldy, double *__restrict__ part, int nblk,
                                                         const Segs segs, int packed)
{
    __shared__ double red[2][4][64];
    const int useg = blockIdx.z, blk = blockIdx.y;
    const Seg sg = seg_at(segs, useg);
    const int L = sg.rows;
    if (blk * 32 >= L) return;
    const int cl = threadIdx.x & 63, rg = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + cl;
    const float *xs = x + (size_t)sg.row0 * ldx;
    float *ys = y + (size_t)sg.row0 * ldy;
    double s1 = 0.0, s2 = 0.0;
    if (c < C)
    {
        const float mean = stat[(size_t)useg * stat_seg + 2 * c], rstd = stat[(size_t)useg * stat_seg + 2 * c + 1];
        const float gc = g[c], bc = b[c];
#pragma unroll
        for (int i = 0; i < 8; i++)
        {
            const int t = blk * 32 + rg * 8 + i;
            if (t < L)
            {
                float v = (xs[(size_t)t * ldx + c] - mean) * rstd;
                v = v * gc;
                v = v + bc;
                ys[(size_t)t * ldy + c] = v;
                s1 += (double)v;
                s2 += (double)v * (double)v;
            }
        }
    }
    if (!part) return;
    red[0][rg][cl] = s1;
    red[1][rg][cl] = s2;
    __syncthreads();
    if (rg == 0 && c < C)
    {
        const double a = (red[0][0][cl] + red[0][1][cl]) + (red[0][2][cl] + red[0][3][cl]);
        const double q = (red[1][0][cl] + red[1][1][cl]) + (red[1][2][cl] + red[1][3][cl]);
        *(double2 *)(part + ((part_block0(sg, useg, nblk, packed) + blk) * C + c) * 2) = make_double2(a, q);
    }
}

hipError_t launch_norm_apply(hipStream_t s, const float *x, int ldx, int C, const float *stat, int stat_seg, const float *g,
                             const float *b, float *y, int ldy, double *part, int nblk, const Segs &segs, int packed)
{
    const int nb = (segs.max_rows + 31) / 32;
    if ((part && nb > nblk) || segs.nseg < 1 || (packed && !segs.tab)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(norm_apply_kernel, dim3((C + 63) / 64, nb, segs.nseg), dim3(256), 0, s, x, ldx, C, stat, stat_seg, g, b, y,
                       ldy, part, nblk, segs, packed);
    return hipGetLastError();
}

// The conv operand of an InstanceNorm / AdaIN layer, written once: y = f16(lrelu(((x - mean) * rstd) * g + b, slope)) —
// the same operations in the same order as the conv kernel's PRO_NORM_ACT prologue, so a conv that reads y (PRO_RAW_F16)
// gives the bits of a conv that normalises on the fly.  Worth its launch when a conv re-stages its input once per group
// of output channels (the decoder's 1 056-wide convs: 9 times) — the f32 prologue then runs once instead of 9 times and the
// staging reads half the bytes.  One workgroup = 64 channels x all rows of one segment; the statistics of channels below
// Cpart are first finalised from the partial sums (exactly stats_finalize_kernel's arithmetic) and also stored in `stat`.
__global__ __launch_bounds__(256) void norm_act_f16_kernel(const float *__restrict__ x, int ldx, int C,
                                                           const double *__restrict__ part, int nblk, int Cpart, float eps,
                                                           float *__restrict__ stat, int stat_seg,
                                                           const float *__restrict__ ga, const float *__restrict__ be, int gb_seg,
                                                           float slope, _Float16 *__restrict__ y, int ldy, _Float16 *__restrict__ yraw,
                                                           const Segs segs, int dec_runs)
{
    __shared__ float sm[4][64];                  // mean, rstd, gamma, beta
    const int useg = blockIdx.y;
    const Seg sg = seg_at(segs, useg);
    const int L = sg.rows;
    if (L <= 0) return;
    const int tid = threadIdx.x;
    if (tid < 64)
    {
        const int c = blockIdx.x * 64 + tid;
        float2 mr = make_float2(0.f, 0.f);
        float g = 0.f, b = 0.f;
        if (c < C)
        {
            float *st = stat + (size_t)useg * stat_seg + 2 * c;
            if (c < Cpart)
            {
                const int2 gap = dec_run_gap(segs, useg, dec_runs);
                const bool tail = (dec_runs & DEC_TAB_CONV_TAIL) && (L & 31);
                mr = stats_from_partials(part + (part_block0(sg, useg, nblk, dec_runs & DEC_TAB_PACKED) * Cpart + c) * 2, Cpart, (L + 31) >> 5,
                                         L + DEC_RUN_BLOCK * gap.y, eps, gap.x, gap.y,
                                         tail ? x + ((size_t)sg.row0 + (L & ~31)) * ldx + c : nullptr, (size_t)ldx, L & 31);
                st[0] = mr.x;
                st[1] = mr.y;
            }
            else
                mr = make_float2(st[0], st[1]);
            g = ga[(size_t)useg * gb_seg + c];
            b = be[(size_t)useg * gb_seg + c];
        }
        sm[0][tid] = mr.x;
        sm[1][tid] = mr.y;
        sm[2][tid] = g;
        sm[3][tid] = b;
    }
    __syncthreads();
    const int c4 = (tid & 15) * 4, rl = tid >> 4;
    const int c = blockIdx.x * 64 + c4;
    if (c >= C) return;                          // C is a multiple of 4
    const float4 mean = *(const float4 *)&sm[0][c4], rstd = *(const float4 *)&sm[1][c4];
    const float4 g = *(const float4 *)&sm[2][c4], b = *(const float4 *)&sm[3][c4];
    const float *xs = x + (size_t)sg.row0 * ldx + c;
    _Float16 *ys = y + (size_t)sg.row0 * ldy + c;
    _Float16 *yr = yraw ? yraw + (size_t)sg.row0 * ldy + c : nullptr;      // f16(x): the operand of a block's 1x1 shortcut conv
    typedef _Float16 half4v __attribute__((ext_vector_type(4)));
    // densely packed decoding: zeros in the slot's guard rows [L, dec_pack_slot(L)) of every operand written here — the zero row a
    // 3-tap conv over the packed rows finds on either side of an utterance.  On every call (the buffers keep nothing between calls),
    // by the segment's first workgroup of each 64 channels
    if ((dec_runs & DEC_TAB_PACKED) && blockIdx.z == 0)
    {
        const half4v z = {0, 0, 0, 0};
        for (int t = L + rl; t < dec_pack_slot(L); t += 16)
        {
            *(half4v *)(ys + (size_t)t * ldy) = z;
            if (yr) *(half4v *)(yr + (size_t)t * ldy) = z;
        }
    }
    // the rows of a segment are dealt over gridDim.z workgroups in chunks of 128 (every one of them finalises the statistics of
    // its 64 channels for itself: the same arithmetic, the same values); eight 16-byte loads per thread in flight
    for (int t0 = blockIdx.z * 128 + rl; t0 < L; t0 += 128 * gridDim.z)
    {
        float4 v[8];
#pragma unroll
        for (int u = 0; u < 8; u++)
        {
            const int t = t0 + 16 * u;
            v[u] = *(const float4 *)(xs + (size_t)(t < L ? t : L - 1) * ldx);
        }
#pragma unroll
        for (int u = 0; u < 8; u++)
        {
            const int t = t0 + 16 * u;
            if (t >= L) continue;
            float4 r;
            r.x = ((v[u].x - mean.x) * rstd.x) * g.x + b.x;
            r.y = ((v[u].y - mean.y) * rstd.y) * g.y + b.y;
            r.z = ((v[u].z - mean.z) * rstd.z) * g.z + b.z;
            r.w = ((v[u].w - mean.w) * rstd.w) * g.w + b.w;
            half4v h;
            h[0] = (_Float16)(r.x > 0.f ? r.x : r.x * slope);
            h[1] = (_Float16)(r.y > 0.f ? r.y : r.y * slope);
            h[2] = (_Float16)(r.z > 0.f ? r.z : r.z * slope);
            h[3] = (_Float16)(r.w > 0.f ? r.w : r.w * slope);
            *(half4v *)(ys + (size_t)t * ldy) = h;
            if (yr)
            {
                half4v hr;
                hr[0] = (_Float16)v[u].x;
                hr[1] = (_Float16)v[u].y;
                hr[2] = (_Float16)v[u].z;
                hr[3] = (_Float16)v[u].w;
                *(half4v *)(yr + (size_t)t * ldy) = hr;
            }
        }
    }
}

hipError_t launch_norm_act_f16(hipStream_t s, const float *x, int ldx, int C, const double *part, int nblk, int Cpart, float eps,
                               float *stat, int stat_seg, const float *ga, const float *be, int gb_seg, float slope, void *y,
                               int ldy, const Segs &segs, void *yraw, int dec_runs)
{
    if ((C & 3) || (ldx & 3) || (ldy & 3) || segs.nseg < 1 || Cpart > C || (dec_runs && !segs.tab)) return hipErrorInvalidValue;
    if (Cpart > 0 && (segs.max_rows + 31) / 32 > nblk) return hipErrorInvalidValue;
    // (row chunks per segment: enough workgroups for about eight per CU, at most one per 128 rows)
    int gz = 1;
    while (gz < 8 && (long)((C + 63) / 64) * segs.nseg * gz < 2048 && gz * 128 < segs.max_rows) gz <<= 1;
    hipLaunchKernelGGL(norm_act_f16_kernel, dim3((C + 63) / 64, segs.nseg, gz), dim3(256), 0, s, x, ldx, C, part, nblk, Cpart, eps, stat,
                       stat_seg, ga, be, gb_seg, slope, (_Float16 *)y, ldy, (_Float16 *)yraw, segs, dec_runs);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------
// f16 operand pre-pass of the wide polyphase transposed convs of a batch (reference src/hifigan.cpp:281-297: leaky_relu in
// front of every upsample conv; the MRF mean of the previous stage, :315, rides in the same pass):
//     out[i] = f16(lrelu(((x0[i] + x1[i]) + x2[i]) * pscale, slope))          (x1 = x2 = null: x0[i] * pscale)
// — the prologue conv1d_mfma_kernel applies while it stages (PRO_ACT / PRO_SCALE_ACT / PRO_SUM3_ACT), element for element,
// so that conv_gemm_kernel can move the operand global -> LDS by DMA.
typedef _Float16 half4v __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(256) void act_f16_kernel(const float4 *__restrict__ x0, const float4 *__restrict__ x1,
                                                      const float4 *__restrict__ x2, float pscale, float slope,
                                                      half4v *__restrict__ out, size_t n4)
{
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i0 = (size_t)blockIdx.x * 256 + threadIdx.x; i0 < n4; i0 += 4 * stride)
    {
        float4 v[4], a[4], b[4];
#pragma unroll
        for (int u = 0; u < 4; u++)
        {
            const size_t i = i0 + u * stride;
            if (i >= n4) continue;
            v[u] = x0[i];
            if (x1)
            {
                a[u] = x1[i];
                b[u] = x2[i];
            }
        }
#pragma unroll
        for (int u = 0; u < 4; u++)
        {
            const size_t i = i0 + u * stride;
            if (i >= n4) continue;
            float4 x = v[u];
            if (x1)
            {
                x.x = ((x.x + a[u].x) + b[u].x) * pscale;
                x.y = ((x.y + a[u].y) + b[u].y) * pscale;
                x.z = ((x.z + a[u].z) + b[u].z) * pscale;
                x.w = ((x.w + a[u].w) + b[u].w) * pscale;
            }
            else
            {
                x.x = x.x * pscale;
                x.y = x.y * pscale;
                x.z = x.z * pscale;
                x.w = x.w * pscale;
            }
            half4v h;
            h[0] = (_Float16)(x.x > 0.f ? x.x : x.x * slope);
            h[1] = (_Float16)(x.y > 0.f ? x.y : x.y * slope);
            h[2] = (_Float16)(x.z > 0.f ? x.z : x.z * slope);
            h[3] = (_Float16)(x.w > 0.f ? x.w : x.w * slope);
            __builtin_nontemporal_store(h, out + i);
        }
    }
}

hipError_t launch_act_f16(hipStream_t s, const float *x0, const float *x1, const float *x2, float pscale, float slope, void *out,
                          size_t n)
{
    if ((n & 3) || !x0 || (!x1) != (!x2)) return hipErrorInvalidValue;
    const size_t n4 = n >> 2;
    const size_t wgs = std::min<size_t>((n4 + 1023) / 1024, (size_t)1 << 20);
    if (wgs == 0) return hipSuccess;
    hipLaunchKernelGGL(act_f16_kernel, dim3((unsigned)wgs), dim3(256), 0, s, (const float4 *)x0, (const float4 *)x1, (const float4 *)x2,
                       pscale, slope, (half4v *)out, n4);
    return hipGetLastError();
}

}  // namespace zv
