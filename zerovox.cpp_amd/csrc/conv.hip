// conv.hip — the generic conv family: fused Conv1d as implicit GEMM on gfx950 matrix cores.
//
// Replaces, per conv, the reference's 8-node ggml pattern
//     im2col(F16) -> mul_mat -> reshape -> cont(transpose) -> repeat(bias) -> add -> cont(transpose)
// (reference src/hifigan.cpp:132-140, ggml/src/ggml.c:3769-3786, ggml-cpu.c:9890-9961,7377-7554) plus
// the element-wise nodes around it (leaky_relu / norm affine / residual add / scale) with ONE launch:
//
//   stage   : a (BM + (K-1)*dil) x ck tile of the input is read once from HBM (coalesced float4 rows of
//             the channels-last layout), run through the prologue, rounded to f16 (RNE, as ggml's
//             im2col does) and parked in LDS.  No im2col matrix ever exists.
//   compute : v_mfma_f32_32x32x16_f16.  M = time, N = output channel, K = (tap, input channel).
//             A fragments are one ds_read_b128 each (8 consecutive channels of one time step; row
//             stride ck*2+16 B makes the 16-lane read groups bank-conflict free); B fragments stream
//             straight from L2 into registers — weights were re-laid-out at load time so that one
//             fragment is 1 KiB contiguous — with a 4-step register prefetch.  Each wave owns a
//             (32*MT) x 32 output tile so one B fragment feeds MT MFMAs.
//   epilogue: bias, residual add, scale, activation, f32 or f16 store (128-B segments per half-wave).
//
// Several independent convs that share a tile configuration (the three MRF branches of a HiFi-GAN
// stage) ride in one launch as "jobs" (blockIdx.z) so that a 512-frame utterance still fills 256 CUs.
//
// Also here: conv_stream_kernel (the memory-bound upsample convs of a batch) and out_conv_tanh_kernel (the vocoder's
// output conv).  The wide decoder convs of a batch run on conv_gemm_kernel (conv_gemm.hip), which launch_conv picks.
#include "conv_xcd.h"
#include "kernels.h"
#include "knobs.h"
#include "mfma_common.h"

#include <hip/hip_fp16.h>
#include <algorithm>
#include <cstdlib>
#include <cstring>

namespace zv
{

static constexpr int CK_MAX = 256;
// 16-byte pieces a thread keeps in flight while it stages a tile (10 — one round trip for every small tile — measured no
// faster on the batch's upsample convs and costs the MT = 1 kernels a wave of occupancy)
#ifndef ZV_STAGE_U
#define ZV_STAGE_U 4
#endif
// ... in the single-utterance form of the generic kernel (one workgroup per CU at most: occupancy is not the price there): the
// 34-row x 256-channel f32 tile of a chunk in one round trip instead of three
#ifndef ZV_STAGE_US
#define ZV_STAGE_US 9
#endif
// ... and its loader waves (ZV_SINGLE_LW of them, conv_plan.h)
#ifndef ZV_STAGE_ULW
#define ZV_STAGE_ULW 10
#endif
// waves per SIMD the 64 x 64 wave-tile instantiation of the generic conv kernel is compiled for (3: 168 registers)
#ifndef ZV_NT2_OCC
#define ZV_NT2_OCC 3
#endif

int conv_pick_ck(int Cin_p, int ck_max)
{
    if (ck_max <= 0 || ck_max > CK_MAX) ck_max = CK_MAX;
    // full 256-channel chunks (they run on the immediate-address MFMA loop; fewer stage/barrier rounds per conv)
    // + one remainder chunk
    return Cin_p < ck_max ? Cin_p : ck_max;
}

size_t packed_conv_weight_halfs(int Cin_p, int Cout_p, int K)
{
    return (size_t)((Cout_p + 31) / 32) * K * (Cin_p / 16) * 512;
}

// dst[(((nt*K*nicb) + K*(c0/16) + tap*nkc_chunk + kc) * 64 + lane) * 8 + j]
//   = w[oc = nt*32 + (lane&31)][ic = c0 + kc*16 + 8*(lane>>5) + j][tap]      (0 outside IC/OC)
// i.e. the B-operand fragment of v_mfma_f32_32x32x16_f16: lane l holds B[k = 8*(l>>5) + j][col = l&31].
void pack_conv_weight(const uint16_t *w, int K, int IC, int OC, int Cin_p, int Cout_p, int ck, uint16_t *dst)
{
    const int ntiles = (Cout_p + 31) / 32, nicb = Cin_p / 16;
    for (int nt = 0; nt < ntiles; nt++)
        for (int c0 = 0; c0 < Cin_p; c0 += ck)
        {
            const int nkc = ((Cin_p - c0 < ck) ? (Cin_p - c0) : ck) / 16;
            for (int tap = 0; tap < K; tap++)
                for (int kc = 0; kc < nkc; kc++)
                {
                    size_t blk = (size_t)nt * K * nicb + (size_t)K * (c0 / 16) + (size_t)tap * nkc + kc;
                    uint16_t *d = dst + blk * 512;
                    for (int lane = 0; lane < 64; lane++)
                        for (int j = 0; j < 8; j++)
                        {
                            int oc = nt * 32 + (lane & 31);
                            int ic = c0 + kc * 16 + 8 * (lane >> 5) + j;
                            d[lane * 8 + j] = (oc < OC && ic < IC) ? w[((size_t)oc * IC + ic) * K + tap] : (uint16_t)0;
                        }
                }
        }
}

// ---- stage: HBM -> prologue -> f16 -> LDS.  U independent 16-byte loads per thread are issued before any of
// them is consumed (hipcc otherwise waits vmcnt(0) after every load and the tile fill becomes a chain of
// full HBM latencies).  LDS row r holds input time row_t0 + r; out-of-range rows are zeros.
// what the staging loop reads: the job's input with every pointer already advanced to the workgroup's segment
struct StageSrc
{
    const void  *x0, *x1, *x2;
    const float *pa, *pb, *pstat;
    int          ldx, L;
    float        slope, pscale;
};

template <int U, int PRO, int NTH = 256>
__device__ __forceinline__ void stage_tile_p(const StageSrc &J, char *smem, int RS, int c0, int ck, int row_t0, int rows,
                                             int tid)
{
    const int cols = ck >> 2;
    const int total = rows * cols;
    const int L = J.L;
    constexpr int pro = PRO;
    int r = tid / cols, c4 = tid - r * cols;
    const int dr = NTH / cols, dc = NTH - dr * cols;
    // cols divides NTH (every 256- / 128- / 64- / 32- / 16-channel chunk): all of a thread's pieces are one column group, its
    // per-channel vectors are loaded once (9 pieces x 4 vectors were 36 more loads per thread and chunk)
    const bool hoist = dc == 0;
    float4 hp0 = {0, 0, 0, 0}, hp1 = hp0, hp2 = hp0, hp3 = hp0;
    if (hoist)
    {
        const int c = c0 + c4 * 4;
        if constexpr (pro == PRO_NORM_ACT)
        {
            hp0 = *(const float4 *)(J.pstat + 2 * c);
            hp1 = *(const float4 *)(J.pstat + 2 * c + 4);
            hp2 = *(const float4 *)(J.pa + c);
            hp3 = *(const float4 *)(J.pb + c);
        }
        else if constexpr (pro == PRO_MELNORM)
        {
            hp2 = *(const float4 *)(J.pa + c);
            hp3 = *(const float4 *)(J.pb + c);
        }
    }
    for (int base = tid; base < total; base += NTH * U)
    {
        float4 v[U], v1[U], v2[U];
        half4 hraw[U];
        int lofs[U];
        bool live[U], inr[U];
#pragma unroll
        for (int u = 0; u < U; u++)
        {
            live[u] = base + u * NTH < total;
            const int t = row_t0 + r;
            inr[u] = live[u] && t >= 0 && t < L;
            lofs[u] = r * RS + c4 * 8;
            const size_t off = (size_t)(inr[u] ? t : 0) * J.ldx + c0 + c4 * 4;
            if constexpr (pro == PRO_RAW_F16)
                hraw[u] = *(const half4 *)((const _Float16 *)J.x0 + off);
            else
            {
                v[u] = *(const float4 *)((const float *)J.x0 + off);
                if constexpr (pro == PRO_SUM3_ACT)
                {
                    v1[u] = *(const float4 *)((const float *)J.x1 + off);
                    v2[u] = *(const float4 *)((const float *)J.x2 + off);
                }
            }
            r += dr;
            c4 += dc;
            if (c4 >= cols) { c4 -= cols; r++; }
        }
#pragma unroll
        for (int u = 0; u < U; u++)
        {
            if (!live[u]) continue;
            half4 h = {0, 0, 0, 0};
            if (inr[u])
            {
                if constexpr (pro == PRO_RAW_F16)
                    h = hraw[u];
                else
                {
                    float4 x = v[u];
                    const int c = c0 + ((lofs[u] % RS) >> 1);
                    (void)c;
                    if constexpr (pro == PRO_SUM3_ACT)
                    {
                        const float sc = J.pscale;
                        x.x = ((x.x + v1[u].x) + v2[u].x) * sc;
                        x.y = ((x.y + v1[u].y) + v2[u].y) * sc;
                        x.z = ((x.z + v1[u].z) + v2[u].z) * sc;
                        x.w = ((x.w + v1[u].w) + v2[u].w) * sc;
                    }
                    else if constexpr (pro == PRO_SCALE_ACT)
                    {
                        const float sc = J.pscale;
                        x.x = x.x * sc;
                        x.y = x.y * sc;
                        x.z = x.z * sc;
                        x.w = x.w * sc;
                    }
                    else if constexpr (pro == PRO_NORM_ACT)
                    {
                        float4 st0 = hp0, st1 = hp1, g = hp2, b = hp3;               // st: mean,rstd,mean,rstd
                        if (!hoist)
                        {
                            st0 = *(const float4 *)(J.pstat + 2 * c);
                            st1 = *(const float4 *)(J.pstat + 2 * c + 4);
                            g = *(const float4 *)(J.pa + c);
                            b = *(const float4 *)(J.pb + c);
                        }
                        x.x = ((x.x - st0.x) * st0.y) * g.x + b.x;
                        x.y = ((x.y - st0.z) * st0.w) * g.y + b.y;
                        x.z = ((x.z - st1.x) * st1.y) * g.z + b.z;
                        x.w = ((x.w - st1.z) * st1.w) * g.w + b.w;
                    }
                    else if constexpr (pro == PRO_MELNORM)
                    {
                        float4 a = hp2, b = hp3;
                        if (!hoist)
                        {
                            a = *(const float4 *)(J.pa + c);
                            b = *(const float4 *)(J.pb + c);
                        }
                        x.x = (x.x - a.x) / b.x;
                        x.y = (x.y - a.y) / b.y;
                        x.z = (x.z - a.z) / b.z;
                        x.w = (x.w - a.w) / b.w;
                    }
                    if constexpr (pro != PRO_MELNORM)
                    {
                        const float sl = J.slope;
                        x.x = lrelu(x.x, sl);
                        x.y = lrelu(x.y, sl);
                        x.z = lrelu(x.z, sl);
                        x.w = lrelu(x.w, sl);
                    }
                    h[0] = (_Float16)x.x;      // v_cvt_f16_f32: round-to-nearest-even, like _cvtss_sh(x, 0)
                    h[1] = (_Float16)x.y;
                    h[2] = (_Float16)x.z;
                    h[3] = (_Float16)x.w;
                }
            }
            *(half4 *)(smem + lofs[u]) = h;
        }
    }
}

// The same fill in two halves for the loader waves of the single-utterance kernel: stage_load_p requests a whole tile (at most
// NTH * U pieces) into registers, stage_store_p applies the prologue and writes LDS — a barrier may sit between the two.  Same
// operations per element as stage_tile_p.
template <int U>
struct StageRegs
{
    float4 v[U];
    float4 p0, p1, p2, p3;      // the thread's per-channel vectors (when all its pieces are one column group)
};
template <int U, int PRO, int NTH>
__device__ __forceinline__ void stage_load_p(const StageSrc &J, int c0, int ck, int row_t0, int rows, int tid, StageRegs<U> &R)
{
    // (an f16 operand tensor travels in 16-byte pieces of 8 channels, everything else in pieces of 4 channels)
    constexpr int PW = PRO == PRO_RAW_F16 ? 8 : 4;
    const int cols = ck / PW, total = rows * cols, L = J.L;
    int r = tid / cols, c4 = tid - r * cols;
    const int dr = NTH / cols, dc = NTH - dr * cols;
    if (dc == 0)
    {
        const int c = c0 + c4 * 4;
        if constexpr (PRO == PRO_NORM_ACT)
        {
            R.p0 = *(const float4 *)(J.pstat + 2 * c);
            R.p1 = *(const float4 *)(J.pstat + 2 * c + 4);
        }
        if constexpr (PRO == PRO_NORM_ACT || PRO == PRO_MELNORM)
        {
            R.p2 = *(const float4 *)(J.pa + c);
            R.p3 = *(const float4 *)(J.pb + c);
        }
    }
#pragma unroll
    for (int u = 0; u < U; u++)
    {
        const int t = row_t0 + r;
        const bool inr = tid + u * NTH < total && t >= 0 && t < L;
        const size_t off = (size_t)(inr ? t : 0) * J.ldx + c0 + c4 * PW;
        if constexpr (PRO == PRO_RAW_F16)
            R.v[u] = *(const float4 *)((const _Float16 *)J.x0 + off);
        else
            R.v[u] = *(const float4 *)((const float *)J.x0 + off);
        r += dr;
        c4 += dc;
        if (c4 >= cols) { c4 -= cols; r++; }
    }
}
template <int U, int PRO, int NTH>
__device__ __forceinline__ void stage_store_p(const StageSrc &J, char *smem, int RS, int c0, int ck, int row_t0, int rows, int tid,
                                              const StageRegs<U> &R)
{
    constexpr int PW = PRO == PRO_RAW_F16 ? 8 : 4;
    const int cols = ck / PW, total = rows * cols, L = J.L;
    int r = tid / cols, c4 = tid - r * cols;
    const int dr = NTH / cols, dc = NTH - dr * cols;
    const bool hoist = dc == 0;
    const float4 hp0 = R.p0, hp1 = R.p1, hp2 = R.p2, hp3 = R.p3;
#pragma unroll
    for (int u = 0; u < U; u++)
    {
        const int t = row_t0 + r;
        const bool live = tid + u * NTH < total;
        const bool inr = live && t >= 0 && t < L;
        const int lofs = r * RS + c4 * 2 * PW;
        if constexpr (PRO == PRO_RAW_F16)
        {
            if (live) *(float4 *)(smem + lofs) = inr ? R.v[u] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        else if (live)
        {
            half4 h = {0, 0, 0, 0};
            if (inr)
            {
                if constexpr (PRO == PRO_RAW_F16)
                {
                }
                else
                {
                    float4 x = R.v[u];
                    const int c = c0 + c4 * 4;
                    (void)c;
                    if constexpr (PRO == PRO_SCALE_ACT)
                    {
                        const float sc = J.pscale;
                        x.x = x.x * sc;
                        x.y = x.y * sc;
                        x.z = x.z * sc;
                        x.w = x.w * sc;
                    }
                    else if constexpr (PRO == PRO_NORM_ACT)
                    {
                        float4 st0 = hp0, st1 = hp1, g = hp2, b = hp3;               // st: mean,rstd,mean,rstd
                        if (!hoist)
                        {
                            st0 = *(const float4 *)(J.pstat + 2 * c);
                            st1 = *(const float4 *)(J.pstat + 2 * c + 4);
                            g = *(const float4 *)(J.pa + c);
                            b = *(const float4 *)(J.pb + c);
                        }
                        x.x = ((x.x - st0.x) * st0.y) * g.x + b.x;
                        x.y = ((x.y - st0.z) * st0.w) * g.y + b.y;
                        x.z = ((x.z - st1.x) * st1.y) * g.z + b.z;
                        x.w = ((x.w - st1.z) * st1.w) * g.w + b.w;
                    }
                    else if constexpr (PRO == PRO_MELNORM)
                    {
                        float4 a = hp2, b = hp3;
                        if (!hoist)
                        {
                            a = *(const float4 *)(J.pa + c);
                            b = *(const float4 *)(J.pb + c);
                        }
                        x.x = (x.x - a.x) / b.x;
                        x.y = (x.y - a.y) / b.y;
                        x.z = (x.z - a.z) / b.z;
                        x.w = (x.w - a.w) / b.w;
                    }
                    if constexpr (PRO != PRO_MELNORM)
                    {
                        const float sl = J.slope;
                        x.x = lrelu(x.x, sl);
                        x.y = lrelu(x.y, sl);
                        x.z = lrelu(x.z, sl);
                        x.w = lrelu(x.w, sl);
                    }
                    h[0] = (_Float16)x.x;
                    h[1] = (_Float16)x.y;
                    h[2] = (_Float16)x.z;
                    h[3] = (_Float16)x.w;
                }
            }
            *(half4 *)(smem + lofs) = h;
        }
        r += dr;
        c4 += dc;
        if (c4 >= cols) { c4 -= cols; r++; }
    }
}
#define ZV_STAGE_SPLIT_SWITCH(pro, CALL)                       \
    switch (pro)                                               \
    {                                                          \
        case PRO_RAW_F16: CALL(PRO_RAW_F16); break;            \
        case PRO_ACT: CALL(PRO_ACT); break;                    \
        case PRO_NORM_ACT: CALL(PRO_NORM_ACT); break;          \
        case PRO_MELNORM: CALL(PRO_MELNORM); break;            \
        default: CALL(PRO_SCALE_ACT); break;                   \
    }

template <int U, int NTH = 256>
__device__ __forceinline__ void stage_tile(int pro, const StageSrc &J, char *smem, int RS, int c0, int ck, int row_t0, int rows,
                                           int tid)
{
    switch (pro)        // wave-uniform; each case is a straight-line batched fill
    {
        case PRO_RAW_F16: stage_tile_p<U, PRO_RAW_F16, NTH>(J, smem, RS, c0, ck, row_t0, rows, tid); break;
        case PRO_ACT: stage_tile_p<U, PRO_ACT, NTH>(J, smem, RS, c0, ck, row_t0, rows, tid); break;
        case PRO_NORM_ACT: stage_tile_p<U, PRO_NORM_ACT, NTH>(J, smem, RS, c0, ck, row_t0, rows, tid); break;
        case PRO_MELNORM: stage_tile_p<U, PRO_MELNORM, NTH>(J, smem, RS, c0, ck, row_t0, rows, tid); break;
        case PRO_SCALE_ACT: stage_tile_p<U, PRO_SCALE_ACT, NTH>(J, smem, RS, c0, ck, row_t0, rows, tid); break;
        default: stage_tile_p<(U > 4 ? 4 : U), PRO_SUM3_ACT, NTH>(J, smem, RS, c0, ck, row_t0, rows, tid); break;   // three tensors per piece
    }
}

// PRO_RAW_F16 in 16-byte pieces (8 channels) for NTH threads: every load of a round is in flight before the first is
// stored (U x 16 B per thread), so a tile of <= NTH * U pieces costs one round trip.
template <int U, int NTH>
__device__ __forceinline__ void stage_raw16(const StageSrc &J, char *smem, int RS, int c0, int ck, int row_t0, int rows, int tid)
{
    const int cols = ck >> 3;
    const int total = rows * cols;
    const int L = J.L;
    int r = tid / cols, c8 = tid - r * cols;
    const int dr = NTH / cols, dc = NTH - dr * cols;
    for (int base = tid; base < total; base += NTH * U)
    {
        uint4 v[U];
        int lofs[U];
        bool live[U], inr[U];
#pragma unroll
        for (int u = 0; u < U; u++)
        {
            live[u] = base + u * NTH < total;
            const int t = row_t0 + r;
            inr[u] = live[u] && t >= 0 && t < L;
            lofs[u] = r * RS + c8 * 16;
            v[u] = *(const uint4 *)((const _Float16 *)J.x0 + (size_t)(inr[u] ? t : 0) * J.ldx + c0 + c8 * 8);
            r += dr;
            c8 += dc;
            if (c8 >= cols) { c8 -= cols; r++; }
        }
#pragma unroll
        for (int u = 0; u < U; u++)
            if (live[u]) *(uint4 *)(smem + lofs[u]) = inr[u] ? v[u] : make_uint4(0, 0, 0, 0);
    }
}

// ---- compute: S = K * nkc MFMA steps over one staged chunk.  A fragments are double-buffered in registers
// (the ds_reads of step s+1 are in flight while the MFMAs of step s run), B fragments come from L2 through a
// 4-deep register ring.
template <int MT, int NT>
__device__ __forceinline__ void mfma_chunk(floatx16 (&acc)[MT][NT], const char *abase, int RS, int dil, const half8 *wp,
                                           size_t wseg, int K, int nkc)
{
    // Branch-free, 4 steps per iteration with static register slots so that hipcc can count its waits: the B
    // fragment consumed in slot u was requested four steps earlier (s_waitcnt vmcnt(3)), the A fragments one step
    // earlier.  Steps S..round_up(S,4)-1 do not exist: they run with B = 0 (adds nothing) on a clamped A address.
    const int S = K * nkc;
    const half8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
    half8 b[4][NT];
#pragma unroll
    for (int u = 0; u < 4; u++)
#pragma unroll
        for (int nt = 0; nt < NT; nt++) b[u][nt] = wp[nt * wseg + (size_t)((u < S) ? u : S - 1) * 64];
    half8 a[MT];
#pragma unroll
    for (int mt = 0; mt < MT; mt++) a[mt] = *(const half8 *)(abase + mt * 32 * RS);
    int tap = 0, kc = 0;
    for (int s0 = 0; s0 < S; s0 += 4)
    {
#pragma unroll
        for (int u = 0; u < 4; u++)
        {
            if (++kc == nkc) { kc = 0; tap++; }
            if (tap >= K) tap = 0;                   // past the last step: any valid address
            const char *ap = abase + tap * dil * RS + kc * 32;
            half8 an[MT];
#pragma unroll
            for (int mt = 0; mt < MT; mt++) an[mt] = *(const half8 *)(ap + mt * 32 * RS);
#pragma unroll
            for (int nt = 0; nt < NT; nt++)
            {
                const half8 bu = (s0 + u < S) ? b[u][nt] : zero8;
#pragma unroll
                for (int mt = 0; mt < MT; mt++)
                    acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[mt], bu, acc[mt][nt], 0, 0, 0);
            }
            const int sn = s0 + u + 4;
#pragma unroll
            for (int nt = 0; nt < NT; nt++) b[u][nt] = wp[nt * wseg + (size_t)((sn < S) ? sn : S - 1) * 64];
#pragma unroll
            for (int mt = 0; mt < MT; mt++) a[mt] = an[mt];
        }
    }
}

// One body = 8 MFMA steps = 8 / (CP/16) taps (half a tap for CP = 256).  Two static B register sets ping-pong
// (b0: steps 0-3, b1: steps 4-7), each refilled for the next body right after its last use; A fragments ping-pong
// one step ahead.  All LDS and weight addresses inside a body are immediates off the body's base.  A wave covers
// NT output tiles of 32 channels (their weight segments are `wseg` half8 apart) and MT row tiles.
template <int CP, int MT, int NT, bool SWAP>
__device__ __forceinline__ void mfma_taps(floatx16 (&acc)[MT][NT], const char *ap, int dilRS, const half8 *wq, size_t wseg, int K)
{
    constexpr int RS = CP * 2 + 16, NKC = CP / 16;
    constexpr int TPB = (NKC >= 8) ? 1 : 8 / NKC;        // taps per body: 4 / 2 / 1 / (1/2) for CP = 32 / 64 / 128 / 256
    constexpr bool HALF = NKC == 16;                     // CP = 256: a tap is two bodies (channels 0-127, 128-255)
    const int nsb = (K * NKC + 3) >> 2;                  // 4-step sub-blocks (the last one may run partly on zero weights)
    const int nb = nsb >> 1;
    half8 b0[4][NT], b1[4][NT];
#pragma unroll
    for (int u = 0; u < 4; u++)
#pragma unroll
        for (int nt = 0; nt < NT; nt++) b0[u][nt] = wq[nt * wseg + u * 64];
    wq += 4 * 64;
    half8 a0[MT], a1[MT];
#pragma unroll
    for (int mt = 0; mt < MT; mt++) a0[mt] = *(const half8 *)(ap + mt * 32 * RS);

#define ZV_A_ADDR(un) ((un) == 8 ? apn : tb[((un) / NKC) % 4] + ((un) % NKC) * 32)
#define ZV_LOAD_A(dst, un)                                                                   \
    {                                                                                        \
        const char *np_ = ZV_A_ADDR(un);                                                     \
        _Pragma("unroll") for (int mt = 0; mt < MT; mt++) dst[mt] = *(const half8 *)(np_ + mt * 32 * RS); \
    }
    for (int ib = 0; ib < nb; ib++)
    {
        const char *tb[4];
        tb[0] = ap;
#pragma unroll
        for (int x = 1; x < 4; x++) tb[x] = (x < TPB) ? ap + x * dilRS : ap;
        const char *apn = HALF ? ((ib & 1) ? ap + (dilRS - 256) : ap + 256) : ap + TPB * dilRS;   // next body
#pragma unroll
        for (int u = 0; u < 4; u++)
#pragma unroll
            for (int nt = 0; nt < NT; nt++) b1[u][nt] = wq[nt * wseg + u * 64];      // steps 4..7 of this body
        __builtin_amdgcn_sched_barrier(0);      // keep the requests here: hipcc otherwise sinks them next to their use
        ZV_LOAD_A(a1, 1) mfma_step<MT, NT, SWAP>(acc, a0, b0[0]);
        ZV_LOAD_A(a0, 2) mfma_step<MT, NT, SWAP>(acc, a1, b0[1]);
        ZV_LOAD_A(a1, 3) mfma_step<MT, NT, SWAP>(acc, a0, b0[2]);
        ZV_LOAD_A(a0, 4) mfma_step<MT, NT, SWAP>(acc, a1, b0[3]);
#pragma unroll
        for (int u = 0; u < 4; u++)
#pragma unroll
            for (int nt = 0; nt < NT; nt++) b0[u][nt] = wq[nt * wseg + (4 + u) * 64];   // steps 0..3 of the next body
        __builtin_amdgcn_sched_barrier(0);
        ZV_LOAD_A(a1, 5) mfma_step<MT, NT, SWAP>(acc, a0, b1[0]);
        ZV_LOAD_A(a0, 6) mfma_step<MT, NT, SWAP>(acc, a1, b1[1]);
        ZV_LOAD_A(a1, 7) mfma_step<MT, NT, SWAP>(acc, a0, b1[2]);
        ZV_LOAD_A(a0, 8) mfma_step<MT, NT, SWAP>(acc, a1, b1[3]);
        ap = apn;
        wq += 8 * 64;
    }
    if (nsb & 1)                                 // odd sub-block count (CP = 64): one more tap on b0
    {
        const char *tb[4] = {ap, ap, ap, ap};
        const char *apn = ap;
        (void)apn;
        ZV_LOAD_A(a1, 1) mfma_step<MT, NT, SWAP>(acc, a0, b0[0]);
        ZV_LOAD_A(a0, 2) mfma_step<MT, NT, SWAP>(acc, a1, b0[1]);
        ZV_LOAD_A(a1, 3) mfma_step<MT, NT, SWAP>(acc, a0, b0[2]);
        mfma_step<MT, NT, SWAP>(acc, a1, b0[3]);
    }
#undef ZV_LOAD_A
#undef ZV_A_ADDR
}


// mfma_taps with ONE set of four weight-fragment slots: the slot a step has consumed is refilled at once with the fragment
// of four steps later (same prefetch distance as the two ping-pong sets above, half their registers: the 64 x 64 wave tile
// then fits 168 registers = three workgroups per CU instead of two).  Same step order, same bits.
template <int CP, int MT, int NT>
__device__ __forceinline__ void mfma_taps_ring4(floatx16 (&acc)[MT][NT], const char *ap, int dilRS, const half8 *wq, size_t wseg, int K)
{
    constexpr int RS = CP * 2 + 16, NKC = CP / 16;
    static_assert(NKC >= 8, "whole 8-step bodies per tap");
    constexpr bool HALF = NKC == 16;
    const int nb = (K * NKC) >> 3;
    half8 b[4][NT];
#pragma unroll
    for (int u = 0; u < 4; u++)
#pragma unroll
        for (int nt = 0; nt < NT; nt++) b[u][nt] = wq[nt * wseg + u * 64];
    half8 a0[MT], a1[MT];
#pragma unroll
    for (int mt = 0; mt < MT; mt++) a0[mt] = *(const half8 *)(ap + mt * 32 * RS);
#define ZV_R4_LOADA(dst, un)                                                                  \
    {                                                                                         \
        const char *np_ = (un) == 8 ? apn : ap + (un) * 32;                                   \
        _Pragma("unroll") for (int mt = 0; mt < MT; mt++) dst[mt] = *(const half8 *)(np_ + mt * 32 * RS); \
    }
#define ZV_R4_STEP(u, acur, anext)                                                            \
    ZV_R4_LOADA(anext, (u) + 1)                                                               \
    mfma_step<MT, NT, false>(acc, acur, b[(u) & 3]);                                          \
    _Pragma("unroll") for (int nt = 0; nt < NT; nt++) b[(u) & 3][nt] = wq[nt * wseg + ((u) + 4) * 64]; \
    __builtin_amdgcn_sched_barrier(0);
    for (int ib = 0; ib < nb; ib++)
    {
        const char *apn = HALF ? ((ib & 1) ? ap + (dilRS - 256) : ap + 256) : ap + dilRS;   // next body
        ZV_R4_STEP(0, a0, a1) ZV_R4_STEP(1, a1, a0) ZV_R4_STEP(2, a0, a1) ZV_R4_STEP(3, a1, a0)
        ZV_R4_STEP(4, a0, a1) ZV_R4_STEP(5, a1, a0) ZV_R4_STEP(6, a0, a1) ZV_R4_STEP(7, a1, a0)
        ap = apn;
        wq += 8 * 64;
    }
#undef ZV_R4_STEP
#undef ZV_R4_LOADA
}

// The MFMA loop of a full 256-channel chunk for single-utterance launches (MT row tiles x ONE output tile per wave, one
// wave per SIMD, at most a round of workgroups: registers are free, latency is everything).  A step is MT MFMAs — 32
// cycles at MT = 1 — so the loops above, whose A fragment is requested one step ahead (an LDS round trip per step) and
// whose weight fragments 4-8 steps ahead (an L2 round trip per 4 steps), take 75 ns per step (phase stamps: 3.6 us per
// chunk for 0.8 us of matrix work).  Here one body = one tap = 16 steps, every address an immediate off the body's base,
// the A fragments travel 6 steps ahead through a ring of 8 register sets and the weight fragments 16 steps ahead through
// a ring of 16 that is carried from chunk to chunk (the generic layout puts the next chunk's first tap right behind this
// chunk's last: the caller preloads the ring once, before the first tile is even staged; the last tap's requests run up
// to 16 KiB past the chunk — load_conv / load_upsample allocate that slack).  Same step order as mfma_taps<256> /
// mfma_chunk — tap-major, 16 channels per step — hence the same bits.  (Measured: 2.8 us per chunk, 1.7 us where the
// weights hit L2; a conv of 33 us becomes 29.6 us.  What is left is the cold weights — every row tile of a channel group
// misses on them together — and the staging round trips between the loops.)
template <int MT>
__device__ __forceinline__ void preload_ring16(half8 (&b)[16], const half8 *wq)
{
#pragma unroll
    for (int u = 0; u < 16; u++) b[u] = wq[u * 64];
}

template <int MT>
__device__ __forceinline__ void mfma_taps_single256(floatx16 (&acc)[MT][1], const char *ap, int dilRS, const half8 *wq, int K,
                                                    half8 (&b)[16])
{
    constexpr int RS = 256 * 2 + 16;
    half8 a[8][MT];
#define ZV_SA(un) (((un) >= 16 ? apn : ap) + ((un) & 15) * 32)
#define ZV_SLOAD(un)                                                                              \
    {                                                                                             \
        const char *np_ = ZV_SA(un);                                                              \
        _Pragma("unroll") for (int mt = 0; mt < MT; mt++) a[(un) & 7][mt] = *(const half8 *)(np_ + mt * 32 * RS); \
    }
#define ZV_SSTEP(u)                                                                               \
    {                                                                                             \
        half8 ac_[MT];                                                                            \
        _Pragma("unroll") for (int mt = 0; mt < MT; mt++) ac_[mt] = a[(u) & 7][mt];               \
        ZV_SLOAD((u) + 6)                                                                         \
        _Pragma("unroll") for (int mt = 0; mt < MT; mt++)                                         \
            acc[mt][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ac_[mt], b[u], acc[mt][0], 0, 0, 0); \
        b[u] = wq[(16 + (u)) * 64];                                                               \
        __builtin_amdgcn_sched_barrier(0);                                                        \
    }
    {
        const char *apn = ap;
        ZV_SLOAD(0) ZV_SLOAD(1) ZV_SLOAD(2) ZV_SLOAD(3) ZV_SLOAD(4) ZV_SLOAD(5)
    }
    for (int tap = 0; tap < K; tap++)
    {
        const char *apn = ap + dilRS;
        ZV_SSTEP(0) ZV_SSTEP(1) ZV_SSTEP(2) ZV_SSTEP(3) ZV_SSTEP(4) ZV_SSTEP(5) ZV_SSTEP(6) ZV_SSTEP(7)
        ZV_SSTEP(8) ZV_SSTEP(9) ZV_SSTEP(10) ZV_SSTEP(11) ZV_SSTEP(12) ZV_SSTEP(13) ZV_SSTEP(14) ZV_SSTEP(15)
        ap = apn;
        wq += 16 * 64;
    }
#undef ZV_SSTEP
#undef ZV_SLOAD
#undef ZV_SA
}

// Each wave owns (32*MT) rows x (32*NT) output channels: NT = 2 halves the LDS reads per MFMA (an A fragment feeds two
// MFMAs) and lets a workgroup cover 256 output channels, so a wide conv stages its input half as often.
// (Measured dead end, round 2: the staged tile double-buffered in LDS and filled by LDS-DMA while the MFMA loop of the
// previous chunk runs.  hipcc answers an LDS-DMA in flight with vmcnt(0) waits on the B-fragment stream of the MFMA
// loop — the counted waits that keep eight fragments in flight are gone — and the wide decoder convs ran 3 % slower.)
// (Measured dead end, round 3: two extra "loader" waves staging chunk c + 1 into a second LDS tile under the MFMA loop of chunk c:
// decoder convs 311 -> 378 us; removed in round 4.)
// Single-utterance convs: every row tile of a channel group walks the same weight stream in step, so each fragment is an L2 miss
// for all of them together (a memory-side round trip per ring refill).  The group's row tiles sit on ONE XCD (see the kernels), so they
// warm its L2 together first: workgroup `part` of `nparts` touches its slice of the group's weight bytes, one 4-byte load per
// 128-byte line (64 lines = 8 KiB per wave instruction, 256 bytes returned).  The result is discarded; nothing waits for it.
__device__ __forceinline__ void l2_warm(const void *base, size_t bytes, int part, int nparts, int tid, int nth)
{
    const size_t lines = (bytes + 127) >> 7;
    const size_t per = (lines + nparts - 1) / nparts, l0 = (size_t)part * per;
    const size_t l1 = l0 + per < lines ? l0 + per : lines;
    unsigned sink = 0;
    for (size_t l = l0 + tid; l < l1; l += nth) sink ^= *(const volatile unsigned *)((const char *)base + (l << 7));
    asm volatile("" ::"v"(sink));
}

template <int MT, int WN, int NT, bool SINGLE = false>
__global__ __launch_bounds__(SINGLE ? 256 + 64 * ZV_SINGLE_LW : 256, (NT == 2 && ZV_NT2_OCC == 3) ? 3 : 2) void conv1d_mfma_kernel(const ConvJobs jobs)
{
    constexpr int WM = 4 / WN;
    constexpr int LW = SINGLE ? ZV_SINGLE_LW : 0;          // loader waves (waves 4 .. 4 + LW - 1)
    constexpr int BM = 32 * MT * WM;
    const ConvJob &J = jobs.j[blockIdx.z];
    // workgroup -> (row tile bx, channel group by of ny).  Single-utterance launches deal the channel groups over the XCDs (the
    // hardware hands workgroup i to XCD i % 8): all row tiles of a channel group run on ONE XCD, whose L2 then holds that group's
    // weight fragments (a 1 056 x 1 056 x 3 conv's 6.7 MB do not fit one XCD's 4 MB; with row tiles dealt over the XCDs every XCD
    // streamed all of them from the memory side: scripts/frag_stream_bw.hip, 7-10 TB/s over the chip)
    // A launch over several segments with fewer than 8 channel groups deals each group's row tiles over several XCDs instead (conv_xcd.h)
    int bx = blockIdx.x, by = blockIdx.y, ny = gridDim.y;
    int warm_part = 0, warm_parts = 1;
    if constexpr (SINGLE)
        if (jobs.xcd_ny)
        {
            ConvXcdSlot slot;
            if (!conv_xcd_slot(blockIdx.x, jobs.xcd_nx, jobs.xcd_ny, jobs.xcd_spread, slot)) return;
            bx = slot.bx;
            by = slot.by;
            ny = jobs.xcd_ny;
            warm_part = slot.part;
            warm_parts = slot.nparts;
        }

    // workgroup -> (segment, row tile inside the segment)
    const int useg = bx / jobs.tps;
    const Seg sg = seg_at(jobs.segs, useg);
    const int L = sg.rows * jobs.rate;
    const int m0 = (bx - useg * jobs.tps) * BM;
    if (m0 >= L) return;
    const size_t row0 = (size_t)sg.row0 * jobs.rate;

    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;

    const int K = J.K, dil = J.dil, Cin_p = J.Cin_p, Cout_p = J.Cout_p;
    const int nicb = Cin_p >> 4;
    const int ntiles = (Cout_p + 31) >> 5;
    // the output tiles are dealt evenly over the gridDim.y channel groups (33 tiles over 5 groups: 7 7 7 6 6, not 8 8 8 8 1 —
    // every workgroup stages its input tile for every chunk, however few of its waves have work)
    const int nt_span = ntiles - jobs.nt_begin;     // (tiles before nt_begin belong to conv_gemm_kernel)
    const int gt0 = jobs.nt_begin + (int)((long)by * nt_span / ny), gt1 = jobs.nt_begin + (int)((long)(by + 1) * nt_span / ny);
    const int nt0 = gt0 + wn * NT;
    const bool n_ok = nt0 < gt1;
    // a wave whose second tile does not exist computes the tile before it twice and stores it once
    const int ntl = nt0 + NT <= gt1 ? nt0 : (gt1 - NT > 0 ? gt1 - NT : 0);
    const int rows = BM + (K - 1) * dil;
    const int RS = J.ck * 2 + 16;            // LDS row stride in bytes
    if constexpr (SINGLE)
        if (jobs.xcd_ny && jobs.warm)
            l2_warm((const char *)J.w + (size_t)gt0 * K * nicb * 1024, (size_t)(gt1 - gt0) * K * nicb * 1024, warm_part, warm_parts, tid, 256 + 64 * LW);

    StageSrc S;
    {
        const size_t xo = row0 * J.ldx * (J.pro == PRO_RAW_F16 ? 2 : 4);
        S.x0 = (const char *)J.x0 + xo;
        S.x1 = J.x1 ? (const char *)J.x1 + xo : nullptr;
        S.x2 = J.x2 ? (const char *)J.x2 + xo : nullptr;
        S.pa = J.pa ? J.pa + (size_t)useg * J.pab_seg : nullptr;
        S.pb = J.pb ? J.pb + (size_t)useg * J.pab_seg : nullptr;
        S.pstat = J.pstat ? J.pstat + (size_t)useg * J.pstat_seg : nullptr;
        S.ldx = J.ldx;
        S.L = L;
        S.slope = J.slope;
        S.pscale = J.pscale;
    }

    floatx16 acc[MT][NT];
#pragma unroll
    for (int i = 0; i < MT; i++)
#pragma unroll
        for (int n = 0; n < NT; n++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[i][n][r] = 0.f;

    const char *abase = smem + (wm * 32 * MT + (lane & 31)) * RS + (lane >> 5) * 16;

    // SINGLE: the weight ring of the full 256-channel chunks, requested before the first tile is staged
    half8 bring[SINGLE ? 16 : 1];
    const bool single256 = SINGLE && NT == 1 && J.ck == 256 && Cin_p >= 256 && n_ok;
#ifdef ZV_STAMPS
    const int stamp_wg = bx + jobs.tps * jobs.segs.nseg * by;
    int stamp_k = 1;
#endif
    ZV_STAMP(0)
    // Loader waves: tile c is staged into LDS tile c & 1; barrier #c = "tile c is staged and the MFMA loop of chunk c - 1 is done", so
    // the loaders fill tile c + 1 (last read by chunk c - 1) while the MFMA waves walk chunk c.  One barrier per chunk for every wave.
    if constexpr (LW > 0)
        if (wave >= 4)
        {
            constexpr int NL = 64 * (LW > 0 ? LW : 1), UL = ZV_STAGE_ULW;
            const int ltid = tid - 256;
            // a tile that fits the loaders' registers (and is one tensor) travels in two halves, TWO tiles ahead: tile c + 2 is requested
            // before barrier #c (into the register set tile c left), tile c + 1 — requested a whole chunk earlier — is written after
            // it.  (One tile ahead, the request had only the loaders' wait at the barrier to land in: behind the MFMA waves' weight stream
            // on the CU's vector-memory path a round trip is ~2.5 us and the MFMA waves waited 2.1 us per chunk for the loaders.)
            // The loaders' raw barrier does not wait for the vector-memory counter.
            const bool split = J.pro != PRO_SUM3_ACT && rows * (J.ck >> 2) <= NL * UL && !(ZV_DBGBITS(J.dbg) & 1);
            StageRegs<UL> Ra, Rb;
            const int nck = J.ck;
            auto ckof = [&](int c) { return (Cin_p - c < nck) ? (Cin_p - c) : nck; };
#define ZV_LOAD_(P) stage_load_p<UL, P, NL>(S, cn_, ckn_, m0 - J.pad, rows, ltid, R_)
#define ZV_STORE_(P) stage_store_p<UL, P, NL>(S, dst_, RS, cn_, ckn_, m0 - J.pad, rows, ltid, R_)
#define ZV_LD_TILE(REGS, c)                                        \
    if ((c) < Cin_p)                                               \
    {                                                              \
        StageRegs<UL> &R_ = REGS;                                  \
        const int cn_ = (c), ckn_ = ckof(c);                       \
        ZV_STAGE_SPLIT_SWITCH(J.pro, ZV_LOAD_)                     \
    }
#define ZV_ST_TILE(REGS, c, buf)                                   \
    if ((c) < Cin_p)                                               \
    {                                                              \
        const StageRegs<UL> &R_ = REGS;                            \
        const int cn_ = (c), ckn_ = ckof(c);                       \
        char *dst_ = smem + (buf) * jobs.tile_bytes;               \
        ZV_STAGE_SPLIT_SWITCH(J.pro, ZV_STORE_)                    \
    }
#define ZV_RAW_BARRIER()                                           \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");             \
    __builtin_amdgcn_s_barrier();                                  \
    asm volatile("" ::: "memory");
            if (split)
            {
                ZV_LD_TILE(Ra, 0)
                ZV_LD_TILE(Rb, nck)
                ZV_ST_TILE(Ra, 0, 0)
                // chunks in pairs: tile c lives in Ra for even chunk indices, in Rb for odd ones
#ifdef ZV_STAMPS_LOADER
                const int stamp_wg = bx + jobs.tps * jobs.segs.nseg * by;
                int lk = 1;
                ZV_STAMP(0)
#define ZV_LSTAMP() if (lk < 11) { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); ZV_STAMP(lk) lk++; }
#else
#define ZV_LSTAMP()
#endif
                for (int c0 = 0; c0 < Cin_p; c0 += 2 * nck)
                {
                    ZV_LD_TILE(Ra, c0 + 2 * nck)
                    ZV_LSTAMP()
                    ZV_RAW_BARRIER()                   // barrier of chunk c0
                    ZV_LSTAMP()
                    ZV_ST_TILE(Rb, c0 + nck, 1)
                    ZV_LSTAMP()
                    if (c0 + nck >= Cin_p) break;
                    ZV_LD_TILE(Rb, c0 + 3 * nck)
                    ZV_LSTAMP()
                    ZV_RAW_BARRIER()                   // barrier of chunk c0 + ck
                    ZV_LSTAMP()
                    ZV_ST_TILE(Ra, c0 + 2 * nck, 0)
                    ZV_LSTAMP()
                }
#ifdef ZV_STAMPS_LOADER
                ZV_STAMP(11)
#endif
#undef ZV_LSTAMP
            }
            else
            {
                int par = 0;
                for (int c0 = 0; c0 < Cin_p; c0 += J.ck)
                {
                    const int ck = ckof(c0);
                    if (!(ZV_DBGBITS(J.dbg) & 1))
                        stage_tile<ZV_STAGE_ULW, NL>(J.pro, S, smem + par * jobs.tile_bytes, RS, c0, ck, m0 - J.pad, rows, ltid);
                    __syncthreads();
                    par ^= 1;
                }
            }
#undef ZV_RAW_BARRIER
#undef ZV_ST_TILE
#undef ZV_LD_TILE
#undef ZV_LOAD_
#undef ZV_STORE_
            return;
        }
    // (behind the loaders' branch: the ring's registers and the loaders' never live side by side)
    if constexpr (SINGLE)
        if (single256) preload_ring16<MT>(bring, (const half8 *)J.w + (size_t)ntl * K * nicb * 64 + lane);
    int par = 0;
    for (int c0 = 0; c0 < Cin_p; c0 += J.ck)
    {
        const int ck = (Cin_p - c0 < J.ck) ? (Cin_p - c0) : J.ck;
        if (LW == 0 && c0) __syncthreads();
        if (LW == 0 && !(ZV_DBGBITS(J.dbg) & 1))
        {
            // an f16 operand tensor (the decoder's pre-pass output) in 16-byte pieces, a 64-row x 256-channel tile in ONE round
            // trip (9 pieces per thread in flight); the 8-byte pieces of stage_tile took four (phase stamps: 5.5-6.2 us per chunk)
            if (J.pro == PRO_RAW_F16 && (ck & 7) == 0 && !SINGLE)
                stage_raw16<(BM >= 64 ? 9 : 5), 256>(S, smem, RS, c0, ck, m0 - J.pad, rows, tid);
            else
                // (the big wave tiles have the registers — dead before the accumulators live — for 8 pieces in flight: a
                // 64-row x 256-channel f32 tile in three round trips instead of five)
                stage_tile<(SINGLE ? ZV_STAGE_US : (MT * NT >= 4 ? 8 : ZV_STAGE_U))>(J.pro, S, smem, RS, c0, ck, m0 - J.pad, rows, tid);
        }
        if constexpr (LW > 0)
        {
            // barrier #c, raw: the weight ring's requests stay in flight across it (__syncthreads would drain them: 1.1 us per chunk)
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
        }
        else
            __syncthreads();
#ifdef ZV_STAMPS
        if (stamp_k < 10) { ZV_STAMP(stamp_k) stamp_k++; }
#endif
        if (n_ok && !(ZV_DBGBITS(J.dbg) & 2))
        {
            const char *ab_ = abase + (LW > 0 ? par * jobs.tile_bytes : 0);
            const half8 *wp = (const half8 *)J.w + ((size_t)ntl * K * nicb + (size_t)K * (c0 >> 4)) * 64 + lane;
            const size_t wseg = (size_t)K * nicb * 64;             // half8 units between consecutive output tiles
            // full chunks of 256 / 128 / 64 channels take the immediate-address loop (S = K*nkc is a multiple of 4 there
            // and the blocks of a chunk are contiguous [tap][kc]: exactly the order mfma_taps walks)
            if constexpr (SINGLE && NT == 1)
            {
                if (ck == 256 && single256)
                    mfma_taps_single256<MT>(acc, ab_, dil * RS, wp, K, bring);
                else
                    mfma_chunk<MT, NT>(acc, ab_, RS, dil, wp, wseg, K, ck >> 4);
            }
            else if constexpr (NT == 2)
            {
                // the 64 x 64 wave tile keeps to loops with ONE set of four weight-fragment slots (168 registers: three
                // workgroups per CU)
                if (ck == 256 && J.ck == 256)
                    mfma_taps_ring4<256, MT, NT>(acc, ab_, dil * RS, wp, wseg, K);
                else
                    mfma_chunk<MT, NT>(acc, ab_, RS, dil, wp, wseg, K, ck >> 4);
            }
            else if (ck == 256 && J.ck == 256)
                mfma_taps<256, MT, NT, false>(acc, ab_, dil * RS, wp, wseg, K);
            else if (ck == 128 && J.ck == 128)
                mfma_taps<128, MT, NT, false>(acc, ab_, dil * RS, wp, wseg, K);
            else if (ck == 64 && J.ck == 64)
                mfma_taps<64, MT, NT, false>(acc, ab_, dil * RS, wp, wseg, K);
            else
                mfma_chunk<MT, NT>(acc, ab_, RS, dil, wp, wseg, K, ck >> 4);
        }
#ifdef ZV_STAMPS
        if (stamp_k < 11) { ZV_STAMP(stamp_k) stamp_k++; }
#endif
        par ^= 1;
    }

    // ---------------- epilogue ----------------
    if (!n_ok || (ZV_DBGBITS(J.dbg) & 4)) return;
    const float escale = J.escale;
    const int tbase = m0 + wm * 32 * MT + 4 * (lane >> 5);
    const bool has_res = J.res != nullptr;
    const float *res = has_res ? J.res + row0 * J.ldres : nullptr;
    const size_t out0 = row0 * J.ldo;
#pragma unroll
    for (int n = 0; n < NT; n++)
    {
        const int nt = ntl + n;
        if (nt < nt0) continue;                       // the duplicate of a clamped pair
        const int oc = nt * 32 + (lane & 31);
        if (oc >= Cout_p) continue;
        const float bias = J.bias ? J.bias[oc] : 0.f;
        // every residual load of the output tile column in flight before the first use (one round trip per 32 output
        // channels, not one per 32 x 32 tile: the weight-fragment registers of the MFMA loop are free by now)
        float resv[MT][16];
        if (has_res)
        {
#pragma unroll
            for (int mt = 0; mt < MT; mt++)
#pragma unroll
                for (int r = 0; r < 16; r++)
                {
                    const int t = tbase + mt * 32 + (r & 3) + 8 * (r >> 2);
                    resv[mt][r] = res[(size_t)(t < L ? t : L - 1) * J.ldres + oc];
                }
        }
#pragma unroll
        for (int mt = 0; mt < MT; mt++)
        {
            float outv[16];
#pragma unroll
            for (int r = 0; r < 16; r++)
            {
                const int t = tbase + mt * 32 + (r & 3) + 8 * (r >> 2);
                float v = acc[mt][n][r] + bias;
                if (has_res) v = v + resv[mt][r];
                v = v * escale;
                if (J.eact) v = lrelu(v, J.oslope);
                outv[r] = v;
                if (t < L)
                {
                    // non-temporal stores: a conv's output is read by the NEXT launch, long after it has left the caches
                    // (measured on the batch: -1 ... -6.5 % per conv kernel, nothing slower)
                    // ... single-utterance launches store plainly: their small outputs are still in the memory-side cache when the next
                    // launch stages them (configs[2]: 1.711 -> 1.693 ms over three interleaved rounds)
                    if constexpr (SINGLE)
                    {
                        if (J.out_f16) ((_Float16 *)J.out)[out0 + (size_t)t * J.ldo + oc] = (_Float16)v;
                        else ((float *)J.out)[out0 + (size_t)t * J.ldo + oc] = v;
                    }
                    else
                    if (J.out_f16)
                        __builtin_nontemporal_store((_Float16)v, (_Float16 *)J.out + out0 + (size_t)t * J.ldo + oc);
                    else
                        __builtin_nontemporal_store(v, (float *)J.out + out0 + (size_t)t * J.ldo + oc);
                }
            }
            if (J.stat_part && oc < J.stat_C)
            {
                const int blk = (m0 >> 5) + wm * MT + mt;                  // 32-row block of the segment
                if (blk * 32 < L)
                    tile_stats_store(outv, tbase + mt * 32, L, J.stat_part + (((size_t)useg * J.stat_nblk + blk) * J.stat_C + oc) * 2);
            }
        }
    }
#ifdef ZV_STAMPS
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    ZV_STAMP(11)
#endif
}

// the plan's geometry (conv_plan.h) into the job table, then the instantiation it names
template <int MT, int WN, int NT, bool SINGLE = false>
static hipError_t launch_cfg(hipStream_t s, ConvJobs &jobs, const ConvPlan &p)
{
#ifdef ZV_STAMPS
    jobs.stamp = knob(ZV_STAMP_CONV) && knob(ZV_STAMP_CONV) == (p.xcd_ny ? p.xcd_ny : p.gy) && p.gz == 1 &&
                         (knob(ZV_STAMP_CIN) ? jobs.j[0].Cin_p == knob(ZV_STAMP_CIN) : jobs.j[0].Cin_p >= 1024)
                     ? stamp_buffer()
                     : nullptr;
#endif
    jobs.tile_bytes = p.tile_bytes;
    jobs.xcd_nx = p.xcd_nx, jobs.xcd_ny = p.xcd_ny, jobs.xcd_spread = p.xcd_spread;
    jobs.warm = p.warm;
    return launch_lds(conv1d_mfma_kernel<MT, WN, NT, SINGLE>, dim3(p.gx, p.gy, p.gz), dim3(p.threads), p.lds_bytes, s, jobs);
}

// defined in conv_gemm.hip
hipError_t launch_conv_gemm(hipStream_t s, const ConvJob &job, const Segs &segs, int rate);

// ---------------------------------------------------------------------------------------------------
// conv_stream_kernel — the memory-bound polyphase transposed convs of a batch (the last two upsample convs, reference
// src/hifigan.cpp:281-297 + 22-71: a few hundred MACs per output element against 8-12 bytes moved) as a stream.
// In conv1d_mfma_kernel every 64-row workgroup of such a conv is a chain of round trips — stage the tile, fetch 36-98 KiB of
// weight fragments from L2, store, wait for the stores to drain — and the launch's rate is workgroups in flight over that chain
// (ablations: with its MFMA loop off the last upsample conv takes 429 of its 610 us, stores alone 280).  Here a workgroup
//   * keeps the weight fragments of its four output tiles in REGISTERS (one 32-channel tile per wave, K * Cin/16 = 12 / 24
//     fragments) and walks a strip of up to 8 consecutive 64-row tiles with them;
//   * requests tile i + 1's rows (f32, one tensor: PRO_ACT / PRO_SCALE_ACT) into registers ahead of tile i's MFMAs, converts and
//     writes them into the other half of a double-buffered LDS tile behind them: one barrier per tile, no staging wait after
//     the first tile, the stores of tile i drain under tile i + 1.
// Same prologue arithmetic, same (tap, channel) chain per output element, same epilogue as conv1d_mfma_kernel: same bits.
template <int NKC>
__global__ __launch_bounds__(256, NKC == 8 ? 2 : 3) void conv_stream_kernel(const ConvJobs jobs, const int strip)
{
    constexpr int K = 3, CIN = 16 * NKC, RS = CIN * 2 + 16, NF = K * NKC, TROWS = 64 + K - 1;
    constexpr int C4 = CIN / 4, NP = (TROWS * C4 + 255) / 256, TILE_B = TROWS * RS;
    const ConvJob &J = jobs.j[0];
    const int useg = blockIdx.x / jobs.tps;
    const Seg sg = seg_at(jobs.segs, useg);
    const int L = sg.rows * jobs.rate;
    const int s0 = (blockIdx.x - useg * jobs.tps) * strip * 64;
    if (s0 >= L) return;
    const size_t row0 = (size_t)sg.row0 * jobs.rate;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ntiles = (J.Cout_p + 31) >> 5;
    const int nt_w = blockIdx.y * 4 + wave;
    const bool n_ok = nt_w < ntiles;
    const int nt = n_ok ? nt_w : ntiles - 1;                 // (a wave without a tile computes the last one again and stores nothing)
    half8 wf[NF];
    {
        const half8 *wp = (const half8 *)J.w + (size_t)nt * NF * 64 + lane;
#pragma unroll
        for (int i = 0; i < NF; i++) wf[i] = wp[i * 64];
    }
    const int oc = nt * 32 + (lane & 31);
    const float bias = J.bias ? J.bias[oc] : 0.f;
    const float *xs = (const float *)J.x0 + row0 * J.ldx;
    float *outp = (float *)J.out + row0 * J.ldo;
    const float sc = J.pro == PRO_ACT ? 1.0f : J.pscale, sl = J.slope;
    const int pad = J.pad;

    float4 v[NP];
    auto load_tile = [&](int m0) {
#pragma unroll
        for (int p = 0; p < NP; p++)
        {
            const int idx = tid + p * 256 < TROWS * C4 ? tid + p * 256 : TROWS * C4 - 1;
            const int r = idx / C4, c4 = idx % C4;
            const int t = m0 - pad + r;
            v[p] = *(const float4 *)(xs + (size_t)(t < 0 ? 0 : (t < L ? t : L - 1)) * J.ldx + c4 * 4);
        }
    };
    auto write_tile = [&](int buf, int m0) {
#pragma unroll
        for (int p = 0; p < NP; p++)
        {
            const int idx = tid + p * 256;
            if (idx >= TROWS * C4) continue;
            const int r = idx / C4, c4 = idx % C4;
            const int t = m0 - pad + r;
            float4 x = v[p];
            x.x = x.x * sc;
            x.y = x.y * sc;
            x.z = x.z * sc;
            x.w = x.w * sc;
            half4 h;
            h[0] = (_Float16)lrelu(x.x, sl);
            h[1] = (_Float16)lrelu(x.y, sl);
            h[2] = (_Float16)lrelu(x.z, sl);
            h[3] = (_Float16)lrelu(x.w, sl);
            uint2 pk = *(uint2 *)&h;
            const bool in = t >= 0 && t < L;
            pk.x = in ? pk.x : 0u;
            pk.y = in ? pk.y : 0u;
            *(uint2 *)(smem + buf * TILE_B + r * RS + c4 * 8) = pk;
        }
    };

    int m0 = s0;
    load_tile(m0);
    write_tile(0, m0);
    __syncthreads();
    const char *abase = smem + (lane & 31) * RS + (lane >> 5) * 16;
    for (int i = 0; i < strip && m0 < L; i++, m0 += 64)
    {
        const bool more = i + 1 < strip && m0 + 64 < L;
        if (more) load_tile(m0 + 64);
        __builtin_amdgcn_sched_barrier(0);          // the requests stay ahead of the MFMAs
        floatx16 acc[2];
        const floatx16 z = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        const char *ab = abase + (i & 1) * TILE_B;
#pragma unroll
        for (int tap = 0; tap < K; tap++)
#pragma unroll
            for (int kc = 0; kc < NKC; kc++)
            {
                const half8 a0 = *(const half8 *)(ab + tap * RS + kc * 32);
                const half8 a1 = *(const half8 *)(ab + (32 + tap) * RS + kc * 32);
                const bool first = tap == 0 && kc == 0;
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, wf[tap * NKC + kc], first ? z : acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, wf[tap * NKC + kc], first ? z : acc[1], 0, 0, 0);
            }
        if (n_ok)
        {
            const int tbase = m0 + 4 * (lane >> 5);
#pragma unroll
            for (int mt = 0; mt < 2; mt++)
#pragma unroll
                for (int r = 0; r < 16; r++)
                {
                    const int t = tbase + mt * 32 + (r & 3) + 8 * (r >> 2);
                    const float vv = (acc[mt][r] + bias) * J.escale;
                    if (t < L) __builtin_nontemporal_store(vv, outp + (size_t)t * J.ldo + oc);
                }
        }
        if (more) write_tile((i + 1) & 1, m0 + 64);
        __syncthreads();
    }
}

// a job as conv_plan.h reads it
static inline ConvDesc conv_desc(const ConvJob &j)
{
    return ConvDesc{j.K, j.dil, j.pad, j.Cin_p, j.Cout_p, j.ck, j.pro, j.ldx, j.w8 != nullptr, j.out_f16 != 0, j.res != nullptr, j.stat_part != nullptr, j.eact != 0, j.x1 || j.x2};
}

static hipError_t launch_conv_from(hipStream_t s, const ConvJob *jobs, int njobs, int n_cu, const Segs &segs, int rate, int nt_begin);

hipError_t launch_conv(hipStream_t s, const ConvJob *jobs, int njobs, int n_cu, const Segs &segs, int rate)
{
    if (njobs < 1 || njobs > CONV_MAX_JOBS || segs.nseg < 1 || segs.max_rows < 1) return hipErrorInvalidValue;
    // the jobs conv_gemm_kernel takes (conv_gemm_takes) there, one by one, each with the tiles it leaves over on the generic kernel;
    // the other jobs in one launch of the generic kernel
    const ConvCall call{njobs, segs.nseg, segs.max_rows, rate, n_cu, 0};
    ConvJob rest[CONV_MAX_JOBS];
    int nrest = 0;
    for (int i = 0; i < njobs; i++)
    {
        const ConvJob &j = jobs[i];
        if (!conv_gemm_takes(conv_desc(j), call))
        {
            rest[nrest++] = j;
            continue;
        }
        hipError_t e = launch_conv_gemm(s, j, segs, rate);
        if (e != hipSuccess) return e;
        const int done = conv_gemm_tiles(j.Cout_p);
        if (done * 32 < j.Cout_p)
        {
            e = launch_conv_from(s, &j, 1, n_cu, segs, rate, done);
            if (e != hipSuccess) return e;
        }
    }
    return nrest ? launch_conv_from(s, rest, nrest, n_cu, segs, rate, 0) : hipSuccess;
}

// one launch of the generic family from output tile nt_begin on: validate, plan (conv_plan.h), fill the job table, dispatch
static hipError_t launch_conv_from(hipStream_t s, const ConvJob *jobs, int njobs, int n_cu, const Segs &segs, int rate, int nt_begin)
{
    const int dbg = diag_bits();
    const int Lmax = segs.max_rows * rate;
    ConvJobs js;
    ConvDesc desc[CONV_MAX_JOBS];
    for (int i = 0; i < njobs; i++)
    {
        js.j[i] = jobs[i];
        js.j[i].dbg = dbg;
        desc[i] = conv_desc(jobs[i]);
        if (jobs[i].stat_part && jobs[i].stat_nblk * 32 < Lmax) return hipErrorInvalidValue;
    }
    for (int i = njobs; i < CONV_MAX_JOBS; i++) js.j[i] = js.j[0];
    const ConvPlan p = conv_plan(desc, ConvCall{njobs, segs.nseg, segs.max_rows, rate, n_cu, nt_begin});
    if (!p.valid) return hipErrorInvalidValue;
    js.segs = segs;
    js.rate = rate;
    js.tps = p.tps;
    js.nt_begin = nt_begin;
    js.order = 0;
    if (p.form == CONV_STREAM)
    {
        if (p.nkc == 8)
            hipLaunchKernelGGL(conv_stream_kernel<8>, dim3(p.gx, p.gy, p.gz), dim3(p.threads), p.lds_bytes, s, js, p.strip);
        else
            hipLaunchKernelGGL(conv_stream_kernel<4>, dim3(p.gx, p.gy, p.gz), dim3(p.threads), p.lds_bytes, s, js, p.strip);
        return hipGetLastError();
    }
    if (p.form == CONV_LOADER) return p.WN == 4 ? launch_cfg<1, 4, 1, true>(s, js, p) : launch_cfg<1, 2, 1, true>(s, js, p);
#define ZV_CASE(mt, wn, nt) \
    if (p.MT == mt && p.WN == wn && p.NT == nt) return launch_cfg<mt, wn, nt>(s, js, p);
    ZV_CASE(4, 4, 1) ZV_CASE(2, 4, 1) ZV_CASE(1, 4, 1) ZV_CASE(2, 4, 2)
    ZV_CASE(4, 2, 1) ZV_CASE(2, 2, 1) ZV_CASE(1, 2, 1)
    ZV_CASE(4, 1, 1) ZV_CASE(2, 1, 1) ZV_CASE(1, 1, 1)
#undef ZV_CASE
    return hipErrorInvalidValue;
}


// ---------------------------------------------------------------------------------------------------
// vocoder tail: lrelu -> conv (C -> 1, K taps) + bias -> tanh.  Cout = 1 has no GEMM shape: each lane owns
// one output sample and walks its K x C window in LDS (f16 operands, f32 accumulate).

typedef float f32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 nt_load4(const float *p)
{
    const f32x4 v = __builtin_nontemporal_load((const f32x4 *)p);
    return make_float4(v[0], v[1], v[2], v[3]);
}

__global__ __launch_bounds__(256) void out_conv_tanh_kernel(const OutConvArgs a)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int Cp = round_up(a.C, 16);
    const int RS = Cp * 2 + 16;
    const int K = a.K, pad = (K - 1) / 2;
    const int rows = 256 + K - 1;
    const int tps = (a.segs.max_rows * a.rate + 255) >> 8;
    const int useg = blockIdx.x / tps;
    const Seg sg = seg_at(a.segs, useg);
    const int L = sg.rows * a.rate;
    const int m0 = (blockIdx.x - useg * tps) * 256;
    if (m0 >= L) return;
    const size_t row0 = (size_t)sg.row0 * a.rate;
    const float *x0 = a.x0 + row0 * a.ldx, *x1 = a.x1 ? a.x1 + row0 * a.ldx : nullptr, *x2 = a.x2 ? a.x2 + row0 * a.ldx : nullptr;
    const int tid = threadIdx.x;
    _Float16 *wl = (_Float16 *)(smem + rows * RS);
    for (int i = tid; i < K * Cp; i += 256) wl[i] = ((const _Float16 *)a.w)[i];

    const int cols = Cp >> 2;
    for (int idx = tid; idx < rows * cols; idx += 256)
    {
        const int r = idx / cols, c4 = idx - r * cols;
        const int t = m0 - pad + r;
        half4 h = {0, 0, 0, 0};
        if (t >= 0 && t < L)
        {
            const size_t off = (size_t)t * a.ldx + c4 * 4;
            // non-temporal loads: the branch outputs are read exactly once, here (measured 620 -> 577 us per batch launch;
            // the same policy on the ResBlock kernels' staging loads costs them 4 ... 9 %: their residual re-read wants L2)
            float4 v = nt_load4(x0 + off);
            if (x1)
            {
                const float4 b = nt_load4(x1 + off);
                const float4 d = nt_load4(x2 + off);
                v.x = ((v.x + b.x) + d.x) * a.pscale;
                v.y = ((v.y + b.y) + d.y) * a.pscale;
                v.z = ((v.z + b.z) + d.z) * a.pscale;
                v.w = ((v.w + b.w) + d.w) * a.pscale;
            }
            else
            {   // x0 already is the branches' sum (merged last pair of the stage)
                v.x = v.x * a.pscale;
                v.y = v.y * a.pscale;
                v.z = v.z * a.pscale;
                v.w = v.w * a.pscale;
            }
            h[0] = (_Float16)lrelu(v.x, a.slope);
            h[1] = (_Float16)lrelu(v.y, a.slope);
            h[2] = (_Float16)lrelu(v.z, a.slope);
            h[3] = (_Float16)lrelu(v.w, a.slope);
        }
        *(half4 *)(smem + r * RS + c4 * 8) = h;
    }
    __syncthreads();
    const int t = m0 + tid;
    if (t >= L) return;
    float acc = 0.f;
    for (int tap = 0; tap < K; tap++)
    {
        const char *row = smem + (tid + tap) * RS;
        for (int c = 0; c < Cp; c += 8)
        {
            const half8 x = *(const half8 *)(row + c * 2);
            const half8 w = *(const half8 *)(wl + tap * Cp + c);
#pragma unroll
            for (int j = 0; j < 8; j++) acc = fmaf((float)x[j], (float)w[j], acc);
        }
    }
    // run-shortened schedule: the frames behind the split belong `shift` frames further on in the waveform (launch_voc_run_fill fills the gap)
    const int skip = a.runs && t >= (sg.aux + 1) * a.rate ? a.segs.tab[useg].pad * a.rate : 0;
    a.out[row0 + t + skip] = tanhf(acc + a.bias);
}

hipError_t launch_out_conv(hipStream_t s, const OutConvArgs &a)
{
    const size_t lds = out_conv_lds_bytes(a.C, a.K);
    if (!out_conv_supported(a.C, a.K) || a.segs.nseg < 1) return hipErrorInvalidValue;
    const int tps = (a.segs.max_rows * a.rate + 255) / 256;
    hipLaunchKernelGGL(out_conv_tanh_kernel, dim3(tps * a.segs.nseg), dim3(256), lds, s, a);
    return hipGetLastError();
}

}  // namespace zv
