// conv1d_mfma.hip — the HiFi-GAN ResBlock kernel family (the vocoder's residual blocks): the fused dilation pair
// (resblock_pair_kernel, resblock_pair64_kernel), the whole-block kernels (resblock_block64_kernel, resblock_triple_kernel,
// resblock_block32_kernel), their weight packers and launchers, and the device helpers only they use.
//
// This file holds nothing else on purpose: bench.py and scripts/traffic.py hash it, and the PMC traffic profile
// (profiles/r04_resblock_traffic.json) counts as measured on the code it names only while that hash matches.  An edit
// to another kernel family (conv.hip, conv_gemm.hip) must not mark the ResBlock traffic stale.  What this family shares
// with the others comes from mfma_common.h, which is not hashed: keep that header minimal.
#include "kernels.h"
#include "knobs.h"
#include "mfma_common.h"
#include "tile_deal.h"

#include <hip/hip_fp16.h>
#include <algorithm>
#include <cstdlib>
#include <cstring>

namespace zv
{

// cache policy of the fused kernels' output stores (aux operand of the buffer store; 0 = default, 2 = non-temporal)
#ifndef ZV_ST_AUX
#define ZV_ST_AUX 2       // measured on the batch: -1.1 % (256 / 128 channels), -3.5 % (64), -1.3 % (32) against the default policy
#endif
// timing-only ablation build (-DZV_ABL_A): only the first row tile's A fragment is read from LDS, the others copy it
#ifdef ZV_ABL_A
#define ZV_ABL_LD(arr, p, mt) ((mt) == 0 ? *(const half8 *)(p) : arr[0])
#else
#define ZV_ABL_LD(arr, p, mt) (*(const half8 *)((p) + (mt) * 32 * RS))
#endif
// 16-byte pieces a thread of resblock_pair_kernel keeps in flight while it stages its tile, 128 / 256 channels
#ifndef ZV_STAGE_U128
#define ZV_STAGE_U128 12
#endif
#ifndef ZV_STAGE_U256
#define ZV_STAGE_U256 19
#endif

// mfma_taps (conv.hip) with the A fragments TWO steps ahead (four register sets in rotation) and a scheduling fence after
// every step.  In mfma_taps hipcc moves each A read down next to the MFMA that consumes it (an lgkmcnt wait right
// behind the read: LDS latency exposed on every step); a fence per step pins the reads where they are written, and two
// steps (>= 4 MFMAs at MT = 2) cover the ds_read_b128 latency.  Used by the fused ResBlock kernels, which have the
// registers to spare; in the generic kernel's widest instantiations the fences cost more registers than they gain.
// The accumulators need no clearing before the call: the first step starts them from the constant 0.  The contraction is
// walked in bodies of 8 steps; CP = 64 with K = 3 mod 4 taps leaves half a body, every other supported shape a whole
// number (pair_shape_ok).
// the first four weight fragments of a contraction: requested by the caller ahead of a phase that does not need them (the
// staging wait, the xt pack) so that the MFMA loop does not start with an exposed L2 round trip
template <int NT>
__device__ __forceinline__ void deep_preload_b(half8 (&b0)[4][NT], const half8 *wq, size_t wseg)
{
#pragma unroll
    for (int u = 0; u < 4; u++)
#pragma unroll
        for (int nt = 0; nt < NT; nt++) b0[u][nt] = wq[nt * wseg + u * 64];
}

template <int CP, int MT, int NT, bool SWAP, int DEPTH = 2>
__device__ __forceinline__ void mfma_taps_deep(floatx16 (&acc)[MT][NT], const char *ap, int dilRS, const half8 *wq, size_t wseg, int K,
                                               half8 (&b0)[4][NT], int wstep = 8 * 64)
{
    constexpr int RS = CP * 2 + 16, NKC = CP / 16;
    constexpr int TPB = (NKC >= 8) ? 1 : 8 / NKC;
    constexpr bool HALF = NKC == 16;
    const int nsb = (K * NKC + 3) >> 2;
    const int nb = nsb >> 1;
    half8 b1[4][NT];
    wq += 4 * 64;
    static_assert(DEPTH >= 1 && DEPTH <= 7, "A fragments travel DEPTH steps ahead through a ring of 8 register sets");
    half8 a[8][MT];
#define ZV_UN8(un) ((un) >= 8 ? (un) - 8 : 0)
#define ZV_A_ADDR2(un) ((un) >= 8 ? tbn[(ZV_UN8(un) / NKC) % 4] + (ZV_UN8(un) % NKC) * 32 : tb[((un) / NKC) % 4] + ((un) % NKC) * 32)
#define ZV_LOAD_A2(un)                                                                        \
    {                                                                                         \
        const char *np_ = ZV_A_ADDR2(un);                                                     \
        _Pragma("unroll") for (int mt = 0; mt < MT; mt++) a[(un) % 8][mt] = ZV_ABL_LD(a[(un) % 8], np_, mt); \
    }
#define ZV_STEP2(u, bset) ZV_LOAD_A2((u) + DEPTH) mfma_step<MT, NT, SWAP>(acc, a[(u) % 8], bset[(u) % 4]); __builtin_amdgcn_sched_barrier(0);
#define ZV_STEP2Z(u, bset) ZV_LOAD_A2((u) + DEPTH) mfma_step<MT, NT, SWAP, true>(acc, a[(u) % 8], bset[(u) % 4]); __builtin_amdgcn_sched_barrier(0);
#define ZV_BODY(FIRSTSTEP)                                                                                       \
    {                                                                                                            \
        const char *tb[4], *tbn[4];                                                                              \
        tb[0] = ap;                                                                                              \
        _Pragma("unroll") for (int x = 1; x < 4; x++) tb[x] = (x < TPB) ? ap + x * dilRS : ap;                   \
        const char *apn = HALF ? ((ib & 1) ? ap + (dilRS - 256) : ap + 256) : ap + TPB * dilRS; /* next body */  \
        tbn[0] = apn;                                                                                            \
        _Pragma("unroll") for (int x = 1; x < 4; x++) tbn[x] = (x < TPB) ? apn + x * dilRS : apn;                \
        _Pragma("unroll") for (int u = 0; u < 4; u++)                                                            \
            _Pragma("unroll") for (int nt = 0; nt < NT; nt++) b1[u][nt] = wq[nt * wseg + u * 64];                \
        __builtin_amdgcn_sched_barrier(0);                                                                       \
        FIRSTSTEP(0, b0) ZV_STEP2(1, b0) ZV_STEP2(2, b0) ZV_STEP2(3, b0)                                         \
        _Pragma("unroll") for (int u = 0; u < 4; u++)                                                            \
            _Pragma("unroll") for (int nt = 0; nt < NT; nt++) b0[u][nt] = wq[nt * wseg + (4 + u) * 64];          \
        __builtin_amdgcn_sched_barrier(0);                                                                       \
        ZV_STEP2(4, b1) ZV_STEP2(5, b1) ZV_STEP2(6, b1) ZV_STEP2(7, b1)                                          \
        ap = apn;                                                                                                \
        wq += wstep;                                                                                             \
    }
    {
        const char *tb[4], *tbn[4];
        tb[0] = ap;
#pragma unroll
        for (int x = 1; x < 4; x++) tb[x] = (x < TPB) ? ap + x * dilRS : ap;
#pragma unroll
        for (int x = 0; x < 4; x++) tbn[x] = ap;
        ZV_LOAD_A2(0)
        if constexpr (DEPTH > 1) ZV_LOAD_A2(1)
        if constexpr (DEPTH > 2) ZV_LOAD_A2(2)
        if constexpr (DEPTH > 3) ZV_LOAD_A2(3)
        if constexpr (DEPTH > 4) ZV_LOAD_A2(4)
        if constexpr (DEPTH > 5) ZV_LOAD_A2(5)
        if constexpr (DEPTH > 6) ZV_LOAD_A2(6)
    }
    {
        const int ib = 0;
        ZV_BODY(ZV_STEP2Z)
    }
    for (int ib = 1; ib < nb; ib++) ZV_BODY(ZV_STEP2)
    if constexpr (CP == 64)
        if (nsb & 1)                             // odd sub-block count (K = 3 mod 4 taps): one more tap on b0
        {
            const char *tb[4] = {ap, ap, ap, ap};
            const char *tbn[4] = {ap, ap, ap, ap};
            (void)tbn;
            ZV_STEP2(0, b0) ZV_STEP2(1, b0) ZV_STEP2(2, b0) ZV_STEP2(3, b0)
        }
#undef ZV_BODY
#undef ZV_STEP2Z
#undef ZV_STEP2
#undef ZV_LOAD_A2
#undef ZV_A_ADDR2
#undef ZV_UN8
}

// ---------------------------------------------------------------------------------------------------
// Fused dilation pair of a HiFi-GAN residual block (reference src/hifigan.cpp:99-182):
//     xt = lrelu(conv(lrelu(y), k, dil) + b1);  out = y + (conv(xt, k, 1) + b2)
// One workgroup produces TM = BM - (k-1) output rows: it stages f16(lrelu(y)) for BM + (k-1)*dil rows, runs
// conv1 over BM rows (the k-1 extra rows are conv2's halo) with the weights as the MFMA A operand so that a
// lane ends up with 4 consecutive channels per register quad, packs xt = f16(lrelu(. + b1)) straight back
// into the same LDS region (rows outside [0, L) are conv2's zero padding), runs conv2 from there and adds
// bias + residual in the epilogue.  xt never touches HBM.
//
// The MFMA loop is specialised on the channel count so that every LDS / weight address inside an iteration is
// an immediate: one body = 8 steps = 8 / (CP/16) taps, the per-body bookkeeping is a handful of vector adds.  The first version of this loop carried ~15 scalar/vector instructions of
// tap/channel bookkeeping per MFMA and was instruction-issue bound (SQ_ACTIVE_INST_ANY ~ 74 % of the kernel with
// the MFMA pipe 19 % busy, profiles/r01_v2_pmc.txt).  Weights for this path are packed per 32-channel output
// tile as round_up(K*CP/16, 4) + 8 blocks, zero blocks behind the real ones: the loop needs no tail handling
// and its prefetch never leaves the tile's segment.
size_t pair_weight_halfs(int Cp, int K)
{
    const int nkc = Cp / 16;
    return (size_t)(Cp / 32) * (round_up(K * nkc, 4) + 8) * 512;
}

void pack_pair_weight(const uint16_t *w, int K, int C, int Cp, uint16_t *dst)
{
    const int nkc = Cp / 16;
    const size_t seg = (size_t)(round_up(K * nkc, 4) + 8) * 512;
    memset(dst, 0, pair_weight_halfs(Cp, K) * 2);
    for (int nt = 0; nt < Cp / 32; nt++)
        for (int tap = 0; tap < K; tap++)
            for (int kc = 0; kc < nkc; kc++)
            {
                uint16_t *d = dst + nt * seg + (size_t)(tap * nkc + kc) * 512;
                for (int lane = 0; lane < 64; lane++)
                    for (int j = 0; j < 8; j++)
                    {
                        const int oc = nt * 32 + (lane & 31), ic = kc * 16 + 8 * (lane >> 5) + j;
                        d[lane * 8 + j] = (oc < C && ic < C) ? w[((size_t)oc * C + ic) * K + tap] : (uint16_t)0;
                    }
            }
}

// leaky-ReLU for 0 <= slope <= 1 as max(x, x*slope): same bits as (x > 0 ? x : x*slope), one instruction less and
// no compare/select pair; raw v_max_f32 keeps hipcc from adding a canonicalising multiply in front of fmaxf
__device__ __forceinline__ float lrelu_max(float x, float s)
{
    float r;
    const float xs = x * s;
    asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(xs));
    return r;
}

// max(x, xs) with xs = x * slope already formed (packed multiplies)
__device__ __forceinline__ float lrelu_max_pre(float x, float xs)
{
    float r;
    asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(xs));
    return r;
}

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

typedef _Float16 half2v __attribute__((ext_vector_type(2)));

// f16(lrelu(x + b)) of four values: packed add / multiply / convert (v_pk_add_f32, v_pk_mul_f32, v_cvt_pk_f16_f32: the
// same IEEE results as the scalar forms), max(x, x*slope) as in lrelu_max
__device__ __forceinline__ uint2 lrelu4_f16(float x0, float x1, float x2, float x3, float sl)
{
    const float2v a = {x0, x1}, c = {x2, x3};
    const float2v as = a * sl, cs = c * sl;
    const float2v ra = {lrelu_max_pre(a[0], as[0]), lrelu_max_pre(a[1], as[1])};
    const float2v rc = {lrelu_max_pre(c[0], cs[0]), lrelu_max_pre(c[1], cs[1])};
    const half2v ha = __builtin_convertvector(ra, half2v), hc = __builtin_convertvector(rc, half2v);
    uint2 pk;
    pk.x = *(const unsigned int *)&ha;
    pk.y = *(const unsigned int *)&hc;
    return pk;
}


// Stage f16(lrelu(y)) rows through a buffer descriptor: rows outside [0, L) are out of the descriptor's range and
// read as 0 (= the conv's zero padding, lrelu(0) = 0) with no per-row predicate; CP is a power of two so the
// row / column split of the flat index is a shift and a mask.
template <int U, int CP>
__device__ __forceinline__ void stage_act_buf(__amdgpu_buffer_rsrc_t rsrc, char *smem, int row_t0, int rows, int tid, float slope)
{
    constexpr int RS = CP * 2 + 16, COLS = CP / 4, SH = (CP == 32) ? 3 : (CP == 64 ? 4 : (CP == 128 ? 5 : 6));
    const int total = rows * COLS;
    for (int base = tid; base < total; base += 256 * U)
    {
        u32x4 v[U];
#pragma unroll
        for (int u = 0; u < U; u++)
        {
            const int idx = base + u * 256;
            const int r = idx >> SH, c4 = idx & (COLS - 1);
            const int voff = (idx < total) ? ((row_t0 + r) * CP + c4 * 4) * 4 : -16;
            v[u] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff, 0, 0);
        }
#pragma unroll
        for (int u = 0; u < U; u++)
        {
            const int idx = base + u * 256;
            if (idx < total)
            {
                const int r = idx >> SH, c4 = idx & (COLS - 1);
                half4 h;
                h[0] = (_Float16)lrelu_max(__uint_as_float(v[u].x), slope);
                h[1] = (_Float16)lrelu_max(__uint_as_float(v[u].y), slope);
                h[2] = (_Float16)lrelu_max(__uint_as_float(v[u].z), slope);
                h[3] = (_Float16)lrelu_max(__uint_as_float(v[u].w), slope);
                *(half4 *)(smem + r * RS + c4 * 8) = h;
            }
        }
    }
}

// MERGE: one workgroup runs the SAME time tile of all the launch's jobs (the MRF branches of a stage) one after the other
// and stores only (out_0 + out_1) + out_2 — the sum the next layer starts with (reference src/hifigan.cpp:300-315) — so the
// branch outputs of a stage's last dilation pair never reach HBM and the consumer reads one tensor instead of three.  The
// tile height is that of the job with the most taps (a few rows of extra halo for the others).
//
// The kernel runs on v_mfma_f32_16x16x32_f16 (round 4; rounds 1-3: 32x32x16, whose MFMA loop — mfma_taps_deep above — the
// single-utterance whole-block kernel resblock_triple_kernel still uses).
//
// The two f16 MFMA shapes give the SAME BITS for one k-ordered accumulation chain: a chain walked 16 products per instruction
// (32x32x16) equals the same chain walked 32 per instruction (16x16x32) — measured on 204 800 random elements at three scales,
// scripts/mfma_shape_bits.hip: 0 differ (neither equals a sequential fma chain nor an f64 sum rounded once: the matrix core has
// its own order, but one order for both shapes), and asserted by tests/test_gpu_mfma_chain.py on chains whose products span the
// whole f16 range (subnormals included), cancel, or meet an accumulator 2^20 out of scale, K up to 3 360: 0 of 68 608 differ,
// profiles/mfma_chain.txt.  So a kernel may change its shape without leaving the family's "every output
// element is ONE chain over (chunk, tap, channel)" contract, and the chip holds a higher clock under the 16 x 16 shape
// (MI355X_MICROARCH.md, DVFS give-back item 7).  One step here = 32 channels of one tap = two steps of the kernel above:
//   LDS side   l[mt][lt]: the two 16-row tiles of 32-row block mt.  Fragment row c of tile lt is block row 2c + lt (even / odd
//              interleave): with the tile's row stride 2 CP + 16 bytes the ds_read_b128 of lane (c, g = k group) then falls on
//              16 distinct 16-byte slots per lane group (rows c and 16 + c would share a slot: 2-way);
//   weights    w[nt][wt]: the two 16-channel tiles of output tile nt, packed in fragment order by pack_pair_weight16 (conv1: the
//              A operand, row r of tile wt = channel 16 wt + r; conv2: the B operand, column c of tile wt = channel 2c + wt, so a
//              lane's two tiles are NEIGHBOURING channels and the epilogue moves 8 bytes per lane: four rows x 128 bytes per
//              instruction, half the instructions of the 4-byte column accesses above).
// acc[mt][nt][wt][lt] is a 16 x 16 tile: conv1 (weights as A) lane (c, g) holds channels 16 wt + 4g + i of time row 2c + lt;
// conv2 holds time rows 8g + 2i + lt of channel 2c + wt.

size_t pair_weight16_halfs(int Cp, int K) { return pair_weight_halfs(Cp, K); }

// conv2_layout: the B-operand form (channel 2c + wt); else the A-operand form (channel 16 wt + r)
void pack_pair_weight16(const uint16_t *w, int K, int C, int Cp, uint16_t *dst, bool conv2_layout)
{
    const int nk2 = Cp / 32;
    const size_t seg = (size_t)(round_up(K * (Cp / 16), 4) + 8) * 512;
    memset(dst, 0, pair_weight16_halfs(Cp, K) * 2);
    for (int nt = 0; nt < Cp / 32; nt++)
        for (int tap = 0; tap < K; tap++)
            for (int k2 = 0; k2 < nk2; k2++)
                for (int wt = 0; wt < 2; wt++)
                {
                    uint16_t *d = dst + nt * seg + ((size_t)(tap * nk2 + k2) * 2 + wt) * 512;
                    for (int lane = 0; lane < 64; lane++)
                        for (int j = 0; j < 8; j++)
                        {
                            const int r = lane & 15, g = lane >> 4;
                            const int oc = nt * 32 + (conv2_layout ? 2 * r + wt : 16 * wt + r), ic = k2 * 32 + 8 * g + j;
                            d[lane * 8 + j] = (oc < C && ic < C) ? w[((size_t)oc * C + ic) * K + tap] : (uint16_t)0;
                        }
                }
}

template <int MT, int NT, bool SWAP, bool ZERO = false>
__device__ __forceinline__ void mfma16_step(floatx4 (&acc)[MT][NT][2][2], const half8 (&l)[MT][2], const half8 (&w)[NT][2])
{
    const floatx4 z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int mt = 0; mt < MT; mt++)
#pragma unroll
        for (int nt = 0; nt < NT; nt++)
#pragma unroll
            for (int wt = 0; wt < 2; wt++)
#pragma unroll
                for (int lt = 0; lt < 2; lt++)
                {
                    if constexpr (SWAP)      // weights as the A operand -> D[oc][time]
                        acc[mt][nt][wt][lt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w[nt][wt], l[mt][lt], ZERO ? z : acc[mt][nt][wt][lt], 0, 0, 0);
                    else
                        acc[mt][nt][wt][lt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(l[mt][lt], w[nt][wt], ZERO ? z : acc[mt][nt][wt][lt], 0, 0, 0);
                }
}

// the first two steps' weight fragments of a contraction (see deep_preload_b)
template <int NT>
__device__ __forceinline__ void deep16_preload_b(half8 (&b0)[2][NT][2], const half8 *wq, size_t wseg)
{
#pragma unroll
    for (int u = 0; u < 2; u++)
#pragma unroll
        for (int nt = 0; nt < NT; nt++)
#pragma unroll
            for (int wt = 0; wt < 2; wt++) b0[u][nt][wt] = wq[nt * wseg + (u * 2 + wt) * 64];
}

// mfma_taps_deep's structure in steps of 32 channels: a body = 4 steps (= its 8), the weight fragments in two ping-pong sets of
// two steps each (requested a set ahead), the LDS fragments one step ahead through a ring of four register sets, a scheduling
// fence per step.  Same (tap, channel) order: the same chain per output element.
template <int CP, int MT, int NT, bool SWAP>
__device__ __forceinline__ void mfma16_taps_deep(floatx4 (&acc)[MT][NT][2][2], const char *ap, int dilRS, const half8 *wq, size_t wseg, int K,
                                                 half8 (&b0)[2][NT][2])
{
    constexpr int RS = CP * 2 + 16, NK2 = CP / 32;
    constexpr int TPB = (NK2 >= 4) ? 1 : 4 / NK2;        // taps per body: 4 / 2 / 1 / (1/2) for CP = 32 / 64 / 128 / 256
    constexpr bool HALF = NK2 == 8;                      // CP = 256: a tap is two bodies
    const int nsb = (K * NK2 + 1) >> 1;                  // 2-step sub-blocks (the last one may run partly on zero weights)
    const int nb = nsb >> 1;
    half8 b1[2][NT][2];
    wq += 4 * 64;
    half8 a[4][MT][2];
#define ZV16_UN(un) ((un) >= 4 ? (un) - 4 : 0)
#define ZV16_A_ADDR(un) ((un) >= 4 ? tbn[(ZV16_UN(un) / NK2) % 4] + (ZV16_UN(un) % NK2) * 64 : tb[((un) / NK2) % 4] + ((un) % NK2) * 64)
#define ZV16_LOAD_A(un)                                                                                          \
    {                                                                                                            \
        const char *np_ = ZV16_A_ADDR(un);                                                                       \
        _Pragma("unroll") for (int mt = 0; mt < MT; mt++)                                                        \
            _Pragma("unroll") for (int lt = 0; lt < 2; lt++) a[(un) % 4][mt][lt] = *(const half8 *)(np_ + (mt * 32 + lt) * RS); \
    }
#define ZV16_STEP(u, bset) ZV16_LOAD_A((u) + 1) mfma16_step<MT, NT, SWAP>(acc, a[(u) % 4], bset[(u) % 2]); __builtin_amdgcn_sched_barrier(0);
#define ZV16_STEPZ(u, bset) ZV16_LOAD_A((u) + 1) mfma16_step<MT, NT, SWAP, true>(acc, a[(u) % 4], bset[(u) % 2]); __builtin_amdgcn_sched_barrier(0);
#define ZV16_BODY(FIRSTSTEP)                                                                                     \
    {                                                                                                            \
        const char *tb[4], *tbn[4];                                                                              \
        tb[0] = ap;                                                                                              \
        _Pragma("unroll") for (int x = 1; x < 4; x++) tb[x] = (x < TPB) ? ap + x * dilRS : ap;                   \
        const char *apn = HALF ? ((ib & 1) ? ap + (dilRS - 256) : ap + 256) : ap + TPB * dilRS; /* next body */  \
        tbn[0] = apn;                                                                                            \
        _Pragma("unroll") for (int x = 1; x < 4; x++) tbn[x] = (x < TPB) ? apn + x * dilRS : apn;                \
        _Pragma("unroll") for (int u = 0; u < 2; u++)                                                            \
            _Pragma("unroll") for (int nt = 0; nt < NT; nt++)                                                    \
                _Pragma("unroll") for (int wt = 0; wt < 2; wt++) b1[u][nt][wt] = wq[nt * wseg + (u * 2 + wt) * 64];        \
        __builtin_amdgcn_sched_barrier(0);                                                                       \
        FIRSTSTEP(0, b0) ZV16_STEP(1, b0)                                                                        \
        _Pragma("unroll") for (int u = 0; u < 2; u++)                                                            \
            _Pragma("unroll") for (int nt = 0; nt < NT; nt++)                                                    \
                _Pragma("unroll") for (int wt = 0; wt < 2; wt++) b0[u][nt][wt] = wq[nt * wseg + (4 + u * 2 + wt) * 64];    \
        __builtin_amdgcn_sched_barrier(0);                                                                       \
        ZV16_STEP(2, b1) ZV16_STEP(3, b1)                                                                        \
        ap = apn;                                                                                                \
        wq += 8 * 64;                                                                                            \
    }
    {
        const char *tb[4], *tbn[4];
        tb[0] = ap;
#pragma unroll
        for (int x = 1; x < 4; x++) tb[x] = (x < TPB) ? ap + x * dilRS : ap;
#pragma unroll
        for (int x = 0; x < 4; x++) tbn[x] = ap;
        ZV16_LOAD_A(0)
    }
    {
        const int ib = 0;
        ZV16_BODY(ZV16_STEPZ)
    }
    for (int ib = 1; ib < nb; ib++) ZV16_BODY(ZV16_STEP)
    if constexpr (CP == 64)
        if (nsb & 1)                             // odd sub-block count (K = 3 mod 4 taps): one more tap on b0
        {
            const char *tb[4] = {ap, ap, ap, ap};
            const char *tbn[4] = {ap, ap, ap, ap};
            (void)tbn;
            ZV16_STEP(0, b0) ZV16_STEP(1, b0)
        }
#undef ZV16_BODY
#undef ZV16_STEPZ
#undef ZV16_STEP
#undef ZV16_LOAD_A
#undef ZV16_A_ADDR
#undef ZV16_UN
}

template <int CP, int MT, bool MERGE>
__global__ __launch_bounds__(256) void resblock_pair_kernel(const PairJobs jobs)
{
    constexpr int NT = (CP == 256) ? 2 : 1;            // output tiles of 32 channels per wave
    constexpr int WN = CP / 32 / NT, WM = 4 / WN;
    constexpr int BM = 32 * MT * WM;
    constexpr int RS = CP * 2 + 16, NKC = CP / 16;
    const int jz = (int)blockIdx.z, bx = (int)blockIdx.x;
    const int TM = BM - (MERGE ? jobs.kmax - 1 : jobs.j[jz].K - 1);
    const int tps = (jobs.segs.max_rows * jobs.rate + TM - 1) / TM;
    const int vt = tile_deal(bx, tps, jobs.segs.nseg, jobs.deal_c);
    if (vt >= tps * jobs.segs.nseg) return;
    const int useg = vt / tps;
    const Seg sg = seg_at(jobs.segs, useg);
    const int L = sg.rows * jobs.rate;
    const int t0 = (vt - useg * tps) * TM;
    if (t0 >= L) return;
    floatx4 msum[MERGE ? MT : 1][MERGE ? NT : 1][2][2];
    for (int jb = MERGE ? 0 : jz; jb < (MERGE ? jobs.njobs : jz + 1); jb++)
    {
    const PairJob &P = jobs.j[jb];
    const int K = P.K, dil = P.dil;
    const int h2 = (K - 1) / 2, h1 = h2 * dil;
    const float *y_seg = P.y + (size_t)sg.row0 * jobs.rate * CP;
    float *out_seg = (MERGE ? jobs.merge_out : P.out) + (size_t)sg.row0 * jobs.rate * CP;
    if (MERGE && jb) __syncthreads();               // the previous job's conv2 is done reading the LDS tile

    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int lc = lane & 15, lg = lane >> 4;
    const size_t wseg = (size_t)(round_up(K * NKC, 4) + 8) * 64;        // half8 units per n-tile segment

    // ---- stage X: LDS row r <-> time t0 - h2 - h1 + r   (+ dil rows: the zero-weight tap of CP = 32 must read finite data)
    const __amdgpu_buffer_rsrc_t rs_y = __builtin_amdgcn_make_buffer_rsrc((void *)y_seg, 0, L * CP * 4, 0x00020000);
    constexpr int STAGE_U = MERGE ? 4 : ((CP == 32) ? 10 : (CP == 64 ? 12 : (CP == 128 ? ZV_STAGE_U128 : ZV_STAGE_U256)));
    constexpr bool EARLY_B = CP <= 64 && !MERGE;
    half8 bw[2][NT][2];
    if constexpr (EARLY_B) deep16_preload_b<NT>(bw, (const half8 *)P.w1 + wn * NT * wseg + lane, wseg);
    stage_act_buf<STAGE_U, CP>(rs_y, smem, t0 - h2 - h1, BM + 2 * h1 + dil, tid, P.slope);
    __syncthreads();

    // this lane's fragment rows: block row 2c (+ lt) of the wave's 32-row blocks, k group g
    const char *abase = smem + (wm * 32 * MT + 2 * lc) * RS + lg * 16;
    floatx4 acc[MT][NT][2][2];

    // ---- conv1 (dilated), transposed product: acc[mt][nt][wt][lt][i] = xt_pre[time = mt*32 + 2c + lt][oc = 16 wt + 4g + i]
    if constexpr (!EARLY_B) deep16_preload_b<NT>(bw, (const half8 *)P.w1 + wn * NT * wseg + lane, wseg);
    mfma16_taps_deep<CP, MT, NT, true>(acc, abase, dil * RS, (const half8 *)P.w1 + wn * NT * wseg + lane, wseg, K, bw);
    if constexpr (EARLY_B) deep16_preload_b<NT>(bw, (const half8 *)P.w2 + wn * NT * wseg + lane, wseg);     // conv2's first fragments travel under the xt pack
    __syncthreads();                       // every wave is done reading X: its LDS region becomes XT

    // ---- xt = f16(lrelu(conv1 + b1)), zero outside [0, L); XT row i <-> time t0 - h2 + i
    {
        const float sl = P.slope;
        const bool edge = t0 - h2 < 0 || t0 - h2 + BM > L;
#pragma unroll
        for (int nt = 0; nt < NT; nt++)
        {
            const int ocb = (wn * NT + nt) * 32;
            float4 bq[2];
#pragma unroll
            for (int wt = 0; wt < 2; wt++) bq[wt] = *(const float4 *)(P.b1 + ocb + 16 * wt + 4 * lg);
#pragma unroll
            for (int mt = 0; mt < MT; mt++)
#pragma unroll
                for (int lt = 0; lt < 2; lt++)
                {
                    const int i = wm * 32 * MT + mt * 32 + 2 * lc + lt;
                    const int t = t0 - h2 + i;
                    const bool in = !edge || (t >= 0 && t < L);
#pragma unroll
                    for (int wt = 0; wt < 2; wt++)
                    {
                        half4 h;
                        h[0] = (_Float16)lrelu_max(acc[mt][nt][wt][lt][0] + bq[wt].x, sl);
                        h[1] = (_Float16)lrelu_max(acc[mt][nt][wt][lt][1] + bq[wt].y, sl);
                        h[2] = (_Float16)lrelu_max(acc[mt][nt][wt][lt][2] + bq[wt].z, sl);
                        h[3] = (_Float16)lrelu_max(acc[mt][nt][wt][lt][3] + bq[wt].w, sl);
                        uint2 pk = *(uint2 *)&h;
                        if (edge)
                        {
                            pk.x = in ? pk.x : 0u;
                            pk.y = in ? pk.y : 0u;
                        }
                        *(uint2 *)(smem + i * RS + (ocb + 16 * wt + 4 * lg) * 2) = pk;
                    }
                }
        }
    }
    __syncthreads();

    // ---- conv2 (dil 1): output row j <-> time t0 + j reads XT rows j .. j + 2*h2; rows j >= TM are discarded
    if constexpr (!EARLY_B) deep16_preload_b<NT>(bw, (const half8 *)P.w2 + wn * NT * wseg + lane, wseg);
    mfma16_taps_deep<CP, MT, NT, false>(acc, abase, RS, (const half8 *)P.w2 + wn * NT * wseg + lane, wseg, K, bw);

    // ---- epilogue: out = y + (conv2 + b2).  acc[mt][nt][wt][lt][i] = time row mt*32 + 8g + 2i + lt, channel 2c + wt: the lane's two
    // weight tiles are neighbouring channels -> 8-byte accesses, four rows x 128 bytes per instruction.  Buffer descriptors over
    // exactly this tile's valid rows: row >= TM or time >= L is out of range (loads give 0, stores are dropped).
    const int nrows = (L - t0 < TM) ? (L - t0) : TM;
    const __amdgpu_buffer_rsrc_t rs_res = __builtin_amdgcn_make_buffer_rsrc((void *)(y_seg + (size_t)t0 * CP), 0, nrows * CP * 4, 0x00020000);
    float *const outp = (!MERGE && P.sum_out) ? P.sum_out + (size_t)sg.row0 * jobs.rate * CP : out_seg;
    const __amdgpu_buffer_rsrc_t rs_out = __builtin_amdgcn_make_buffer_rsrc((void *)(outp + (size_t)t0 * CP), 0, nrows * CP * 4, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_sum = __builtin_amdgcn_make_buffer_rsrc(
        (void *)((P.sum_in ? P.sum_in : y_seg) + (P.sum_in ? (size_t)sg.row0 * jobs.rate * CP : 0) + (size_t)t0 * CP), 0, nrows * CP * 4, 0x00020000);
    typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
#pragma unroll
    for (int nt = 0; nt < NT; nt++)
    {
        const int oc = (wn * NT + nt) * 32 + 2 * lc;
        const float2 bias = *(const float2 *)(P.b2 + oc);
        const int voff = ((wm * 32 * MT + 8 * lg) * CP + oc) * 4;
#pragma unroll
        for (int mt = 0; mt < MT; mt++)
        {
            u32x2 resv[2][4];
#pragma unroll
            for (int lt = 0; lt < 2; lt++)
#pragma unroll
                for (int i = 0; i < 4; i++)
                    resv[lt][i] = __builtin_amdgcn_raw_buffer_load_b64(rs_res, voff, (mt * 32 + 2 * i + lt) * CP * 4, 0);
            u32x2 sumv[2][4];
            if (!MERGE && P.sum_out && P.sum_in)
#pragma unroll
                for (int lt = 0; lt < 2; lt++)
#pragma unroll
                    for (int i = 0; i < 4; i++)
                        sumv[lt][i] = __builtin_amdgcn_raw_buffer_load_b64(rs_sum, voff, (mt * 32 + 2 * i + lt) * CP * 4, 0);
#pragma unroll
            for (int lt = 0; lt < 2; lt++)
#pragma unroll
                for (int i = 0; i < 4; i++)
                {
                    float v0 = (acc[mt][nt][0][lt][i] + bias.x) + __uint_as_float(resv[lt][i][0]);
                    float v1 = (acc[mt][nt][1][lt][i] + bias.y) + __uint_as_float(resv[lt][i][1]);
                    if constexpr (MERGE)
                    {
                        msum[mt][nt][0][lt][i] = jb == 0 ? v0 : msum[mt][nt][0][lt][i] + v0;
                        msum[mt][nt][1][lt][i] = jb == 0 ? v1 : msum[mt][nt][1][lt][i] + v1;
                        if (jb != jobs.njobs - 1) continue;
                        v0 = msum[mt][nt][0][lt][i];
                        v1 = msum[mt][nt][1][lt][i];
                    }
                    else if (P.sum_out && P.sum_in)
                    {
                        // this branch's term of the MRF sum: sum_out = sum_in + v (the first branch stores v itself)
                        v0 = __uint_as_float(sumv[lt][i][0]) + v0;
                        v1 = __uint_as_float(sumv[lt][i][1]) + v1;
                    }
                    const u32x2 o = {__float_as_uint(v0), __float_as_uint(v1)};
                    __builtin_amdgcn_raw_buffer_store_b64(o, rs_out, voff, (mt * 32 + 2 * i + lt) * CP * 4, ZV_ST_AUX);
                }
        }
    }
    }
}

#ifdef ZV_STAMPS
__device__ unsigned long long zv_stamp_buf[(size_t)ZV_STAMP_WGS * ZV_STAMP_N];

unsigned long long *stamp_buffer()
{
    void *p = nullptr;
    return hipGetSymbolAddress(&p, HIP_SYMBOL(zv_stamp_buf)) == hipSuccess ? (unsigned long long *)p : nullptr;
}

extern "C" int zv_debug_read_stamps(unsigned long long *out, size_t n)
{
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(zv_stamp_buf), n * sizeof(unsigned long long), 0, hipMemcpyDeviceToHost);
}
#endif

// ---------------------------------------------------------------------------------------------------
// The fused dilation pair of the 64-channel stage for batches: weights through an LDS ring.
// In resblock_pair_kernel<64> every wave streams its own copy of every B fragment from L1 (1 KiB per two MFMAs per wave,
// the two row halves of a workgroup fetching the same fragments twice): at the matrix pipe's full rate that alone is the
// whole 64 B/clk of the CU's vector-memory path, which the staging loads, the residual loads and the stores share — the
// MFMA loops run at 40 % of the pipe's rate (measured: 0.87 ms per launch against 0.36 ms of MFMA time).  Here
//   * a workgroup is 4 waves x (64 rows x all 64 channels) = 256 rows (halo recompute 1.04 instead of 1.08 at 11 taps),
//   * the weights of both convs travel global -> LDS once per workgroup as one stream of 2K chunks (one tap = 8 fragments
//     = 8 KiB each) through a ring of four slots, by LDS-DMA, two chunks ahead of the MFMAs (one workgroup barrier per
//     tap; the stream keeps running under the xt pack),
//   * both MFMA operands are ds_read_b128s two steps ahead; one A fragment feeds two MFMAs and so does one B fragment.
// Vector-memory bytes per output row fall 5x.  Same operations in the same order per output element as
// resblock_pair_kernel (tap-major, 16 channels per step), hence the same bits.
// Weight layout (pack_pair_weight_ring): [tap][kc][ntile][lane][8 halfs].
size_t pair_ring_weight_halfs(int Cp, int K) { return (size_t)K * (Cp / 16) * (Cp / 32) * 512; }

// the ring stream in v_mfma_f32_16x16x32_f16 fragment order (resblock_pair64_kernel / resblock_block64_kernel): [tap][step of 32
// channels][ntile][wt][lane][8 halfs]; conv2_layout as in pack_pair_weight16
void pack_pair_weight_ring(const uint16_t *w, int K, int C, int Cp, uint16_t *dst, bool conv2_layout)
{
    const int nk2 = Cp / 32, nnt = Cp / 32;
    for (int tap = 0; tap < K; tap++)
        for (int k2 = 0; k2 < nk2; k2++)
            for (int nt = 0; nt < nnt; nt++)
                for (int wt = 0; wt < 2; wt++)
                {
                    uint16_t *d = dst + ((((size_t)(tap * nk2 + k2) * nnt + nt) * 2) + wt) * 512;
                    for (int lane = 0; lane < 64; lane++)
                        for (int j = 0; j < 8; j++)
                        {
                            const int r = lane & 15, g = lane >> 4;
                            const int oc = nt * 32 + (conv2_layout ? 2 * r + wt : 16 * wt + r), ic = k2 * 32 + 8 * g + j;
                            d[lane * 8 + j] = (oc < C && ic < C) ? w[((size_t)oc * C + ic) * K + tap] : (uint16_t)0;
                        }
                }
}

template <bool MERGE>
__global__ __launch_bounds__(256, 2) void resblock_pair64_kernel(const PairJobs jobs)
{
    constexpr int CP = 64, MT = 2, NT = 2, BM = 256, RS = CP * 2 + 16;
    constexpr int CHUNK = 8 * 1024;                  // one tap: 4 channel steps x 2 output tiles
    const int jz = (int)blockIdx.z, bx = (int)blockIdx.x;
    const int TM = BM - (MERGE ? jobs.kmax - 1 : jobs.j[jz].K - 1);
    const int tps = (jobs.segs.max_rows * jobs.rate + TM - 1) / TM;
    const int vt = tile_deal(bx, tps, jobs.segs.nseg, jobs.deal_c);
    if (vt >= tps * jobs.segs.nseg) return;
    const int useg = vt / tps;
    const Seg sg = seg_at(jobs.segs, useg);
    const int L = sg.rows * jobs.rate;
    const int t0 = (vt - useg * tps) * TM;
    if (t0 >= L) return;

#ifdef ZV_STAMPS
    const int stamp_wg = (int)(blockIdx.x + gridDim.x * blockIdx.z);
    if (jobs.stamp && threadIdx.x == 0 && stamp_wg < ZV_STAMP_WGS)
    {
        jobs.stamp[(size_t)stamp_wg * ZV_STAMP_N + 8] = __builtin_amdgcn_s_getreg(63492);      // HW_ID
        jobs.stamp[(size_t)stamp_wg * ZV_STAMP_N + 9] = __builtin_amdgcn_s_getreg(63508);      // XCC_ID
    }
#endif
    ZV_STAMP(0)
    extern __shared__ __attribute__((aligned(1024))) char smem[];
    char *ring = smem + jobs.ring_off;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lc = lane & 15, lg = lane >> 4;
    const char *abase = smem + (wave * 32 * MT + 2 * lc) * RS + lg * 16;      // block row 2c (+ lt), k group g (see resblock_pair_kernel)
    const char *bl = ring + lane * 16;

    floatx4 msum[MERGE ? MT : 1][MERGE ? NT : 1][2][2];
    for (int jb = MERGE ? 0 : jz; jb < (MERGE ? jobs.njobs : jz + 1); jb++)
    {
        const PairJob &P = jobs.j[jb];
        const int K = P.K, dil = P.dil;
        const int h2 = (K - 1) / 2, h1 = h2 * dil;
        const float *y_seg = P.y + (size_t)sg.row0 * jobs.rate * CP;
        float *out_seg = (MERGE ? jobs.merge_out : P.out) + (size_t)sg.row0 * jobs.rate * CP;
        const int nchunk = 2 * K;
        // chunk g of the pair's weight stream (conv1's taps, then conv2's) -> ring slot g & 3; a wave moves 2 of its 8 fragments
        // (the stream's base pointers pinned in scalar registers: re-reading them from the kernel arguments at every request
        // would put an lgkmcnt(0) wait — which also waits for the LDS reads in flight — into every tap)
        const uint64_t w1a = (uint64_t)P.w1r + wave * 2048, w2a = (uint64_t)P.w2r + wave * 2048 - (uint64_t)K * CHUNK;
        const uint32_t w1lo = __builtin_amdgcn_readfirstlane((uint32_t)w1a), w1hi = __builtin_amdgcn_readfirstlane((uint32_t)(w1a >> 32));
        const uint32_t w2lo = __builtin_amdgcn_readfirstlane((uint32_t)w2a), w2hi = __builtin_amdgcn_readfirstlane((uint32_t)(w2a >> 32));
        auto issue = [&](int g) {
            const uint64_t base = g < K ? ((uint64_t)w1hi << 32 | w1lo) : ((uint64_t)w2hi << 32 | w2lo);
            const char *src = (const char *)base + (size_t)g * CHUNK + lane * 16;
            char *dst = ring + (g & 3) * CHUNK + wave * 2048;
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)src, (__attribute__((address_space(3))) void *)dst, 16, 0, 0);
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(src + 1024), (__attribute__((address_space(3))) void *)(dst + 1024), 16, 0, 0);
        };
        if (MERGE && jb) __syncthreads();               // the previous job's conv2 is done reading the tile and the ring
        issue(0);
        issue(1);
        issue(2);

        // ---- stage X: LDS row r <-> time t0 - h2 - h1 + r
        const __amdgpu_buffer_rsrc_t rs_y = __builtin_amdgcn_make_buffer_rsrc((void *)y_seg, 0, L * CP * 4, 0x00020000);
        // (two workgroups per CU whatever the register count — LDS decides — so every staging load of the tile is in flight at once)
        stage_act_buf<20, CP>(rs_y, smem, t0 - h2 - h1, BM + 2 * h1 + dil, tid, P.slope);
        // the residual operand (the tile's centre rows again, in the accumulator layout) is requested right behind the
        // staging loads, while their lines are still in L2, and waits in registers until the epilogue
        const int nrows = (L - t0 < TM) ? (L - t0) : TM;
        const __amdgpu_buffer_rsrc_t rs_res = __builtin_amdgcn_make_buffer_rsrc((void *)(y_seg + (size_t)t0 * CP), 0, nrows * CP * 4, 0x00020000);
        // conv2's accumulator layout: [mt][nt][wt][lt][i] = time row mt*32 + 8g + 2i + lt, channel nt*32 + 2c + wt — 8 bytes per lane
        const int voff0 = ((wave * 32 * MT + 8 * lg) * CP + 2 * lc) * 4;
        typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
        u32x2 resv[MT][NT][2][4];
        auto load_res = [&]() {
#pragma unroll
            for (int nt = 0; nt < NT; nt++)
#pragma unroll
                for (int mt = 0; mt < MT; mt++)
#pragma unroll
                    for (int lt = 0; lt < 2; lt++)
#pragma unroll
                        for (int i = 0; i < 4; i++)
                            resv[mt][nt][lt][i] = __builtin_amdgcn_raw_buffer_load_b64(rs_res, voff0 + nt * 128, (mt * 32 + 2 * i + lt) * CP * 4, 0);
        };
        if constexpr (!MERGE) load_res();      // (the merged form holds the branches' running sum: it loads in the epilogue)
        ZV_STAMP(1)
        __syncthreads();                                // X complete; the barrier drains the first three chunks too
        ZV_STAMP(2)

        floatx4 acc[MT][NT][2][2];
        half8 a[2][MT][2], b[2][NT][2];
        int g = 0;                                      // chunk = tap of the stream
        // one step = 32 channels: the operand's two 16-row tiles per 32-row block (rows 2c + lt), the weights' two 16-channel tiles per
        // output tile, both from LDS; a chunk = [step 2][nt 2][wt 2] fragments
#define ZV_LDR(slot, aptr, boff)                                                                                      \
    {                                                                                                                 \
        const char *ap_ = (aptr);                                                                                     \
        _Pragma("unroll") for (int mt = 0; mt < MT; mt++)                                                             \
            _Pragma("unroll") for (int lt = 0; lt < 2; lt++) a[slot][mt][lt] = *(const half8 *)(ap_ + (mt * 32 + lt) * RS);    \
        _Pragma("unroll") for (int nt = 0; nt < NT; nt++)                                                             \
            _Pragma("unroll") for (int wt = 0; wt < 2; wt++) b[slot][nt][wt] = *(const half8 *)(bp_ + (boff) + (nt * 2 + wt) * 1024); \
    }
#define ZV_MF(slot, SW, Z)                                \
    mfma16_step<MT, NT, SW, Z>(acc, a[slot], b[slot]);    \
    __builtin_amdgcn_sched_barrier(0);
        // one tap: step 0 | wait for the next chunk, barrier, request the chunk three ahead | step 1 (which already reads the
        // next tap's first fragments)
#define ZV_TAP(SW, Z0, tapstride)                                                                         \
    {                                                                                                     \
        const char *bp_ = bl + (g & 3) * CHUNK, *bn_ = bl + ((g + 1) & 3) * CHUNK;                        \
        ZV_LDR(1, ap + 64, 4 * 1024) ZV_MF(0, SW, Z0)                                                     \
        if (g + 2 < nchunk) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");                              \
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                             \
        __builtin_amdgcn_s_barrier();                                                                     \
        if (g + 3 < nchunk) issue(g + 3);                                                                 \
        __builtin_amdgcn_sched_barrier(0);                                                                \
        ap += (tapstride);                                                                                \
        bp_ = bn_;                                                                                        \
        ZV_LDR(0, ap, 0) ZV_MF(1, SW, false)                                                              \
        g++;                                                                                              \
    }
        // ---- conv1 (dilated), transposed product
        {
            const char *ap = abase;
            {
                const char *bp_ = bl;
                ZV_LDR(0, ap, 0)
            }
            ZV_TAP(true, true, dil * RS)
            for (int tap = 1; tap < K; tap++) ZV_TAP(true, false, dil * RS)
        }
        ZV_STAMP(3)
        // every wave is done reading X: its LDS region becomes XT (raw barriers here: __syncthreads would drain the weight
        // stream, whose next chunks are in flight under the pack)
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();

        ZV_STAMP(4)
        // ---- xt = f16(lrelu(conv1 + b1)), zero outside [0, L); XT row i <-> time t0 - h2 + i.  acc[mt][nt][wt][lt][i]: time row
        // mt*32 + 2c + lt, channel nt*32 + 16 wt + 4g + i
        {
            const float sl = P.slope;
            const bool edge = t0 - h2 < 0 || t0 - h2 + BM > L;
#pragma unroll
            for (int nt = 0; nt < NT; nt++)
            {
                float4 bq[2];
#pragma unroll
                for (int wt = 0; wt < 2; wt++) bq[wt] = *(const float4 *)(P.b1 + nt * 32 + 16 * wt + 4 * lg);
#pragma unroll
                for (int mt = 0; mt < MT; mt++)
#pragma unroll
                    for (int lt = 0; lt < 2; lt++)
                    {
                        const int i = wave * 32 * MT + mt * 32 + 2 * lc + lt;
                        const int t = t0 - h2 + i;
                        const bool in = !edge || (t >= 0 && t < L);
#pragma unroll
                        for (int wt = 0; wt < 2; wt++)
                        {
                            uint2 pk = lrelu4_f16(acc[mt][nt][wt][lt][0] + bq[wt].x, acc[mt][nt][wt][lt][1] + bq[wt].y,
                                                  acc[mt][nt][wt][lt][2] + bq[wt].z, acc[mt][nt][wt][lt][3] + bq[wt].w, sl);
                            if (edge)
                            {
                                pk.x = in ? pk.x : 0u;
                                pk.y = in ? pk.y : 0u;
                            }
                            *(uint2 *)(smem + i * RS + (nt * 32 + 16 * wt + 4 * lg) * 2) = pk;
                        }
                    }
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();

        ZV_STAMP(5)
        // ---- conv2 (dil 1): output row j <-> time t0 + j reads XT rows j .. j + 2*h2; rows j >= TM are discarded
        {
            const char *ap = abase;
            {
                const char *bp_ = bl + (g & 3) * CHUNK;
                ZV_LDR(0, ap, 0)
            }
            ZV_TAP(false, true, RS)
            for (int tap = 1; tap < K; tap++) ZV_TAP(false, false, RS)
        }
#undef ZV_TAP
#undef ZV_MF
#undef ZV_LDR

        // ---- epilogue: out = y + (conv2 + b2); descriptors over exactly this tile's valid rows (see resblock_pair_kernel)
        ZV_STAMP(6)
        if constexpr (MERGE) load_res();
        const __amdgpu_buffer_rsrc_t rs_out = __builtin_amdgcn_make_buffer_rsrc((void *)(out_seg + (size_t)t0 * CP), 0, nrows * CP * 4, 0x00020000);
#pragma unroll
        for (int nt = 0; nt < NT; nt++)
        {
            const float2 bias = *(const float2 *)(P.b2 + nt * 32 + 2 * lc);
            const int voff = voff0 + nt * 128;
#pragma unroll
            for (int mt = 0; mt < MT; mt++)
#pragma unroll
                for (int lt = 0; lt < 2; lt++)
#pragma unroll
                    for (int i = 0; i < 4; i++)
                    {
                        float v0 = (acc[mt][nt][0][lt][i] + bias.x) + __uint_as_float(resv[mt][nt][lt][i][0]);
                        float v1 = (acc[mt][nt][1][lt][i] + bias.y) + __uint_as_float(resv[mt][nt][lt][i][1]);
                        if constexpr (MERGE)
                        {
                            msum[mt][nt][0][lt][i] = jb == 0 ? v0 : msum[mt][nt][0][lt][i] + v0;
                            msum[mt][nt][1][lt][i] = jb == 0 ? v1 : msum[mt][nt][1][lt][i] + v1;
                            if (jb != jobs.njobs - 1) continue;
                            v0 = msum[mt][nt][0][lt][i];
                            v1 = msum[mt][nt][1][lt][i];
                        }
                        const u32x2 o = {__float_as_uint(v0), __float_as_uint(v1)};
                        __builtin_amdgcn_raw_buffer_store_b64(o, rs_out, voff, (mt * 32 + 2 * i + lt) * CP * 4, ZV_ST_AUX);
                    }
        }
#ifdef ZV_STAMPS
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
        ZV_STAMP(7)
    }
}

// ---------------------------------------------------------------------------------------------------
// resblock_block64_kernel — SEVERAL dilation pairs of a 64-channel residual block in one launch, for the branches whose halo is
// small (3 taps: 2 rows per pair and dilation step): resblock_pair64_kernel's machinery (weights of every conv through the
// four-slot LDS ring as ONE stream over all the pairs, both operands from LDS, 64 x 64 per wave) around resblock_block32_kernel's
// data flow (the f32 tile stays in registers in the accumulator layout — it is the residual operand of every pair —, the f16
// operand tile is regenerated in LDS per pair, every conv runs over the full 256-row tile as a zero-padded sequence and only
// the TM = 256 - 2H centre rows are stored).  The branch's tensor crosses HBM once per block instead of once per pair.
// Same operations in the same order per output element as the pair kernels: same bits.
__global__ __launch_bounds__(256, 2) void resblock_block64_kernel(const TripleJobs jobs)
{
    constexpr int CP = 64, MT = 2, NT = 2, BM = 256, RS = CP * 2 + 16;
    constexpr int CHUNK = 8 * 1024;
    const TripleJob &P = jobs.j[blockIdx.z];
    const int K = P.K, nd = P.n_dil;
    const int h2 = (K - 1) / 2;
    int sumd = 0, dmax = 1;
    for (int d = 0; d < nd; d++) { sumd += P.dil[d]; dmax = P.dil[d] > dmax ? P.dil[d] : dmax; }
    const int H = h2 * (sumd + nd);
    const int TM = BM - 2 * H;
    const int tps = (jobs.segs.max_rows * jobs.rate + TM - 1) / TM;
    const int vt = tile_deal((int)blockIdx.x, tps, jobs.segs.nseg, jobs.deal_c);
    if (vt >= tps * jobs.segs.nseg) return;
    const int useg = vt / tps;
    const Seg sg = seg_at(jobs.segs, useg);
    const int L = sg.rows * jobs.rate;
    const int t0 = (vt - useg * tps) * TM;
    if (t0 >= L) return;
    const float *y_seg = P.y + (size_t)sg.row0 * jobs.rate * CP;
    float *out_seg = P.out + (size_t)sg.row0 * jobs.rate * CP;
    const int XM = h2 * dmax;                         // zero margin of the operand region on either side of the tile
    const int xrows = BM + 2 * XM + 2 * dmax;         // + slack: the last tap's look-ahead reads one tap past the end
    const bool edge = t0 - H < 0 || t0 - H + BM > L;

    extern __shared__ __attribute__((aligned(1024))) char smem[];
    char *ring = smem + jobs.ring_off;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lc = lane & 15, lg = lane >> 4;
    const char *abase = smem + (wave * 32 * MT + 2 * lc) * RS + lg * 16;      // block row 2c (+ lt), k group g (see resblock_pair_kernel)
    const char *bl = ring + lane * 16;
    const int nchunk = 2 * K * nd;                    // the block's weight stream: per pair conv1's taps, then conv2's
    // chunk g -> ring slot g & 3; base pointers of the (at most six) convs in scalar registers
    uint32_t wlo[2 * TRIPLE_MAX_DIL], whi[2 * TRIPLE_MAX_DIL];
#pragma unroll
    for (int c = 0; c < 2 * TRIPLE_MAX_DIL; c++)
    {
        const int d = c >> 1 < nd ? c >> 1 : 0;
        const uint64_t a = (uint64_t)((c & 1) ? P.w2[d] : P.w1[d]) + wave * 2048;
        wlo[c] = __builtin_amdgcn_readfirstlane((uint32_t)a);
        whi[c] = __builtin_amdgcn_readfirstlane((uint32_t)(a >> 32));
    }
    auto issue = [&](int g) {
        const int c = g / K, tap = g - c * K;         // conv index (2 * pair + conv), tap
        uint32_t lo = wlo[0], hi = whi[0];
#pragma unroll
        for (int q = 1; q < 2 * TRIPLE_MAX_DIL; q++)
            if (c == q) { lo = wlo[q]; hi = whi[q]; }
        const char *src = (const char *)((uint64_t)hi << 32 | lo) + (size_t)tap * CHUNK + lane * 16;
        char *dst = ring + (g & 3) * CHUNK + wave * 2048;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)src, (__attribute__((address_space(3))) void *)dst, 16, 0, 0);
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(src + 1024), (__attribute__((address_space(3))) void *)(dst + 1024), 16, 0, 0);
    };
    issue(0);
    issue(1);
    issue(2);
    // the whole operand region starts as zeros (margins stay zero for the whole kernel; nothing in it is ever uninitialised)
    for (int i = tid; i < xrows * RS / 16; i += 256) ((uint4 *)smem)[i] = make_uint4(0, 0, 0, 0);
    // tile row i <-> time t0 - H + i; register [mt][nt][wt][lt][i] (conv2's accumulator layout): row wave*64 + mt*32 + 8g + 2i + lt,
    // channel nt*32 + 2c + wt — the lane's two weight tiles are neighbouring channels: 8-byte loads / stores, 4-byte operand writes
    typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
    float yreg[MT][NT][2][2][4];
    {
        const __amdgpu_buffer_rsrc_t rs_y = __builtin_amdgcn_make_buffer_rsrc((void *)y_seg, 0, L * CP * 4, 0x00020000);
        const int voff = ((t0 - H + wave * 32 * MT + 8 * lg) * CP + 2 * lc) * 4;
#pragma unroll
        for (int nt = 0; nt < NT; nt++)
#pragma unroll
            for (int mt = 0; mt < MT; mt++)
#pragma unroll
                for (int lt = 0; lt < 2; lt++)
#pragma unroll
                    for (int i = 0; i < 4; i++)
                    {
                        const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(rs_y, voff + nt * 128 + (mt * 32 + 2 * i + lt) * CP * 4, 0, 0);
                        yreg[mt][nt][0][lt][i] = __uint_as_float(v[0]);
                        yreg[mt][nt][1][lt][i] = __uint_as_float(v[1]);
                    }
    }
    __syncthreads();                                  // zeros written (and the first chunks landed)
    const float sl = P.slope;
    int g = 0;
    floatx4 acc[MT][NT][2][2];
    half8 a[2][MT][2], b[2][NT][2];
#define ZV_LDR(slot, aptr, boff)                                                                                      \
    {                                                                                                                 \
        const char *ap_ = (aptr);                                                                                     \
        _Pragma("unroll") for (int mt = 0; mt < MT; mt++)                                                             \
            _Pragma("unroll") for (int lt = 0; lt < 2; lt++) a[slot][mt][lt] = *(const half8 *)(ap_ + (mt * 32 + lt) * RS);    \
        _Pragma("unroll") for (int nt = 0; nt < NT; nt++)                                                             \
            _Pragma("unroll") for (int wt = 0; wt < 2; wt++) b[slot][nt][wt] = *(const half8 *)(bp_ + (boff) + (nt * 2 + wt) * 1024); \
    }
#define ZV_MF(slot, SW, Z)                                \
    mfma16_step<MT, NT, SW, Z>(acc, a[slot], b[slot]);    \
    __builtin_amdgcn_sched_barrier(0);
#define ZV_TAP(SW, Z0, tapstride)                                                                         \
    {                                                                                                     \
        const char *bp_ = bl + (g & 3) * CHUNK, *bn_ = bl + ((g + 1) & 3) * CHUNK;                        \
        ZV_LDR(1, ap + 64, 4 * 1024) ZV_MF(0, SW, Z0)                                                     \
        if (g + 2 < nchunk) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");                              \
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                             \
        __builtin_amdgcn_s_barrier();                                                                     \
        if (g + 3 < nchunk) issue(g + 3);                                                                 \
        __builtin_amdgcn_sched_barrier(0);                                                                \
        ap += (tapstride);                                                                                \
        bp_ = bn_;                                                                                        \
        ZV_LDR(0, ap, 0) ZV_MF(1, SW, false)                                                              \
        g++;                                                                                              \
    }
    for (int d = 0; d < nd; d++)
    {
        const int dil = P.dil[d], h1 = h2 * dil;
        // ---- X = f16(lrelu(Y)) into region rows XM .. XM + BM - 1 (Y is zero outside [0, L): so is X)
        {
#pragma unroll
            for (int nt = 0; nt < NT; nt++)
#pragma unroll
                for (int mt = 0; mt < MT; mt++)
#pragma unroll
                    for (int lt = 0; lt < 2; lt++)
#pragma unroll
                        for (int i = 0; i < 4; i++)
                        {
                            const int row = wave * 32 * MT + mt * 32 + 8 * lg + 2 * i + lt;
                            half2v h;
                            h[0] = (_Float16)lrelu_max(yreg[mt][nt][0][lt][i], sl);
                            h[1] = (_Float16)lrelu_max(yreg[mt][nt][1][lt][i], sl);
                            *(half2v *)(smem + (XM + row) * RS + (nt * 32 + 2 * lc) * 2) = h;
                        }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();                 // (raw: the weight stream stays in flight)
        // ---- conv1 (dilated), transposed product; output tile row i reads region rows XM + i - h1 + tap * dil
        {
            const char *ap = abase + (XM - h1) * RS;
            {
                const char *bp_ = bl + (g & 3) * CHUNK;
                ZV_LDR(0, ap, 0)
            }
            ZV_TAP(true, true, dil * RS)
            for (int tap = 1; tap < K; tap++) ZV_TAP(true, false, dil * RS)
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();                 // every wave is done reading X: its rows become XT
        // ---- xt = f16(lrelu(conv1 + b1)), zero outside [0, L): acc[mt][nt][wt][lt][i] = time row mt*32 + 2c + lt, channel nt*32 + 16 wt + 4g + i
        {
            const float *b1 = P.b1[d];
#pragma unroll
            for (int nt = 0; nt < NT; nt++)
            {
                float4 bq[2];
#pragma unroll
                for (int wt = 0; wt < 2; wt++) bq[wt] = *(const float4 *)(b1 + nt * 32 + 16 * wt + 4 * lg);
#pragma unroll
                for (int mt = 0; mt < MT; mt++)
#pragma unroll
                    for (int lt = 0; lt < 2; lt++)
                    {
                        const int i = wave * 32 * MT + mt * 32 + 2 * lc + lt;
                        const int t = t0 - H + i;
                        const bool in = !edge || (t >= 0 && t < L);
#pragma unroll
                        for (int wt = 0; wt < 2; wt++)
                        {
                            uint2 pk = lrelu4_f16(acc[mt][nt][wt][lt][0] + bq[wt].x, acc[mt][nt][wt][lt][1] + bq[wt].y,
                                                  acc[mt][nt][wt][lt][2] + bq[wt].z, acc[mt][nt][wt][lt][3] + bq[wt].w, sl);
                            if (edge)
                            {
                                pk.x = in ? pk.x : 0u;
                                pk.y = in ? pk.y : 0u;
                            }
                            *(uint2 *)(smem + (XM + i) * RS + (nt * 32 + 16 * wt + 4 * lg) * 2) = pk;
                        }
                    }
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        // ---- conv2 (dil 1): output tile row i reads region rows XM + i - h2 + tap;  Y = Y + (conv2 + b2), 0 outside [0, L)
        {
            const char *ap = abase + (XM - h2) * RS;
            {
                const char *bp_ = bl + (g & 3) * CHUNK;
                ZV_LDR(0, ap, 0)
            }
            ZV_TAP(false, true, RS)
            for (int tap = 1; tap < K; tap++) ZV_TAP(false, false, RS)
        }
        {
            const float *b2 = P.b2[d];
#pragma unroll
            for (int nt = 0; nt < NT; nt++)
            {
                const float2 bias = *(const float2 *)(b2 + nt * 32 + 2 * lc);
#pragma unroll
                for (int mt = 0; mt < MT; mt++)
#pragma unroll
                    for (int lt = 0; lt < 2; lt++)
#pragma unroll
                        for (int i = 0; i < 4; i++)
                        {
                            const float v0 = (acc[mt][nt][0][lt][i] + bias.x) + yreg[mt][nt][0][lt][i];
                            const float v1 = (acc[mt][nt][1][lt][i] + bias.y) + yreg[mt][nt][1][lt][i];
                            bool in = true;
                            if (edge)
                            {
                                const int t = t0 - H + wave * 32 * MT + mt * 32 + 8 * lg + 2 * i + lt;
                                in = t >= 0 && t < L;
                            }
                            yreg[mt][nt][0][lt][i] = in ? v0 : 0.f;
                            yreg[mt][nt][1][lt][i] = in ? v1 : 0.f;
                        }
            }
        }
        if (d + 1 < nd)
        {
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();             // every wave is done reading XT before the next X goes over it
        }
    }
#undef ZV_TAP
#undef ZV_MF
#undef ZV_LDR
    // ---- store the centre rows (tile rows H .. H + TM - 1, time < L): anything else gets an out-of-range offset
    const __amdgpu_buffer_rsrc_t rs_out = __builtin_amdgcn_make_buffer_rsrc((void *)out_seg, 0, L * CP * 4, 0x00020000);
#pragma unroll
    for (int nt = 0; nt < NT; nt++)
#pragma unroll
        for (int mt = 0; mt < MT; mt++)
#pragma unroll
            for (int lt = 0; lt < 2; lt++)
#pragma unroll
                for (int i = 0; i < 4; i++)
                {
                    const int row = wave * 32 * MT + mt * 32 + 8 * lg + 2 * i + lt;
                    const int t = t0 - H + row;
                    const int voff = (row >= H && row < H + TM && t >= 0) ? (t * CP + nt * 32 + 2 * lc) * 4 : -8;
                    const u32x2 o = {__float_as_uint(yreg[mt][nt][0][lt][i]), __float_as_uint(yreg[mt][nt][1][lt][i])};
                    __builtin_amdgcn_raw_buffer_store_b64(o, rs_out, voff, 0, ZV_ST_AUX);
                }
}

// a block as conv_plan.h reads it
static inline BlockDesc block_desc(const TripleJob &P)
{
    BlockDesc b{P.Cp, P.K, P.n_dil, {0, 0, 0}};
    for (int d = 0; d < P.n_dil && d < TRIPLE_MAX_DIL; d++) b.dil[d] = P.dil[d];
    return b;
}

hipError_t launch_block64(hipStream_t s, const TripleJob *jobs, int njobs, const Segs &segs, int rate)
{
    if (njobs < 1 || njobs > PAIR_MAX_JOBS || segs.nseg < 1 || segs.max_rows < 1) return hipErrorInvalidValue;
    TripleJobs js;
    BlockDesc desc[PAIR_MAX_JOBS];
    for (int i = 0; i < njobs; i++)
    {
        js.j[i] = jobs[i];
        js.j[i].dbg = 0;
        desc[i] = block_desc(jobs[i]);
    }
    for (int i = njobs; i < PAIR_MAX_JOBS; i++) js.j[i] = js.j[0];
    const Block64Plan p = block64_plan(desc, ConvCall{njobs, segs.nseg, segs.max_rows, rate, 0, 0});
    if (!p.valid) return hipErrorInvalidValue;
    js.segs = segs;
    js.rate = rate;
    js.interleave = 1;
    js.db_mask = 0;
    js.deal_c = p.deal_c;
    js.ring_off = p.ring_off;
    return launch_lds(resblock_block64_kernel, dim3(p.gx, 1, p.gz), dim3(p.threads), p.lds_bytes, s, js);
}

template <int CP, int MT, bool MERGE>
static hipError_t launch_pair_cfg(hipStream_t s, const PairJobs &js, const PairPlan &p)
{
    size_t lds = p.lds_bytes;
#ifdef ZV_DIAG
    lds += (size_t)knob(ZV_LDS_PAD);       // diagnostic build: extra bytes of LDS per workgroup = a lower occupancy on purpose
#endif
    return launch_lds(resblock_pair_kernel<CP, MT, MERGE>, dim3(p.gx, 1, p.gz), dim3(256), lds, s, js);
}

// validate, plan (conv_plan.h pair_plan: the ring form, the tile height), fill the job table, dispatch
hipError_t launch_pair(hipStream_t s, const PairJob *jobs, int njobs, int n_cu, const Segs &segs, int rate, float *merge_out)
{
    if (njobs < 1 || njobs > PAIR_MAX_JOBS || segs.nseg < 1 || segs.max_rows < 1) return hipErrorInvalidValue;
    const int dbg = diag_bits();
    PairJobs js;
    js.segs = segs;
    js.rate = rate;
    js.njobs = njobs;
    js.merge_out = merge_out;
#ifdef ZV_STAMPS
    js.stamp = knob(ZV_STAMP_CP) && knob(ZV_STAMP_CP) == jobs[0].Cp && !merge_out ? stamp_buffer() : nullptr;
#endif
    int  Kmax = 0, dmax = 0;
    bool any_sum = false, all_ring = true;
    for (int i = 0; i < njobs; i++)
    {
        js.j[i] = jobs[i];
        js.j[i].dbg = dbg;
        if (jobs[i].Cp != jobs[0].Cp) return hipErrorInvalidValue;
        Kmax = jobs[i].K > Kmax ? jobs[i].K : Kmax;
        dmax = jobs[i].dil > dmax ? jobs[i].dil : dmax;
        any_sum = any_sum || jobs[i].sum_out || jobs[i].sum_in;
        all_ring = all_ring && jobs[i].w1r && jobs[i].w2r;
    }
    for (int i = njobs; i < PAIR_MAX_JOBS; i++) js.j[i] = js.j[0];
    const int Cp = jobs[0].Cp;
    const PairPlan p = pair_plan(Cp, Kmax, dmax, any_sum, merge_out != nullptr, all_ring, ConvCall{njobs, segs.nseg, segs.max_rows, rate, n_cu, 0});
    if (!p.valid) return hipErrorInvalidValue;
    js.kmax = Kmax;
    js.deal_c = p.deal_c;
    if (p.ring)
    {
        js.ring_off = p.ring_off;
        return merge_out ? launch_lds(resblock_pair64_kernel<true>, dim3(p.gx, 1, p.gz), dim3(256), p.lds_bytes, s, js)
                         : launch_lds(resblock_pair64_kernel<false>, dim3(p.gx, 1, p.gz), dim3(256), p.lds_bytes, s, js);
    }
#define ZV_PCASE(cp, mt)                                                                 \
    if (Cp == cp && p.MT == mt)                                                          \
        return merge_out ? launch_pair_cfg<cp, mt, true>(s, js, p)                       \
                         : launch_pair_cfg<cp, mt, false>(s, js, p);
    ZV_PCASE(32, 4) ZV_PCASE(32, 2) ZV_PCASE(64, 4) ZV_PCASE(64, 2) ZV_PCASE(128, 4) ZV_PCASE(128, 2) ZV_PCASE(256, 2) ZV_PCASE(256, 3) ZV_PCASE(256, 4)
#undef ZV_PCASE
    return hipErrorInvalidValue;
}

// ---------------------------------------------------------------------------------------------------
// Whole residual block in one launch (reference src/hifigan.cpp:99-182, all iterations of the dilation loop).
// The narrow stages are HBM-bound: per dilation pair the fused kernel above reads y (+ halo) and writes y, i.e. the
// block's three pairs move the tile through HBM three times.  Here a workgroup loads a tile of R = 256 rows once
// (f32, in registers) and for every dilation d
//     X  = f16(lrelu(Y))                    (registers -> LDS)
//     xt = f16(lrelu(conv(X, k, d) + b1))   (MFMA, weights as the A operand; packed over X like in the pair kernel)
//     Y += conv(xt, k, 1) + b2              (MFMA; accumulated into the f32 tile)
// All convs run over the full tile as if it were a zero-padded sequence of R rows, so after pair d the rows within
// the cumulative halo of a tile edge are wrong — they never reach the TM = R - 2*H centre rows that are stored
// (H = h2 * (sum(dil) + n_dil), h2 = (k-1)/2).  Rows outside [0, L) are forced to zero after every pair: they are the
// reference's zero padding, not computed values.  Same operations in the same order per output element as the pair
// kernel, hence the same bits.
// LDS: X/XT region rows [0, R + 2*XM + slack), row XM + i <-> tile row i (XM = h2 * max(dil): zero margins, written
// once).  The f32 tile itself stays in registers (see below).
template <int CP, int MT, int R>
__global__ __launch_bounds__(64 * (R / 32 / MT)) void resblock_triple_kernel(const TripleJobs jobs)
{
    // 8 / MT waves, each owns 32*MT tile rows x all CP (= 32) channels; its slice of the f32 tile Y lives in 16*MT
    // registers per lane in the MFMA accumulator layout (row = (r&3) + 8*(r>>2) + 4*(lane>>5), channel = lane & 31)
    // for the whole kernel, so LDS only holds the f16 operand tile (26 KiB: several workgroups per CU).  Every wave
    // streams the same weight fragments (one output tile), MT row tiles per fragment.
    constexpr int NWV = R / 32 / MT, NTH = 64 * NWV;
    constexpr int RS = CP * 2 + 16, NKC = CP / 16;
    static_assert(CP == 32, "one 32-channel output tile per wave");
    const TripleJob &P = jobs.j[blockIdx.z];
    const int K = P.K, nd = P.n_dil;
    const int h2 = (K - 1) / 2;
    int sumd = 0, dmax = 1;
    for (int d = 0; d < nd; d++) { sumd += P.dil[d]; dmax = P.dil[d] > dmax ? P.dil[d] : dmax; }
    const int H = h2 * (sumd + nd);
    const int TM = R - 2 * H;
    const int tps = (jobs.segs.max_rows * jobs.rate + TM - 1) / TM;      // (segment, tile) as in resblock_pair_kernel
    const int vt = tile_deal((int)blockIdx.x, tps, jobs.segs.nseg, jobs.deal_c);
    if (vt >= tps * jobs.segs.nseg) return;
    const int useg = vt / tps;
    const Seg sg = seg_at(jobs.segs, useg);
    const int L = sg.rows * jobs.rate;
    const int t0 = (vt - useg * tps) * TM;
    if (t0 >= L) return;
    const float *y_seg = P.y + (size_t)sg.row0 * jobs.rate * CP;
    float *out_seg = P.out + (size_t)sg.row0 * jobs.rate * CP;
    const int XM = h2 * dmax;
    // only the tiles at a segment's ends hold rows outside [0, L): the others skip every range mask
    const bool edge = t0 - H < 0 || t0 - H + R > L;
    const int xrows = R + 2 * XM + 5 * dmax;          // + slack: zero-weight taps and the last A prefetch read past the margin

    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const size_t wseg = (size_t)(round_up(K * NKC, 4) + 8) * 64;
    const int col = lane & 31;
    const int irow0 = wave * 32 * MT + 4 * (lane >> 5);   // tile row of register [mt][r]: irow0 + mt*32 + (r&3) + 8*(r>>2)

    // ---- zero the X region (its margins stay zero for the whole kernel); load this lane's slice of the tile:
    // tile row i <-> time t0 - H + i, rows outside [0, L) are out of the descriptor's range and read as 0
    for (int i = tid; i < xrows * RS / 16; i += NTH) ((uint4 *)smem)[i] = make_uint4(0, 0, 0, 0);
    float yreg[MT][16];
    {
        const __amdgpu_buffer_rsrc_t rs_y = __builtin_amdgcn_make_buffer_rsrc((void *)y_seg, 0, L * CP * 4, 0x00020000);
        const int voff = ((t0 - H + irow0) * CP + col) * 4;
#pragma unroll
        for (int mt = 0; mt < MT; mt++)
#pragma unroll
            for (int r = 0; r < 16; r++)
                yreg[mt][r] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs_y, voff + (mt * 32 + (r & 3) + 8 * (r >> 2)) * CP * 4, 0, 0));
    }

    const char *abase = smem + (wave * 32 * MT + (lane & 31)) * RS + (lane >> 5) * 16;
    const float sl = P.slope;
    half8 bw[4][1];
    deep_preload_b<1>(bw, (const half8 *)P.w1[0] + lane, wseg);            // the first conv's fragments travel under the tile load
    for (int d = 0; d < nd; d++)
    {
        const int dil = P.dil[d], h1 = h2 * dil;
        __syncthreads();                       // zero fill done / previous conv2 done reading XT
        // ---- X = f16(lrelu(Y)) into region rows XM .. XM + R - 1
        {
            char *xp = smem + (XM + irow0) * RS + col * 2;
#pragma unroll
            for (int mt = 0; mt < MT; mt++)
#pragma unroll
                for (int r = 0; r < 16; r++)
                    *(_Float16 *)(xp + (mt * 32 + (r & 3) + 8 * (r >> 2)) * RS) = (_Float16)lrelu_max(yreg[mt][r], sl);
        }
        __syncthreads();

        // ---- conv1 (dilated), transposed product; output tile row i reads region rows XM + i - h1 + tap*dil
        floatx16 acc[MT][1];
        if (ZV_DBGBITS(P.dbg) & 2)      // timing ablation only: the MFMA loops (which start the accumulators from 0) are skipped
#pragma unroll
            for (int mt = 0; mt < MT; mt++)
#pragma unroll
                for (int r = 0; r < 16; r++) acc[mt][0][r] = 0.f;
        if (!(ZV_DBGBITS(P.dbg) & 2))
            mfma_taps_deep<CP, MT, 1, true>(acc, abase + (XM - h1) * RS, dil * RS, (const half8 *)P.w1[d] + lane, wseg, K, bw);
        deep_preload_b<1>(bw, (const half8 *)P.w2[d] + lane, wseg);                 // under the xt pack
        __syncthreads();                       // every wave is done reading X: the region becomes XT
        {
            const int hh = lane >> 5;
            float4 bq[4];
#pragma unroll
            for (int q = 0; q < 4; q++) bq[q] = *(const float4 *)(P.b1[d] + 8 * q + 4 * hh);
#pragma unroll
            for (int mt = 0; mt < MT; mt++)
            {
                const int i = wave * 32 * MT + mt * 32 + (lane & 31);
                const int t = t0 - H + i;
                const bool in = !edge || (t >= 0 && t < L);
#pragma unroll
                for (int q = 0; q < 4; q++)
                {
                    half4 h;
                    h[0] = (_Float16)lrelu_max(acc[mt][0][4 * q + 0] + bq[q].x, sl);
                    h[1] = (_Float16)lrelu_max(acc[mt][0][4 * q + 1] + bq[q].y, sl);
                    h[2] = (_Float16)lrelu_max(acc[mt][0][4 * q + 2] + bq[q].z, sl);
                    h[3] = (_Float16)lrelu_max(acc[mt][0][4 * q + 3] + bq[q].w, sl);
                    uint2 pk = *(uint2 *)&h;
                    if (edge)
                    {
                        pk.x = in ? pk.x : 0u;
                        pk.y = in ? pk.y : 0u;
                    }
                    *(uint2 *)(smem + (XM + i) * RS + (8 * q + 4 * hh) * 2) = pk;
                }
            }
        }
        __syncthreads();

        // ---- conv2 (dil 1): output tile row i reads region rows XM + i - h2 + tap;  Y = Y + (conv2 + b2), 0 outside [0, L)
        if (!(ZV_DBGBITS(P.dbg) & 2))
            mfma_taps_deep<CP, MT, 1, false>(acc, abase + (XM - h2) * RS, RS, (const half8 *)P.w2[d] + lane, wseg, K, bw);
        if (d + 1 < nd) deep_preload_b<1>(bw, (const half8 *)P.w1[d + 1] + lane, wseg);      // under the epilogue and the next X write
        {
            const float bias = P.b2[d][col];
            if (edge)
            {
#pragma unroll
                for (int mt = 0; mt < MT; mt++)
#pragma unroll
                    for (int r = 0; r < 16; r++)
                    {
                        const int t = t0 - H + irow0 + mt * 32 + (r & 3) + 8 * (r >> 2);
                        const float v = (acc[mt][0][r] + bias) + yreg[mt][r];
                        yreg[mt][r] = (t >= 0 && t < L) ? v : 0.f;
                    }
            }
            else
            {
#pragma unroll
                for (int mt = 0; mt < MT; mt++)
#pragma unroll
                    for (int r = 0; r < 16; r++) yreg[mt][r] = (acc[mt][0][r] + bias) + yreg[mt][r];
            }
        }
    }

    // ---- store the centre rows (tile rows H .. H + TM - 1, time < L): anything else gets an out-of-range offset
    if (ZV_DBGBITS(P.dbg) & 4) return;
    const __amdgpu_buffer_rsrc_t rs_out = __builtin_amdgcn_make_buffer_rsrc((void *)out_seg, 0, L * CP * 4, 0x00020000);
#pragma unroll
    for (int mt = 0; mt < MT; mt++)
#pragma unroll
        for (int r = 0; r < 16; r++)
        {
            const int i = irow0 + mt * 32 + (r & 3) + 8 * (r >> 2);
            const int t = t0 - H + i;
            const int voff = (i >= H && i < H + TM && t >= 0) ? (t * CP + col) * 4 : -4;
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(yreg[mt][r]), rs_out, voff, 0, ZV_ST_AUX);
        }
}

// ---------------------------------------------------------------------------------------------------
// The whole-block kernel, second form (batches): the conv weights go through LDS.
// In the kernel above every wave streams its own copy of every B fragment from L1/L2 (1 KiB per two MFMAs per wave: the
// CU's vector-memory path is the busiest unit of the launch) through a 32-register ring, which puts the kernel at 150
// registers: ONE 8-wave workgroup per CU, whose waves sit in the same phase between the same barriers, so the matrix
// pipe idles during every pack / epilogue phase and the vector ALUs during every MFMA loop.  Here the 8 ... 24 KiB of a
// conv's fragments are copied global -> LDS once per workgroup (LDS-DMA, one 1-KiB fragment per wave-instruction, no
// registers) while the waves write the operand tile, both MFMA operands are ds_read_b128s two steps ahead, and the
// kernel fits 128 registers: two workgroups per CU, one in its MFMA loop while the other packs.  Same operations in the
// same order per output element as resblock_triple_kernel / resblock_pair_kernel, hence the same bits.
__device__ __forceinline__ void dma_weights32(const void *wsrc, char *wlds, int nblk, int wave, int lane, int nwv)
{
    for (int blk = wave; blk < nblk; blk += nwv)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)((const char *)wsrc + blk * 1024 + lane * 16),
                                         (__attribute__((address_space(3))) void *)(wlds + blk * 1024), 16, 0, 0);
}

// (A variant with Y in the transposed accumulator layout — both convs with the weights as the A operand, 8-byte operand
// writes, 16-byte tile loads / stores: half the vector instructions — measured 7 % SLOWER: a 16-byte access per lane in
// that layout touches 32 rows x 32 bytes per instruction, against 2 rows x 128 bytes for the 4-byte column accesses.)
// LDS stores the compiler does not see as LDS stores: hipcc orders every visible LDS access behind an LDS-DMA in flight with
// s_waitcnt vmcnt(0), which would drain the weight stream at the first operand write of every phase.  The hazards these
// stores do have (against the other waves' reads) are covered by the kernel's own barriers and lgkmcnt waits.
template <int OFF>
__device__ __forceinline__ void lds_st_b64(unsigned addr, uint2 v)
{
    asm volatile("ds_write_b64 %0, %1 offset:%2" : : "v"(addr), "v"(v), "n"(OFF) : "memory");
}
// ---- the whole-block kernel on v_mfma_f32_16x16x32_f16 (round 4; layouts as in resblock_pair_kernel, same bits) ----
// one conv of the 32-channel block: one step per tap (32 channels), operand rows (two 16-row tiles per 32-row block: rows 2c + lt)
// and weight fragments (two 16-channel tiles) from LDS, one tap ahead of the MFMAs that consume them
template <int MT, bool SWAP>
__device__ __forceinline__ void mfma32x_ldsw(floatx4 (&acc)[MT][1][2][2], const char *ap, int dilRS, const char *wl, int K)
{
    constexpr int RS = 32 * 2 + 16;
    half8 a[2][MT][2], b[2][1][2];
#define ZV_LD(slot, aptr, woff)                                                                                       \
    {                                                                                                                 \
        const char *ap_ = (aptr);                                                                                     \
        _Pragma("unroll") for (int mt = 0; mt < MT; mt++)                                                             \
            _Pragma("unroll") for (int lt = 0; lt < 2; lt++) a[slot][mt][lt] = *(const half8 *)(ap_ + (mt * 32 + lt) * RS);    \
        _Pragma("unroll") for (int wt = 0; wt < 2; wt++) b[slot][0][wt] = *(const half8 *)(wl + (woff) + wt * 1024);   \
    }
#define ZV_ST(slot, Z)                                     \
    mfma16_step<MT, 1, SWAP, Z>(acc, a[slot], b[slot]);    \
    __builtin_amdgcn_sched_barrier(0);
    // tap 0 starts the accumulators from the constant 0; the other K - 1 taps (K odd) go two at a time.  The last iteration's
    // look-ahead reads one tap past the end (operand rows and weight-buffer slack that exist) and is never used.
    const char *t1 = ap + dilRS;
    ZV_LD(0, ap, 0)
    ZV_LD(1, t1, 2 * 1024) ZV_ST(0, true)
    for (int it = (K - 1) >> 1; it > 0; it--)
    {
        const char *t2 = t1 + dilRS, *t3 = t2 + dilRS;
        ZV_LD(0, t2, 4 * 1024) ZV_ST(1, false)
        ZV_LD(1, t3, 6 * 1024) ZV_ST(0, false)
        t1 = t3;
        wl += 4 * 1024;
    }
#undef ZV_ST
#undef ZV_LD
}

template <int OFF>
__device__ __forceinline__ void lds_st_b32(unsigned addr, unsigned v)
{
    asm volatile("ds_write_b32 %0, %1 offset:%2" : : "v"(addr), "v"(v), "n"(OFF) : "memory");
}
// the operand writes (two neighbouring channels per lane and row: 4-byte stores) and the xt pack, unrolled at compile time
// (y[mt][wt][lt] holds four rows of one channel: the slope multiply goes two rows at a time, v_pk_mul_f32)
template <int MT_, int I = 0>
__device__ __forceinline__ void xwrite_all16(unsigned xa, const floatx4 (&y)[MT_][2][2], float sl)
{
    constexpr int mt = I / 2, lt = I % 2;
    const floatx4 s0 = y[mt][0][lt] * sl, s1 = y[mt][1][lt] * sl;
#define ZV_XW(i)                                                                                                  \
    {                                                                                                             \
        const float2v r = {lrelu_max_pre(y[mt][0][lt][i], s0[i]), lrelu_max_pre(y[mt][1][lt][i], s1[i])};      \
        const half2v h = __builtin_convertvector(r, half2v);                                                     \
        lds_st_b32<(mt * 32 + 2 * i + lt) * 80>(xa, *(const unsigned *)&h);                                       \
    }
    ZV_XW(0) ZV_XW(1) ZV_XW(2) ZV_XW(3)
#undef ZV_XW
    if constexpr (I + 1 < MT_ * 2) xwrite_all16<MT_, I + 1>(xa, y, sl);
}
template <int MT_, int I = 0>
__device__ __forceinline__ void pack_all16(unsigned pa, const uint2 (&pk)[MT_][2][2])
{
    constexpr int mt = I / 4, lt = (I / 2) % 2, wt = I % 2;
    lds_st_b64<(mt * 32 + lt) * 80 + 32 * wt>(pa, pk[mt][lt][wt]);
    if constexpr (I + 1 < MT_ * 4) pack_all16<MT_, I + 1>(pa, pk);
}

template <int MT, int R>
__global__ __launch_bounds__(64 * (R / 32 / MT), (MT >= 4 ? 2 : 4)) void resblock_block32_kernel(const TripleJobs jobs)
{
    constexpr int CP = 32, NWV = R / 32 / MT, NTH = 64 * NWV;
    constexpr int RS = CP * 2 + 16, NKC = CP / 16;
    // workgroup -> (job, tile): with `il` jobs interleaved the MRF branches of one stretch of the sequence run next to each
    // other on the same XCD (blockIdx.x & 7 picks the XCD), so only the first of them fetches the shared input from HBM.
    const int il = jobs.interleave;
    const int bx = il > 1 ? (int)(((blockIdx.x >> 3) / il) << 3 | (blockIdx.x & 7)) : (int)blockIdx.x;
    const int jb = il > 1 ? (int)((blockIdx.x >> 3) % il) : (int)blockIdx.z;
    const TripleJob &P = jobs.j[jb];
    int H;
    {
        int sumd0 = 0;
        for (int d = 0; d < P.n_dil; d++) sumd0 += P.dil[d];
        H = ((P.K - 1) / 2) * (sumd0 + P.n_dil);
    }
    const int TM = R - 2 * H;
    const int tps = (jobs.segs.max_rows * jobs.rate + TM - 1) / TM;
    const int vt = tile_deal(bx, tps, jobs.segs.nseg, jobs.deal_c);
    if (vt >= tps * jobs.segs.nseg) return;
    const int useg = vt / tps;
    const Seg sg = seg_at(jobs.segs, useg);
    const int L = sg.rows * jobs.rate;
    const int t0 = (vt - useg * tps) * TM;
    if (t0 >= L) return;
    const bool edge = t0 - H < 0 || t0 - H + R > L;
    extern __shared__ __attribute__((aligned(1024))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // 16 x 16 x 32 layouts (see resblock_pair_kernel): lane (c, g); the f32 tile in conv2's accumulator layout
    // y[mt][wt][lt][i] = tile row wave*32*MT + mt*32 + 8g + 2i + lt, channel 2c + wt
    const int lc = lane & 15, lg = lane >> 4;
    const int irow0 = wave * 32 * MT + 8 * lg;
    typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
#ifdef ZV_STAMPS
    const int stamp_wg = blockIdx.x;
    int stamp_k = 1;
#endif
    ZV_STAMP(0)

    const int K = P.K, nd = P.n_dil;
    const int h2 = (K - 1) / 2;
    int dmax = 1;
    for (int d = 0; d < nd; d++) dmax = P.dil[d] > dmax ? P.dil[d] : dmax;
    const float *y_seg = P.y + (size_t)sg.row0 * jobs.rate * CP;
    const int XM = h2 * dmax;
    const int xrows = R + 2 * XM + 5 * dmax;          // + slack: zero-weight taps and the last A prefetch read past the margin
    const int nb = ((K * NKC + 3) >> 2) >> 1;         // 8-step bodies per conv
    const int nblk = 8 * nb;                          // weight fragments per conv (real ones first, zero blocks behind)

    // Two weight buffers where they fit (jobs.db_mask: 3- and 7-tap branches): a conv's fragments are requested while the
    // conv BEFORE it runs and have a whole MFMA loop plus a pack / epilogue phase to land.  With one buffer (11 taps) the
    // request can only follow the barrier that ends the previous conv and the next barrier waits for it: phase stamps of
    // that form show 2 us of DMA latency in each of a block's six pack / epilogue phases (27.6 us per workgroup).
    // The biases of the block's six convs sit in LDS, so nothing in the loop below waits on the vector-memory counter but
    // the barriers that are meant to.
    const bool db = (jobs.db_mask >> jb) & 1;
    char *wlds = smem + round_up(xrows * RS, 1024);
    char *wlds2 = db ? wlds + nblk * 1024 : wlds;                  // conv2's weights
    float *blds = (float *)(wlds + (db ? 2 : 1) * nblk * 1024 + 2048);      // behind the last-prefetch slack: [d][conv][32]
    dma_weights32(P.w1[0], wlds, nblk, wave, lane, NWV);
    if (tid < 64 * nd)
    {
        const int d_ = tid >> 6, c_ = tid & 31;
        blds[tid] = (tid & 32) ? P.b2[d_][c_] : P.b1[d_][c_];
    }
    // the margins of the operand region stay zero for the whole kernel: rows [0, XM) and [XM + R, xrows)
    {
        const int lo = XM * RS / 16, hi0 = (XM + R) * RS / 16, hi = xrows * RS / 16;
        for (int i = tid; i < lo; i += NTH) ((uint4 *)smem)[i] = make_uint4(0, 0, 0, 0);
        for (int i = hi0 + tid; i < hi; i += NTH) ((uint4 *)smem)[i] = make_uint4(0, 0, 0, 0);
    }
    // tile row i <-> time t0 - H + i; rows outside [0, L) are out of the descriptor's range and read as 0
    floatx4 yreg[MT][2][2];          // [mt][wt][lt][i]
    {
        const __amdgpu_buffer_rsrc_t rs_y = __builtin_amdgcn_make_buffer_rsrc((void *)y_seg, 0, L * CP * 4, 0x00020000);
        const int voff = ((t0 - H + irow0) * CP + 2 * lc) * 4;
#pragma unroll
        for (int mt = 0; mt < MT; mt++)
#pragma unroll
            for (int lt = 0; lt < 2; lt++)
#pragma unroll
                for (int i = 0; i < 4; i++)
                {
                    const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(rs_y, voff + (mt * 32 + 2 * i + lt) * CP * 4, 0, 0);
                    yreg[mt][0][lt][i] = __uint_as_float(v[0]);
                    yreg[mt][1][lt][i] = __uint_as_float(v[1]);
                }
    }

    const char *abase = smem + (wave * 32 * MT + 2 * lc) * RS + lg * 16;
    const char *wl = wlds + lane * 16, *wl2 = wlds2 + lane * 16;
    const float sl = P.slope;
    for (int d = 0; d < nd; d++)
    {
        const int dil = P.dil[d], h1 = h2 * dil;
        if (d)
        {
            // the previous conv2 is done reading XT and its weights (raw barrier: conv1's weights may be in flight)
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            if (!db) dma_weights32(P.w1[d], wlds, nblk, wave, lane, NWV);
        }
        // ---- X = f16(lrelu(Y)) into region rows XM .. XM + R - 1
        {
            static_assert(RS == 80, "xwrite_all / pack_all carry the row stride");
            xwrite_all16<MT>((unsigned)(uintptr_t)(smem + (XM + irow0) * RS + 2 * lc * 2), yreg, sl);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        }
        __syncthreads();                       // X complete, conv1's weights landed (the barrier drains the DMA)
        if (db) dma_weights32(P.w2[d], wlds2, nblk, wave, lane, NWV);      // under conv1 and the pack
#ifdef ZV_STAMPS
        if (stamp_k < 11) { ZV_STAMP(stamp_k) stamp_k++; }
#endif

        // ---- conv1 (dilated), transposed product; output tile row i reads region rows XM + i - h1 + tap*dil
        floatx4 acc[MT][1][2][2];
        mfma32x_ldsw<MT, true>(acc, abase + (XM - h1) * RS, dil * RS, wl, K);
#ifdef ZV_STAMPS
        if (stamp_k < 11) { ZV_STAMP(stamp_k) stamp_k++; }
#endif
        // every wave is done reading X and conv1's weights (raw barrier: conv2's weights may be in flight)
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        // (the biases are read before any request goes out: hipcc orders an LDS read behind a pending LDS-DMA with vmcnt(0))
        // (raw ds_reads: hipcc would order a visible LDS read behind the weight DMA in flight with vmcnt(0) and drain it here)
        float4 bq[2];
        float2v bias2;
        {
            // conv1: channels 16 wt + 4g + i; conv2: channels 2c + wt
            const unsigned ba = (unsigned)(uintptr_t)(blds + d * 64 + 4 * lg), bb = (unsigned)(uintptr_t)(blds + d * 64 + 32 + 2 * lc);
            asm volatile("ds_read_b128 %0, %3\n\tds_read_b128 %1, %3 offset:64\n\tds_read_b64 %2, %4\n\ts_waitcnt lgkmcnt(0)"
                         : "=&v"(bq[0]), "=&v"(bq[1]), "=&v"(bias2)
                         : "v"(ba), "v"(bb)
                         : "memory");
        }
        if (!db) dma_weights32(P.w2[d], wlds, nblk, wave, lane, NWV);
        // ---- xt = f16(lrelu(conv1 + b1)), zero outside [0, L): acc[mt][0][wt][lt][i] = tile row mt*32 + 2c + lt, channel 16 wt + 4g + i
        {
            const unsigned pa = (unsigned)(uintptr_t)(smem + (XM + wave * 32 * MT + 2 * lc) * RS + 4 * lg * 2);
            uint2 pkv[MT][2][2];
#pragma unroll
            for (int mt = 0; mt < MT; mt++)
#pragma unroll
                for (int lt = 0; lt < 2; lt++)
                {
#pragma unroll
                    for (int wt = 0; wt < 2; wt++)
                        pkv[mt][lt][wt] = lrelu4_f16(acc[mt][0][wt][lt][0] + bq[wt].x, acc[mt][0][wt][lt][1] + bq[wt].y,
                                                     acc[mt][0][wt][lt][2] + bq[wt].z, acc[mt][0][wt][lt][3] + bq[wt].w, sl);
                }
            if (edge)
            {
                // (a branch the compiler keeps: interior tiles skip the selects)
                asm volatile("; edge tile: rows outside [0, L) are zero");
#pragma unroll
                for (int mt = 0; mt < MT; mt++)
#pragma unroll
                    for (int lt = 0; lt < 2; lt++)
                    {
                        const int t = t0 - H + wave * 32 * MT + mt * 32 + 2 * lc + lt;
                        const bool in = t >= 0 && t < L;
#pragma unroll
                        for (int wt = 0; wt < 2; wt++)
                        {
                            pkv[mt][lt][wt].x = in ? pkv[mt][lt][wt].x : 0u;
                            pkv[mt][lt][wt].y = in ? pkv[mt][lt][wt].y : 0u;
                        }
                    }
            }
            pack_all16<MT>(pa, pkv);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        }
        __syncthreads();                       // XT complete, conv2's weights landed
        if (db && d + 1 < nd) dma_weights32(P.w1[d + 1], wlds, nblk, wave, lane, NWV);      // under conv2, the update and the next X write
#ifdef ZV_STAMPS
        if (stamp_k < 11) { ZV_STAMP(stamp_k) stamp_k++; }
#endif

        // ---- conv2 (dil 1): output tile row i reads region rows XM + i - h2 + tap;  Y = Y + (conv2 + b2), 0 outside [0, L)
        mfma32x_ldsw<MT, false>(acc, abase + (XM - h2) * RS, RS, wl2, K);
        {
            // (four rows of a channel per accumulator: packed adds, v_pk_add_f32, two rows at a time)
#pragma unroll
            for (int mt = 0; mt < MT; mt++)
#pragma unroll
                for (int wt = 0; wt < 2; wt++)
#pragma unroll
                    for (int lt = 0; lt < 2; lt++) yreg[mt][wt][lt] = (acc[mt][0][wt][lt] + bias2[wt]) + yreg[mt][wt][lt];
            if (edge)
            {
                asm volatile("; edge tile: rows outside [0, L) are zero");
#pragma unroll
                for (int mt = 0; mt < MT; mt++)
#pragma unroll
                    for (int lt = 0; lt < 2; lt++)
#pragma unroll
                        for (int i = 0; i < 4; i++)
                        {
                            const int t = t0 - H + irow0 + mt * 32 + 2 * i + lt;
                            const bool in = t >= 0 && t < L;
                            yreg[mt][0][lt][i] = in ? yreg[mt][0][lt][i] : 0.f;
                            yreg[mt][1][lt][i] = in ? yreg[mt][1][lt][i] : 0.f;
                        }
            }
        }
    }

    // ---- store the centre rows (tile rows H .. H + TM - 1, time < L): anything else gets an out-of-range offset
    float *const out_seg = P.out + (size_t)sg.row0 * jobs.rate * CP;
    const __amdgpu_buffer_rsrc_t rs_out = __builtin_amdgcn_make_buffer_rsrc((void *)out_seg, 0, L * CP * 4, 0x00020000);
#pragma unroll
    for (int mt = 0; mt < MT; mt++)
#pragma unroll
        for (int lt = 0; lt < 2; lt++)
#pragma unroll
            for (int i = 0; i < 4; i++)
            {
                // (row >= H gives t = t0 + row - H >= 0; t < L is the descriptor's range)
                const int ro = irow0 - H + mt * 32 + 2 * i + lt;
                const int voff = (unsigned)ro < (unsigned)TM ? ((t0 + ro) * CP + 2 * lc) * 4 : -8;
                const u32x2 o = {__float_as_uint(yreg[mt][0][lt][i]), __float_as_uint(yreg[mt][1][lt][i])};
                __builtin_amdgcn_raw_buffer_store_b64(o, rs_out, voff, 0, ZV_ST_AUX);
            }
#ifdef ZV_STAMPS
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    ZV_STAMP(11)
#endif
}

// validate, plan (conv_plan.h triple_plan: the tile height, the form with the weights in LDS, its weight buffers), fill, dispatch
hipError_t launch_triple(hipStream_t s, const TripleJob *jobs, int njobs, int n_cu, const Segs &segs, int rate)
{
    if (njobs < 1 || njobs > PAIR_MAX_JOBS || segs.nseg < 1 || segs.max_rows < 1) return hipErrorInvalidValue;
    const int dbg = diag_bits();
    TripleJobs js;
    BlockDesc desc[PAIR_MAX_JOBS];
    for (int i = 0; i < njobs; i++)
    {
        js.j[i] = jobs[i];
        js.j[i].dbg = dbg;
        desc[i] = block_desc(jobs[i]);
    }
    for (int i = njobs; i < PAIR_MAX_JOBS; i++) js.j[i] = js.j[0];
    const TriplePlan p = triple_plan(desc, ConvCall{njobs, segs.nseg, segs.max_rows, rate, n_cu, 0});
    if (!p.valid) return hipErrorInvalidValue;
    js.segs = segs;
    js.rate = rate;
    js.deal_c = p.deal_c;
    js.interleave = p.interleave;
    js.db_mask = p.db_mask;
#ifdef ZV_STAMPS
    js.stamp = knob(ZV_STAMP_CP) == 32 ? stamp_buffer() : nullptr;
#endif
    const dim3 grid(p.gx, 1, p.gz);
    if (p.lds_form)
    {
        // (the whole-block kernel of batches reads the 16 x 16 x 32 fragment order: TripleJob::w1x / w2x)
        for (int i = 0; i < njobs; i++)
            for (int d = 0; d < jobs[i].n_dil; d++)
                if (!jobs[i].w1x[d] || !jobs[i].w2x[d]) return hipErrorInvalidValue;
        for (int i = 0; i < PAIR_MAX_JOBS; i++)
            for (int d = 0; d < TRIPLE_MAX_DIL; d++)
            {
                js.j[i].w1[d] = js.j[i].w1x[d];
                js.j[i].w2[d] = js.j[i].w2x[d];
            }
        return p.R == 512 ? launch_lds(resblock_block32_kernel<2, 512>, grid, dim3(p.threads), p.lds_bytes, s, js)
                          : launch_lds(resblock_block32_kernel<2, 256>, grid, dim3(p.threads), p.lds_bytes, s, js);
    }
#define ZV_TCASE(mt, r) \
    if (p.MT == mt && p.R == r) { hipLaunchKernelGGL((resblock_triple_kernel<32, mt, r>), grid, dim3(p.threads), p.lds_bytes, s, js); return hipGetLastError(); }
    ZV_TCASE(2, 256) ZV_TCASE(2, 512)
#undef ZV_TCASE
    return hipErrorInvalidValue;
}

}  // namespace zv
