// mfma_common.h — what more than one of the conv sources (conv.hip, conv_gemm.hip, conv1d_mfma.hip) uses, and nothing more.
// Device code, plus the one host helper every launcher of the three uses (launch_lds).
//
// conv1d_mfma.hip (the ResBlock family) includes this header but bench.py / scripts/traffic.py hash only that file, so an
// edit here can change the ResBlock kernels without marking their traffic profile stale.  Keep it minimal: a helper used by
// one family lives in that family's file.
#pragma once

#include "kernels.h"

#include <hip/hip_runtime.h>

namespace zv
{

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef float float2v __attribute__((ext_vector_type(2)));

__device__ __forceinline__ float lrelu(float x, float s) { return x > 0.f ? x : x * s; }

// ZERO: the first step of a contraction — the accumulator operand is the constant 0 (an inline constant of the
// instruction: no 16 x MT x NT register moves to clear the accumulators first)
template <int MT, int NT, bool SWAP, bool ZERO = false>
__device__ __forceinline__ void mfma_step(floatx16 (&acc)[MT][NT], const half8 (&a)[MT], const half8 (&b)[NT])
{
    const floatx16 z = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int mt = 0; mt < MT; mt++)
#pragma unroll
        for (int nt = 0; nt < NT; nt++)
        {
            if constexpr (SWAP)      // weights as the A operand -> D[oc][time]
                acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(b[nt], a[mt], ZERO ? z : acc[mt][nt], 0, 0, 0);
            else
                acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[mt], b[nt], ZERO ? z : acc[mt][nt], 0, 0, 0);
        }
}

// f64 partial sums of a wave's 32 x 32 output tile per channel (= lane & 31): the lane's 16 rows in register order, then
// the two half-waves (rows 4*(lane>>5) + ...); rows at or past L do not count.  See launch_stats_finalize.
__device__ __forceinline__ void tile_stats_store(const float (&v)[16], int t_first, int L, double *dst)
{
    double s1 = 0.0, s2 = 0.0;
#pragma unroll
    for (int r = 0; r < 16; r++)
    {
        const int t = t_first + (r & 3) + 8 * (r >> 2);
        const double x = (t < L) ? (double)v[r] : 0.0;
        s1 += x;
        s2 += x * x;
    }
    s1 += __shfl_xor(s1, 32, 64);
    s2 += __shfl_xor(s2, 32, 64);
    if ((threadIdx.x & 63) < 32) *(double2 *)dst = make_double2(s1, s2);
}

// ---- diagnostic build only (-DZV_STAMPS, never the shipped library): wave 0 of a workgroup of a stamped launch stamps the
// clock at its phase boundaries into the launch's `stamp` buffer (cdna_hip_programming.md §7, in-kernel stamps).  The one
// buffer lives in conv1d_mfma.hip; launchers hand it out with stamp_buffer(), zv_debug_read_stamps reads it back.
#ifdef ZV_STAMPS
constexpr int ZV_STAMP_WGS = 1 << 17, ZV_STAMP_N = 12;
#ifdef ZV_STAMPS_LOADER
#define ZV_STAMP_TID 256
#else
#define ZV_STAMP_TID 0
#endif
#define ZV_STAMP(k)                                                                                   \
    if (jobs.stamp && threadIdx.x == ZV_STAMP_TID && stamp_wg < ZV_STAMP_WGS)                         \
    {                                                                                                 \
        jobs.stamp[(size_t)stamp_wg * ZV_STAMP_N + (k)] = __builtin_amdgcn_s_memrealtime();           \
    }
unsigned long long *stamp_buffer();
#else
#define ZV_STAMP(k)
#endif

// The launch sequence of a kernel with `lds` bytes of dynamic LDS: above the default 64 KiB the kernel's limit is raised first
// (per launch: the attribute is stored per device).
template <typename Kernel, typename Args>
static hipError_t launch_lds(Kernel kern, dim3 grid, dim3 block, size_t lds, hipStream_t s, const Args &args)
{
    if (lds > 64 * 1024)
    {
        hipError_t e = hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kern, grid, block, lds, s, args);
    return hipGetLastError();
}

}  // namespace zv
