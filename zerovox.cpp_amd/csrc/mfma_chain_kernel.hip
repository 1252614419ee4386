// mfma_chain_kernel.hip — a test-only kernel: one MFMA accumulation chain per form, for tests/test_gpu_mfma_chain.py.
// A part of misc_kernels.hip's unit.
#include "kernels.h"
#include "wave_sum.h"

namespace zv
{

// ---------------------------------------------------------------------------------------------------
// Tests (zv_debug_mfma_chain): C[32][32] = C0 + A[32][K] * B[K][32] by one wave as one k-ordered chain per element, on each
// matrix-core instruction the product's kernels accumulate with (lane layouts of scripts/mfma_shape_bits.hip and of
// linear_mfma_kernel, encoder_kernels.hip).  What the same-bits contract of conv1d_mfma.hip rests on, measurable on any operands.
typedef _Float16 half8c __attribute__((ext_vector_type(8)));
typedef float floatx4c __attribute__((ext_vector_type(4)));

// FORM 0: v_mfma_f32_32x32x16_f16, 16 products per instruction (lane half h holds k0 + 8 h .. + 7)
// FORM 1: v_mfma_f32_16x16x32_f16, four 16x16 tiles, 32 products per instruction (lane group g holds k0 + 8 g .. + 7)
// FORM 2: v_mfma_f32_32x32x2_f32, 2 products per instruction (lane half h holds k0 + h)
template <int FORM>
__global__ __launch_bounds__(64) void mfma_chain_kernel(const void *__restrict__ Av, const void *__restrict__ Bv,
                                                        const float *__restrict__ C0, int K, float *__restrict__ C)
{
    const int lane = threadIdx.x;
    if constexpr (FORM == 1)
    {
        const _Float16 *A = (const _Float16 *)Av, *B = (const _Float16 *)Bv;
        const int r = lane & 15, g = lane >> 4;
        for (int tm = 0; tm < 2; tm++)
            for (int tn = 0; tn < 2; tn++)
            {
                floatx4c acc;
                for (int i = 0; i < 4; i++) acc[i] = C0[(tm * 16 + 4 * g + i) * 32 + tn * 16 + r];
                for (int k0 = 0; k0 < K; k0 += 32)
                {
                    half8c a, b;
                    for (int j = 0; j < 8; j++)
                    {
                        a[j] = A[(size_t)(tm * 16 + r) * K + k0 + 8 * g + j];
                        b[j] = B[(size_t)(k0 + 8 * g + j) * 32 + tn * 16 + r];
                    }
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, acc, 0, 0, 0);
                }
                for (int i = 0; i < 4; i++) C[(tm * 16 + 4 * g + i) * 32 + tn * 16 + r] = acc[i];
            }
    }
    else
    {
        const int r = lane & 31, h = lane >> 5;
        floatx16m acc;
        for (int i = 0; i < 16; i++) acc[i] = C0[((i & 3) + 8 * (i >> 2) + 4 * h) * 32 + r];
        if constexpr (FORM == 0)
        {
            const _Float16 *A = (const _Float16 *)Av, *B = (const _Float16 *)Bv;
            for (int k0 = 0; k0 < K; k0 += 16)
            {
                half8c a, b;
                for (int j = 0; j < 8; j++)
                {
                    a[j] = A[(size_t)r * K + k0 + 8 * h + j];
                    b[j] = B[(size_t)(k0 + 8 * h + j) * 32 + r];
                }
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, acc, 0, 0, 0);
            }
        }
        else
        {
            const float *A = (const float *)Av, *B = (const float *)Bv;
            for (int k0 = 0; k0 < K; k0 += 2)
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(A[(size_t)r * K + k0 + h], B[(size_t)(k0 + h) * 32 + r], acc, 0, 0, 0);
        }
        for (int i = 0; i < 16; i++) C[((i & 3) + 8 * (i >> 2) + 4 * h) * 32 + r] = acc[i];
    }
}

hipError_t launch_mfma_chain(hipStream_t s, int form, const void *a, const void *b, const float *c0, int K, float *out)
{
    if (form < 0 || form > 2 || !a || !b || !c0 || !out || K < 32 || (K & 31)) return hipErrorInvalidValue;
    if (form == 0)
        hipLaunchKernelGGL(mfma_chain_kernel<0>, dim3(1), dim3(64), 0, s, a, b, c0, K, out);
    else if (form == 1)
        hipLaunchKernelGGL(mfma_chain_kernel<1>, dim3(1), dim3(64), 0, s, a, b, c0, K, out);
    else
        hipLaunchKernelGGL(mfma_chain_kernel<2>, dim3(1), dim3(64), 0, s, a, b, c0, K, out);
    return hipGetLastError();
}

}  // namespace zv
