// wave_sum.h — what the parts of misc_kernels.hip's unit share on the device: a wave's sum by butterfly (every lane gets it) and the
// 32 x 32 MFMA accumulator type.
#pragma once

#include <hip/hip_runtime.h>

namespace zv
{

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_sum_f(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

typedef float floatx16m __attribute__((ext_vector_type(16)));

}  // namespace zv
