// conv_kernels.hip — the three conv sources compiled as ONE translation unit: the generic conv (conv.hip), the ResBlock family
// (conv1d_mfma.hip) and the wide-conv GEMM (conv_gemm.hip).
//
// They are separate files so that each kernel family, and what it depends on, can be read (and hashed) on its own; they
// compile together because hipcc's interprocedural passes optimise a helper by the callers it sees in the unit.  Compiled
// apart, four generic-conv kernels come out with other code: mfma_step<2, 1> loses its caller in resblock_triple_kernel's loop
// and gets its array arguments promoted to values (conv1d_mfma_kernel<2, *, 1> then issues its weight-fragment loads in another
// order), and round_up's one remaining alignment is folded into its body (out_conv_tanh_kernel allocates other registers).
// One unit keeps every kernel's device code independent of how the sources are split.
#include "conv.hip"
#include "conv1d_mfma.hip"
#include "conv_gemm.hip"
