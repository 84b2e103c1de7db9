// K-grouped instantiations of the implicit-GEMM convolution (conv_igemm_kg.hip), f16 (IEEE half, inference plans):
// forward epilogues only
#include "conv_igemm_kernel.h"

int dyk_conv_launch_kgh(const DykConvDesc* d, hipStream_t s) {
    if (d->dtype != DYK_F16) return DYK_ERR_UNSUPPORTED;
    return dispatch_conv_kg<f16_t>(d, s);
}
