// 128-pixel tile, f16 (IEEE half, inference plans): forward epilogues only
#include "conv_igemm_kernel.h"

int dyk_conv_launch_n128h(const DykConvDesc* d, hipStream_t s) {
    if (d->dtype != DYK_F16) return DYK_ERR_UNSUPPORTED;
    return dispatch_conv_bn<f16_t, 128>(d, s);
}
