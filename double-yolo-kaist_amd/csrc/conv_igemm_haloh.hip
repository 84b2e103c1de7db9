// 3x3 halo-tile convolution, f16 (IEEE half, inference plans): forward epilogues only
#include "conv_igemm_kernel.h"

int dyk_conv_launch_haloh(const DykConvDesc* d, hipStream_t s, int th) {
    if (d->dtype != DYK_F16) return DYK_ERR_UNSUPPORTED;
    if (th == 4) return dispatch_conv_halo<f16_t, 4>(d, s);
    if (th == 8) return dispatch_conv_halo<f16_t, 8>(d, s);
    return DYK_ERR_UNSUPPORTED;
}
