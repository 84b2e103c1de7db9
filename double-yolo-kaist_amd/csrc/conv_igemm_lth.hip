// Instantiations of the large-tile 3x3 convolution (conv_lt_kernel.h), f16 (IEEE half, inference plans): forward epilogues
#include "conv_lt_kernel.h"

int dyk_conv_launch_lth(const DykConvDesc* d, hipStream_t s) {
    if (d->dtype != DYK_F16) return DYK_ERR_UNSUPPORTED;
    return dispatch_conv_lt<0, f16_t>(d, s);
}
