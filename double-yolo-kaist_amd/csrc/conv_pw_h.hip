// Instantiations of the persistent pointwise convolution (conv_pw_kernel.h), f16 (IEEE half, inference plans): plain store
#include "conv_pw_kernel.h"

int dyk_conv_launch_pwh(const DykConvDesc* d, hipStream_t s) {
    if (d->dtype != DYK_F16) return DYK_ERR_UNSUPPORTED;
    return dispatch_conv_pw<0, 0, f16_t>(d, s);
}
