// K-grouped instantiations of the implicit-GEMM convolution (two 4-wave groups per workgroup walk the two halves of the
// input channels; conv_igemm_kernel.h, dispatch_conv_kg): bf16, 128-byte K step, 2-stage rings, 80 / 160 pixel
// tiles.  For the deep layers whose ~256 tiles leave one 4-wave workgroup per CU.  Both epilogue families (8 kernels).
#include "conv_igemm_kernel.h"

int dyk_conv_launch_kg(const DykConvDesc* d, hipStream_t s) {
    if ((d->dtype != DYK_BF16 && d->dtype != DYK_F16) || (d->Cin * 2) % 128 || d->Cin / 64 < 2 * conv_splitk_of(d)) return DYK_ERR_UNSUPPORTED;
    if (d->dtype == DYK_F16) return dyk_conv_launch_kgh(d, s);
    return (d->flags & DYK_EPI_BNBWD) ? dispatch_conv_kg<bf16_t, 1>(d, s) : dispatch_conv_kg<bf16_t, 0>(d, s);
}
