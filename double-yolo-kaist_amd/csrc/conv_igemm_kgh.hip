// K-grouped instantiations of the implicit-GEMM convolution (conv_igemm_kg.hip), f16 (IEEE half, inference plans):
// forward epilogues only
#include "conv_igemm_kernel.h"

int dyk_conv_launch_kgh(const DykConvDesc* d, hipStream_t s) {
    if (d->dtype != DYK_F16) return DYK_ERR_UNSUPPORTED;
    const int tile = (d->tune >> 12) & 0xf;
    int bm = d->Cout > 64 ? 128 : 64;
    const int bm_code = (d->tune >> 24) & 0xf;
    if (bm_code == 2) bm = 64;
    if (bm_code == 3) bm = 128;
    if (tile == 1) return bm == 128 ? launch_conv_impl<f16_t, 128, 80, 128, 2, 2, 0>(d, s) : launch_conv_impl<f16_t, 64, 80, 128, 2, 2, 0>(d, s);
    if (tile == 2) return bm == 128 ? launch_conv_impl<f16_t, 128, 160, 128, 2, 2, 0>(d, s) : launch_conv_impl<f16_t, 64, 160, 128, 2, 2, 0>(d, s);
    return DYK_ERR_UNSUPPORTED;
}
