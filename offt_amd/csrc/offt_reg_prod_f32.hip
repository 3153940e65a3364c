// offt_reg_prod_f32.hip -- single-precision pseudo-spectral product kernels (fft_prod_panel_k): every power of two from 64
// to 1024 points.  The stage shapes are those of offt_reg_conv_sum_f32.hip with sixteen columns -- the lines are strided, and
// sixteen single-precision columns are one 128-B segment of a scratch line -- except at 1024 points, where sixteen columns
// are 512 threads at two waves per SIMD and spill (116 B per lane): eight columns, one wave per SIMD, 64-B segments
#include "offt_panel.hpp"

namespace offtk {

void reg_prod_f32() {
  reg_variant_prod<float, 64, 8, 8, 8, 1, 16, false>();
  reg_variant_prod<float, 128, 16, 16, 8, 1, 16, false>();
  reg_variant_prod<float, 256, 16, 16, 16, 1, 16, false>();
  reg_variant_prod<float, 512, 32, 32, 16, 1, 16, false>();
  reg_variant_prod<float, 1024, 32, 32, 32, 1, 8, false>();
}

}  // namespace offtk
