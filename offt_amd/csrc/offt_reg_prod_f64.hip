// offt_reg_prod_f64.hip -- double-precision pseudo-spectral product kernels (fft_prod_panel_k): every power of two from 64
// to 1024 points.  The stage shapes are those of offt_reg_conv_sum_f64.hip -- the accumulator doubles the data registers
// here as there -- with eight columns throughout: the lines are strided, and eight double-precision columns are one 128-B
// segment of a scratch line
#include "offt_panel.hpp"

namespace offtk {

void reg_prod_f64() {
  reg_variant_prod<double, 64, 8, 8, 8, 1, 8, false>();
  reg_variant_prod<double, 128, 16, 16, 8, 1, 8, false>();
  reg_variant_prod<double, 256, 16, 16, 16, 1, 8, false>();
  reg_variant_prod<double, 512, 16, 16, 16, 2, 8, true>();
  reg_variant_prod<double, 1024, 16, 16, 16, 4, 8, true>();
}

}  // namespace offtk
