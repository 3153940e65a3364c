// offt_reg_conv_oop_f64.hip -- double-precision out-of-place fused convolution kernels (fft_conv_oop_panel_k,
// fft_conv_oop_half_panel_k): the shapes of offt_reg_conv_f64.hip, every power of two from 64 to 1024 points
#include "offt_panel.hpp"

namespace offtk {

void reg_conv_oop_f64() {
  reg_variant_conv_oop<double, 64, 8, 8, 8, 1, 8, false>();
  reg_variant_conv_oop<double, 128, 16, 16, 8, 1, 8, false>();
  reg_variant_conv_oop<double, 256, 16, 16, 16, 1, 8, false>();
  reg_variant_conv_oop<double, 512, 16, 16, 16, 2, 8, true>();
  reg_variant_conv_oop<double, 1024, 16, 16, 16, 4, 8, true>();
}

}  // namespace offtk
