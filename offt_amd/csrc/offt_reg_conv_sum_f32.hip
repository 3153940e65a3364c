// offt_reg_conv_sum_f32.hip -- single-precision multi-input fused convolution kernels (fft_conv_sum_panel_k,
// fft_conv_sum_half_panel_k): the shapes of offt_reg_conv_f32.hip, every power of two from 64 to 1024 points
#include "offt_panel.hpp"

namespace offtk {

void reg_conv_sum_f32() {
  reg_variant_conv_sum<float, 64, 8, 8, 8, 1, 16, false>();
  reg_variant_conv_sum<float, 128, 16, 16, 8, 1, 16, false>();
  reg_variant_conv_sum<float, 256, 16, 16, 16, 1, 16, false>();
  reg_variant_conv_sum<float, 512, 32, 32, 16, 1, 8, false>();
  reg_variant_conv_sum<float, 1024, 32, 32, 32, 1, 8, false>();
}

}  // namespace offtk
