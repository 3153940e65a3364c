// offt_reg_half_f64.hip -- double-precision half-line kernels (fft_half_panel_k, fft_conv_half_panel_k; offt_pass_desc::half):
// the default shape of every power of two from 64 to 1024 points, in the four forms the z-y-x half-box schedule and its
// mirror launch
#include "offt_panel.hpp"

namespace offtk {

void reg_half_f64() {
  reg_variant_half<double, 64, 8, 8, 8, 1, 8, false>();
  reg_variant_half<double, 128, 16, 16, 8, 1, 8, false>();
  reg_variant_half<double, 256, 16, 16, 16, 1, 8, false>();
  reg_variant_half<double, 512, 16, 16, 16, 2, 8, true>();
  reg_variant_half<double, 1024, 16, 16, 16, 4, 8, true>();
  reg_variant_conv_half<double, 64, 8, 8, 8, 1, 8, false>();
  reg_variant_conv_half<double, 128, 16, 16, 8, 1, 8, false>();
  reg_variant_conv_half<double, 256, 16, 16, 16, 1, 8, false>();
  reg_variant_conv_half<double, 512, 16, 16, 16, 2, 8, true>();
  reg_variant_conv_half<double, 1024, 16, 16, 16, 4, 8, true>();
}

}  // namespace offtk
