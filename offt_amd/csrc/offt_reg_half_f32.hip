// offt_reg_half_f32.hip -- single-precision half-line kernels (fft_half_panel_k, fft_conv_half_panel_k; offt_pass_desc::half):
// the one-column default shapes of 64 ... 1024 points in the four forms the z-y-x half-box schedule and its mirror launch,
// and the column-pair shapes (T = f32x2) of the two lengths that have pair kernels at all, 512 and 1024
#include "offt_panel.hpp"

namespace offtk {

void reg_half_f32() {
  reg_variant_half<float, 64, 8, 8, 8, 1, 16, false>();
  reg_variant_half<float, 128, 16, 16, 8, 1, 16, false>();
  reg_variant_half<float, 256, 16, 16, 16, 1, 16, false>();
  reg_variant_half<float, 512, 32, 32, 16, 1, 16, false, H_CS1 | H_SC2>();
  reg_variant_half<float, 512, 32, 32, 16, 1, 8, false, H_CC1 | H_CC2>();
  reg_variant_half<float, 1024, 32, 32, 32, 1, 16, true, H_CS1 | H_SC2>();
  reg_variant_half<float, 1024, 32, 32, 32, 1, 8, false, H_CC1 | H_CC2>();
  reg_variant_half<f32x2, 512, 16, 16, 16, 2, 8, true>();
  reg_variant_half<f32x2, 1024, 16, 16, 16, 4, 8, true>();
  reg_variant_conv_half<float, 64, 8, 8, 8, 1, 16, false>();
  reg_variant_conv_half<float, 128, 16, 16, 8, 1, 16, false>();
  reg_variant_conv_half<float, 256, 16, 16, 16, 1, 16, false>();
  reg_variant_conv_half<float, 512, 32, 32, 16, 1, 8, false>();
  reg_variant_conv_half<float, 1024, 32, 32, 32, 1, 8, false>();
}

}  // namespace offtk
