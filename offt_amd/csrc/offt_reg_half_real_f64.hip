// offt_reg_half_real_f64.hip -- double-precision real ends of a half-box chain (fft_half_r2c_panel_k, fft_half_c2r_panel_k;
// offt_pass_desc::real_input together with ::half): the shapes of offt_reg_half_f64.hip, 64 to 1024 points
#include "offt_panel.hpp"

namespace offtk {

void reg_half_real_f64() {
  reg_variant_half_real<double, 64, 8, 8, 8, 1, 8, false>();
  reg_variant_half_real<double, 128, 16, 16, 8, 1, 8, false>();
  reg_variant_half_real<double, 256, 16, 16, 16, 1, 8, false>();
  reg_variant_half_real<double, 512, 16, 16, 16, 2, 8, true>();
  reg_variant_half_real<double, 1024, 16, 16, 16, 4, 8, true>();
}

}  // namespace offtk
