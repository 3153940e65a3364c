// offt_reg_half_real_f32.hip -- single-precision real ends of a half-box chain (fft_half_r2c_panel_k, fft_half_c2r_panel_k;
// offt_pass_desc::real_input together with ::half): the one-column shapes offt_reg_half_f32.hip has for its contiguous /
// strided flavours, 64 to 1024 points.  No column pairs: they take complex input only
#include "offt_panel.hpp"

namespace offtk {

void reg_half_real_f32() {
  reg_variant_half_real<float, 64, 8, 8, 8, 1, 16, false>();
  reg_variant_half_real<float, 128, 16, 16, 8, 1, 16, false>();
  reg_variant_half_real<float, 256, 16, 16, 16, 1, 16, false>();
  reg_variant_half_real<float, 512, 32, 32, 16, 1, 16, false>();
  reg_variant_half_real<float, 1024, 32, 32, 32, 1, 16, true>();
}

}  // namespace offtk
