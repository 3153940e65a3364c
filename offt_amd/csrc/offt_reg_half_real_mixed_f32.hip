// offt_reg_half_real_mixed_f32.hip -- single-precision real ends of a half-box chain at the mixed-radix lengths
// (fft_half_r2c_panelx_k, fft_half_c2r_panelx_k; offt_pass_desc::real_input together with ::half and its bit 4): the shapes
// of offt_reg_half_mixed_f32.hip, one column per lane.
#include "offt_panel.hpp"

namespace offtk {

void reg_half_real_mixed_f32() {
  reg_variantx_half_real<float, 384, 16, 8, 8, 6, 16, true>();
  reg_variantx_half_real<float, 640, 40, 16, 5, 8, 16, true>();
  reg_variantx_half_real<float, 768, 32, 8, 8, 12, 16, true>();
  reg_variantx_half_real<float, 1000, 40, 20, 5, 10, 16, true>();
}

}  // namespace offtk
