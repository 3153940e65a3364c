// offt_reg_half_real_mixed_f64.hip -- double-precision real ends of a half-box chain at the mixed-radix lengths
// (fft_half_r2c_panelx_k, fft_half_c2r_panelx_k; offt_pass_desc::real_input together with ::half and its bit 4): for every
// length of offt_reg_half_mixed_f64.hip the shape (radix order, threads per line, columns) that file has for its contiguous /
// strided flavours, one column per lane.
#include "offt_panel.hpp"

namespace offtk {

void reg_half_real_mixed_f64() {
  reg_variantx_half_real<double, 96, 8, 4, 6, 4, 16, true>();
  reg_variantx_half_real<double, 192, 8, 8, 3, 8, 16, true>();
  reg_variantx_half_real<double, 320, 16, 8, 10, 4, 8, true>();
  reg_variantx_half_real<double, 384, 16, 12, 4, 8, 16, true>();
  reg_variantx_half_real<double, 640, 80, 10, 8, 8, 8, true>();
  reg_variantx_half_real<double, 768, 32, 12, 8, 8, 8, true>();
  reg_variantx_half_real<double, 1000, 100, 10, 10, 10, 8, true>();
}

}  // namespace offtk
