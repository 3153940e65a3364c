// offt_reg_prod_real_f64.hip -- double-precision pseudo-spectral product kernels for real fields held as half spectra
// (fft_prod_real_panel_k): every power of two from 64 to 1024 real points.  The stage shapes and the eight columns (one 128-B
// segment of a scratch line) are those of offt_reg_prod_f64.hip; there is one data array instead of two, so the waves per
// SIMD are bounded like the fused convolution's (DESIGN.md 4.5 has the register table)
#include "offt_panel.hpp"

namespace offtk {

void reg_prod_real_f64() {
  reg_variant_prod_real<double, 64, 8, 8, 8, 1, 8, false>();
  reg_variant_prod_real<double, 128, 16, 16, 8, 1, 8, false>();
  reg_variant_prod_real<double, 256, 16, 16, 16, 1, 8, false>();
  reg_variant_prod_real<double, 512, 16, 16, 16, 2, 8, true>();
  reg_variant_prod_real<double, 1024, 16, 16, 16, 4, 8, true>();
}

}  // namespace offtk
