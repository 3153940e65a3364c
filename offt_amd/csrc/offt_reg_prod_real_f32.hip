// offt_reg_prod_real_f32.hip -- single-precision pseudo-spectral product kernels for real fields held as half spectra
// (fft_prod_real_panel_k): every power of two from 64 to 1024 real points.  The stage shapes are those of
// offt_reg_prod_f32.hip with sixteen columns (one 128-B segment of a scratch line) -- at 1024 points too: without the
// accumulator array the sixteen-column shape (512 threads, two waves per SIMD) has no scratch, where the complex product
// spills and falls back to eight columns.  DESIGN.md 4.5 has the register table and the shapes tried and rejected
#include "offt_panel.hpp"

namespace offtk {

void reg_prod_real_f32() {
  reg_variant_prod_real<float, 64, 8, 8, 8, 1, 16, false>();
  reg_variant_prod_real<float, 128, 16, 16, 8, 1, 16, false>();
  reg_variant_prod_real<float, 256, 16, 16, 16, 1, 16, false>();
  reg_variant_prod_real<float, 512, 32, 32, 16, 1, 16, false>();
  reg_variant_prod_real<float, 1024, 32, 32, 32, 1, 16, false>();
}

}  // namespace offtk
