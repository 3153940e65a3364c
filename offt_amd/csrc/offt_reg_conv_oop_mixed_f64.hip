// offt_reg_conv_oop_mixed_f64.hip -- double-precision out-of-place fused convolution kernels of mixed-radix lengths
// (fft_conv_oop_panelx_k, fft_conv_oop_half_panelx_k; picked only with both bits of offt_filter_desc::mixed): the shapes
// of offt_reg_conv_mixed_f64.hip, one per length for the full-line and the half-line form alike, so that an out-of-place
// launch does the arithmetic of the in-place one.  No cache-keeping twins, as there.  No instance uses scratch memory.
#include "offt_panel.hpp"

namespace offtk {

void reg_conv_oop_mixed_f64() {
  reg_variantx_conv_oop<double, 96, 8, 4, 6, 4, 16, true>();
  reg_variantx_conv_oop<double, 192, 16, 12, 4, 4, 16, true>();
  reg_variantx_conv_oop<double, 320, 40, 8, 10, 4, 8, true>();
  reg_variantx_conv_oop<double, 384, 32, 12, 4, 8, 8, true>();
  reg_variantx_conv_oop<double, 640, 80, 10, 8, 8, 4, true>();
  reg_variantx_conv_oop<double, 768, 64, 12, 8, 8, 4, true>();
  reg_variantx_conv_oop<double, 1000, 100, 10, 10, 10, 4, true>();
}

}  // namespace offtk
