// offt_reg_conv_oop_mixed_f32.hip -- single-precision out-of-place fused convolution kernels of mixed-radix lengths
// (fft_conv_oop_panelx_k, fft_conv_oop_half_panelx_k; picked only with both bits of offt_filter_desc::mixed): the shapes
// of offt_reg_conv_mixed_f32.hip, one per length for the full-line and the half-line form alike, so that an out-of-place
// launch does the arithmetic of the in-place one.  No cache-keeping twins, as there.  No instance uses scratch memory.
#include "offt_panel.hpp"

namespace offtk {

void reg_conv_oop_mixed_f32() {
  reg_variantx_conv_oop<float, 384, 16, 8, 8, 6, 16, true>();
  reg_variantx_conv_oop<float, 640, 40, 16, 5, 8, 8, true>();
  reg_variantx_conv_oop<float, 768, 32, 8, 8, 12, 16, true>();
  reg_variantx_conv_oop<float, 1000, 50, 20, 5, 10, 8, true>();
}

}  // namespace offtk
