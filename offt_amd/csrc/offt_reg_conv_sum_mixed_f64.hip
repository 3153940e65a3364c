// offt_reg_conv_sum_mixed_f64.hip -- double-precision multi-input fused convolution kernels of mixed-radix lengths
// (fft_conv_sum_panelx_k, fft_conv_sum_half_panelx_k; picked only with bits 1 and 3 of offt_filter_desc::mixed), one shape
// per length for the full-line and the half-line form alike.  The radix orders and threads per line are those of
// offt_reg_conv_mixed_f64.hip (first and last radix even); the accumulator comes on top of those kernels' registers, so every
// instance is compiled for the fewest waves per SIMD its workgroup admits (convx_sum_wps) and has as many columns as fit
// 256 threads, one wave per SIMD: 320 has 6 columns instead of 8, 640 has 3 instead of 4 and 1000 has 2 instead of 4
// (contiguous lines coalesce whatever the column count).  No instance uses scratch memory (DESIGN.md 4.5 has the table).
#include "offt_panel.hpp"

namespace offtk {

void reg_conv_sum_mixed_f64() {
  reg_variantx_conv_sum<double, 96, 8, 4, 6, 4, 16, true>();
  reg_variantx_conv_sum<double, 192, 16, 12, 4, 4, 16, true>();
  reg_variantx_conv_sum<double, 320, 40, 8, 10, 4, 6, true>();
  reg_variantx_conv_sum<double, 384, 32, 12, 4, 8, 8, true>();
  reg_variantx_conv_sum<double, 640, 80, 10, 8, 8, 3, true>();
  reg_variantx_conv_sum<double, 768, 64, 12, 8, 8, 4, true>();
  reg_variantx_conv_sum<double, 1000, 100, 10, 10, 10, 2, true>();
}

}  // namespace offtk
