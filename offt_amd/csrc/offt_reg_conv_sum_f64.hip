// offt_reg_conv_sum_f64.hip -- double-precision multi-input fused convolution kernels (fft_conv_sum_panel_k,
// fft_conv_sum_half_panel_k): every power of two from 64 to 1024 points.  The stage shapes are those of
// offt_reg_conv_f64.hip; the 1024-point instance has four columns instead of eight (one wave per SIMD: the accumulator
// needs the registers, and contiguous lines coalesce whatever the column count)
#include "offt_panel.hpp"

namespace offtk {

void reg_conv_sum_f64() {
  reg_variant_conv_sum<double, 64, 8, 8, 8, 1, 8, false>();
  reg_variant_conv_sum<double, 128, 16, 16, 8, 1, 8, false>();
  reg_variant_conv_sum<double, 256, 16, 16, 16, 1, 8, false>();
  reg_variant_conv_sum<double, 512, 16, 16, 16, 2, 8, true>();
  reg_variant_conv_sum<double, 1024, 16, 16, 16, 4, 4, true>();
}

}  // namespace offtk
