// offt_reg_spec_f64.hip -- double-precision filtered forward and filtered inverse kernels (fft_filt_fwd_panel_k,
// fft_filt_inv_panel_k): the shapes of the fused convolution (offt_reg_conv_f64.hip), every power of two from 64 to 1024 points
#include "offt_panel.hpp"

namespace offtk {

void reg_spec_f64() {
  reg_variant_filt<double, 64, 8, 8, 8, 1, 8, false>();
  reg_variant_filt<double, 128, 16, 16, 8, 1, 8, false>();
  reg_variant_filt<double, 256, 16, 16, 16, 1, 8, false>();
  reg_variant_filt<double, 512, 16, 16, 16, 2, 8, true>();
  reg_variant_filt<double, 1024, 16, 16, 16, 4, 8, true>();
}

}  // namespace offtk
