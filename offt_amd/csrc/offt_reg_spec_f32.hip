// offt_reg_spec_f32.hip -- single-precision filtered forward and filtered inverse kernels (fft_filt_fwd_panel_k,
// fft_filt_inv_panel_k): the one-column shapes of the fused convolution (offt_reg_conv_f32.hip), every power of two from 64
// to 1024 points
#include "offt_panel.hpp"

namespace offtk {

void reg_spec_f32() {
  reg_variant_filt<float, 64, 8, 8, 8, 1, 16, false>();
  reg_variant_filt<float, 128, 16, 16, 8, 1, 16, false>();
  reg_variant_filt<float, 256, 16, 16, 16, 1, 16, false>();
  reg_variant_filt<float, 512, 32, 32, 16, 1, 8, false>();
  reg_variant_filt<float, 1024, 32, 32, 32, 1, 8, false>();
}

}  // namespace offtk
