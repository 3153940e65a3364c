// offt_reg_spec_mixed_f64.hip -- double-precision filtered forward and filtered inverse kernels of mixed-radix lengths
// (fft_filt_fwd_panelx_k, fft_filt_inv_panelx_k; picked only with bit 4 of offt_filter_desc::mixed): the shapes of the fused
// convolution (offt_reg_conv_mixed_f64.hip), full lines only.  No instance uses scratch memory.
#include "offt_panel.hpp"

namespace offtk {

void reg_spec_mixed_f64() {
  reg_variantx_spec<double, 96, 8, 4, 6, 4, 16, true>();
  reg_variantx_spec<double, 192, 16, 12, 4, 4, 16, true>();
  reg_variantx_spec<double, 320, 40, 8, 10, 4, 8, true>();
  reg_variantx_spec<double, 384, 32, 12, 4, 8, 8, true>();
  reg_variantx_spec<double, 640, 80, 10, 8, 8, 4, true>();
  reg_variantx_spec<double, 768, 64, 12, 8, 8, 4, true>();
  reg_variantx_spec<double, 1000, 100, 10, 10, 10, 4, true>();
}

}  // namespace offtk
