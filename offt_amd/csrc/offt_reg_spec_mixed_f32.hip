// offt_reg_spec_mixed_f32.hip -- single-precision filtered forward and filtered inverse kernels of mixed-radix lengths
// (fft_filt_fwd_panelx_k, fft_filt_inv_panelx_k; picked only with bit 4 of offt_filter_desc::mixed): the shapes of the fused
// convolution (offt_reg_conv_mixed_f32.hip), full lines only.  No instance uses scratch memory.
#include "offt_panel.hpp"

namespace offtk {

void reg_spec_mixed_f32() {
  reg_variantx_spec<float, 384, 16, 8, 8, 6, 16, true>();
  reg_variantx_spec<float, 640, 40, 16, 5, 8, 8, true>();
  reg_variantx_spec<float, 768, 32, 8, 8, 12, 16, true>();
  reg_variantx_spec<float, 1000, 50, 20, 5, 10, 8, true>();
}

}  // namespace offtk
