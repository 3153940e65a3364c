// offt_reg_half_mixed_f64.hip -- double-precision half-line kernels of mixed-radix lengths (fft_half_panelx_k;
// offt_pass_desc::half): the shapes (threads per line, columns) of the full-line instances of offt_reg_mixed_f64_*.hip, in the
// four forms the z-y-x half-box schedule and its mirror launch.  The first and the last radix of a half instance are even:
// 192 runs as 8 x 3 x 8 here (8 x 8 x 3 on full lines).  320 runs as 8 x 10 x 4 (10 x 8 x 4 on full lines): in the full-line
// order three of its four forms spill 32-52 B per lane at the 168 registers of three waves per SIMD, in this order none
// does.  Every other length keeps its radix order.  640 and 1000 keep the narrow contiguous / contiguous shape of their
// full-line kernels.
#include "offt_panel.hpp"

namespace offtk {

void reg_half_mixed_f64() {
  reg_variantx_half<double, 96, 8, 4, 6, 4, 16, true>();
  reg_variantx_half<double, 192, 8, 8, 3, 8, 16, true>();
  reg_variantx_half<double, 320, 16, 8, 10, 4, 8, true>();
  reg_variantx_half<double, 384, 16, 12, 4, 8, 16, true>();
  reg_variantx_half<double, 640, 80, 10, 8, 8, 8, true, H_CS1 | H_SC2>();
  reg_variantx_half<double, 640, 80, 10, 8, 8, 4, true, H_CC1 | H_CC2>();
  reg_variantx_half<double, 768, 32, 12, 8, 8, 8, true>();
  reg_variantx_half<double, 1000, 100, 10, 10, 10, 8, true, H_CS1 | H_SC2>();
  reg_variantx_half<double, 1000, 100, 10, 10, 10, 4, true, H_CC1 | H_CC2>();
}

}  // namespace offtk
