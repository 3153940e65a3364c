// offt_reg_conv_sum_mixed_f32.hip -- single-precision multi-input fused convolution kernels of mixed-radix lengths
// (fft_conv_sum_panelx_k, fft_conv_sum_half_panelx_k; picked only with bits 1 and 3 of offt_filter_desc::mixed), one shape
// per length for the full-line and the half-line form alike, with the radix orders of offt_reg_conv_mixed_f32.hip (first and
// last radix even).  Every instance is compiled for one wave per SIMD (convx_sum_wps) and has at most 256 threads.  640 and
// 1000 keep their threads per line and run 6 and 5 columns.  384 on 16 threads a line (24 points a thread) spills 88 B per
// lane in the full-line form even with all 512 registers, as 6 x 8 x 8 156 B and as 8 x 6 x 8 80 B; 768 on 32 threads spills
// 120 B.  Both run on twice the threads a line (384 on 32, 768 on 64: 16 points a thread, the second butterfly of the two
// radix-8 stages predicated) and half the columns.  No instance uses scratch memory (DESIGN.md 4.5 has the table).
#include "offt_panel.hpp"

namespace offtk {

void reg_conv_sum_mixed_f32() {
  reg_variantx_conv_sum<float, 384, 32, 8, 8, 6, 8, true>();
  reg_variantx_conv_sum<float, 640, 40, 16, 5, 8, 6, true>();
  reg_variantx_conv_sum<float, 768, 64, 8, 8, 12, 4, true>();
  reg_variantx_conv_sum<float, 1000, 50, 20, 5, 10, 5, true>();
}

}  // namespace offtk
