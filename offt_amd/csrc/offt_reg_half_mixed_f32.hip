// offt_reg_half_mixed_f32.hip -- single-precision half-line kernels of mixed-radix lengths (fft_half_panelx_k;
// offt_pass_desc::half), one column per lane: the shapes of the full-line instances of offt_reg_mixed_f32_*.hip.  The first and
// the last radix of a half instance are even: 640 runs as 16 x 5 x 8 (16 x 8 x 5 on full lines) and 1000 as 20 x 5 x 10
// (25 x 8 x 5), whose 50 and 100 butterflies of the first and the last stage do not fill 40 threads a line evenly -- the last
// one of a thread is predicated (10 x 10 x 10 on 40 threads spills 64-72 B per lane at 128 registers; this order does not).
#include "offt_panel.hpp"

namespace offtk {

void reg_half_mixed_f32() {
  reg_variantx_half<float, 384, 16, 8, 8, 6, 16, true>();
  reg_variantx_half<float, 640, 40, 16, 5, 8, 16, true>();
  reg_variantx_half<float, 768, 32, 8, 8, 12, 16, true>();
  reg_variantx_half<float, 1000, 40, 20, 5, 10, 16, true>();
}

}  // namespace offtk
