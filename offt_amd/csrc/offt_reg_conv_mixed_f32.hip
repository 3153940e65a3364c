// offt_reg_conv_mixed_f32.hip -- single-precision fused convolution kernels of mixed-radix lengths (fft_conv_panelx_k,
// fft_conv_half_panelx_k; picked only with offt_filter_desc::mixed), one shape per length for the full-line and the
// half-line form alike: the radix orders and threads per line of offt_reg_half_mixed_f32.hip, whose first and last radix
// are even.  640 runs on 40 threads a line, which do not divide the 128 butterflies of its middle stage: the last butterfly
// of a thread is predicated.  16 columns of 40 threads are 10 waves, i.e. 3 per SIMD and 168 registers, where 640 spills 52 B
// per lane and 1000 384 B: both run 8 columns a workgroup (2 waves per SIMD, 256 registers).  1000 on 40 threads (40 points
// a thread) still spills 52 B there, and 36-76 B as 10 x 10 x 10; on 50 threads (20 points, every stage even) it does not.
// No instance uses scratch memory.
#include "offt_panel.hpp"

namespace offtk {

template <int N, int TPL, int R0, int R1, int R2, int COLS>
static void both() {
  reg_variantx_conv<float, N, TPL, R0, R1, R2, COLS, true>();
  reg_variantx_conv_half<float, N, TPL, R0, R1, R2, COLS, true>();
}

void reg_conv_mixed_f32() {
  both<384, 16, 8, 8, 6, 16>();
  both<640, 40, 16, 5, 8, 8>();
  both<768, 32, 8, 8, 12, 16>();
  both<1000, 50, 20, 5, 10, 8>();
}

}  // namespace offtk
