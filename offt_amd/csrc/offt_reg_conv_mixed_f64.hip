// offt_reg_conv_mixed_f64.hip -- double-precision fused convolution kernels of mixed-radix lengths (fft_conv_panelx_k,
// fft_conv_half_panelx_k; picked only with offt_filter_desc::mixed), one shape per length for the full-line and the
// half-line form alike, first and last radix even.  96, 640 and 1000 have the contiguous / contiguous shapes of
// offt_reg_half_mixed_f64.hip.  The other four spill in those shapes at the 256 registers of two waves per SIMD (192: 40-168 B
// per lane, 320: 40-52 B, 384 and 768: 268-332 B -- the filter values and the second transform's live ranges on top of 24
// points a thread) and run on more threads a line with the same radix order: 320 on 40 (10 points a thread), 384 on 32
// and 768 on 64 (16 points; the second butterfly of 768's last two stages is predicated); 192 as 12 x 4 x 4 on 16
// threads (12 points; 8 x 3 x 8 leaves 24 butterflies of a stage to 16 threads).  No instance uses scratch memory.
#include "offt_panel.hpp"

namespace offtk {

template <int N, int TPL, int R0, int R1, int R2, int COLS>
static void both() {
  reg_variantx_conv<double, N, TPL, R0, R1, R2, COLS, true>();
  reg_variantx_conv_half<double, N, TPL, R0, R1, R2, COLS, true>();
}

void reg_conv_mixed_f64() {
  both<96, 8, 4, 6, 4, 16>();
  both<192, 16, 12, 4, 4, 16>();
  both<320, 40, 8, 10, 4, 8>();
  both<384, 32, 12, 4, 8, 8>();
  both<640, 80, 10, 8, 8, 4>();
  both<768, 64, 12, 8, 8, 4>();
  both<1000, 100, 10, 10, 10, 4>();
}

}  // namespace offtk
