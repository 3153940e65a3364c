// offt_reg_pair_yx_f64.hip -- two passes of the forward z-y-x schedule in one grid (offt_hipk_fft_pass_pair): the x pass of
// one group of z-planes next to the y pass of the following group.  The two work on different planes, so nothing orders
// them inside the launch: no flag, no atomic, no wait.  What x reads was stored by the launch before.
#include "offt_panel.hpp"

namespace offtk {

// One entry, two bodies: a workgroup-uniform branch on the block index hands the workgroup to the y pass's contig-in /
// strided-out KEEP body or to the x pass's contig / contig body, each on its role-local block index (the XCD-aware panel
// order of panel_body works on that index; a run is a multiple of 8 blocks, so the index keeps its XCD).
// Dispatch order: runs of `run` = 2^run_shift blocks alternate x, y, x, y, ... while both roles have a whole run left
// (blocks below 2 * both); behind them the rest of x, then the rest of y.  x goes first: its input is what the previous
// launch left in the cache.  The order is a matter of speed only.
// Both shapes have the same number of threads; the dynamic LDS is the larger of the two footprints.
template <typename T, int NY, int EY, int R0Y, int R1Y, int R2Y, int COLSY, bool SPLITY, int NX, int EX, int R0X, int R1X, int R2X, int COLSX,
          bool SPLITX>
__global__ void __launch_bounds__((NY / EY) * COLSY, (PanelCfg<NY, EY, R0Y, R1Y, R2Y, COLSY, SPLITY, T>::WPS_E < PanelCfg<NX, EX, R0X, R1X, R2X, COLSX, SPLITX, T>::WPS_E
                                                          ? PanelCfg<NY, EY, R0Y, R1Y, R2Y, COLSY, SPLITY, T>::WPS_E
                                                          : PanelCfg<NX, EX, R0X, R1X, R2X, COLSX, SPLITX, T>::WPS_E))
fft_pair_yx_k(PassArgs ay, const typename vec2<T>::type *iny, typename vec2<T>::type *outy, const typename vec2<T>::type *twy, PassArgs ax,
              const typename vec2<T>::type *inx, typename vec2<T>::type *outx, const typename vec2<T>::type *twx, unsigned nx, unsigned both,
              unsigned run_shift) {
  static_assert((NY / EY) * COLSY == (NX / EX) * COLSX, "both roles run the same number of threads");
  const unsigned b = blockIdx.x;
  bool is_x;
  unsigned l;
  if (b < 2u * both) {
    const unsigned r = b >> run_shift;
    is_x = (r & 1u) == 0u;
    l = ((r >> 1) << run_shift) + (b & ((1u << run_shift) - 1u));
  } else {
    const unsigned rest = b - 2u * both;
    is_x = rest < nx - both;
    l = is_x ? both + rest : both + rest - (nx - both);
  }
  if (is_x) panel_body<T, NX, EX, R0X, R1X, R2X, COLSX, true, true, SPLITX, false, false, false, false>(ax, inx, outx, twx, l);
  else panel_body<T, NY, EY, R0Y, R1Y, R2Y, COLSY, true, false, SPLITY, false, true, false, false>(ay, iny, outy, twy, l);
}

// (y shape, registry id of that shape at NY; x shape, registry id at NX): the shapes and ids of the defaults in
// offt_reg_pow2_f64.hip and offt_reg_pow2_f64_1024.hip -- the launcher checks both against what the two descriptors resolve
// to on their own, and a pair whose passes would run on anything else is not taken
template <int NY, int EY, int R0Y, int R1Y, int R2Y, int COLSY, bool SPLITY, int IDY, int NX, int EX, int R0X, int R1X, int R2X, int COLSX,
          bool SPLITX, int IDX>
void reg_pair() {
  VariantShape s = panel_shape<double, NY, EY, R0Y, R1Y, R2Y, COLSY, SPLITY>();
  const VariantShape sx = panel_shape<double, NX, EX, R0X, R1X, R2X, COLSX, SPLITX>();
  if (sx.lds > s.lds) s.lds = sx.lds;
  char suffix[64];
  snprintf(suffix, sizeof suffix, " + x pass N=%d E=%d cols=%d in one grid", NX, EX, COLSX);
  add_variant(VariantKey{NY, OFFT_PREC_F64, true, false, Role::PairYX, true, 0}, s,
              (const void *)fft_pair_yx_k<double, NY, EY, R0Y, R1Y, R2Y, COLSY, SPLITY, NX, EX, R0X, R1X, R2X, COLSX, SPLITX>, "fft_pair_yx_k", suffix, NX,
              false);
  Variant &v = registry().back();
  v.pair_y_id = IDY; v.pair_x_id = IDX; v.pair_x_cols = COLSX;
}

// Only pairs whose union keeps each body's own occupancy: equal lengths, so both roles have one shape (equal threads, VGPR
// budget and LDS).  A short body next to a longer one would run at the longer one's register count (64 points: 54 VGPRs
// and 8 waves per SIMD alone, 4 next to the 128-point body), so such plans keep their alternating launches.
#define SAME(...) reg_pair<__VA_ARGS__, __VA_ARGS__>()
void reg_pair_yx_f64() {
  SAME(64, 8, 8, 8, 1, 8, false, 0);
  SAME(128, 16, 16, 8, 1, 8, false, 0);
  SAME(256, 16, 16, 16, 1, 8, false, 0);
  SAME(512, 16, 16, 16, 2, 8, true, 1);
  SAME(1024, 16, 16, 16, 4, 8, true, 1);  // the headline: 1024^3
}
#undef SAME

}  // namespace offtk
