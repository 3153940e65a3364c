// Every registry query of offt_hipk.h that needs no device, over a small product of descriptors, printed line by line.
// A stand-alone program (`make asan-registry` builds the host side of the kernel sources under ASan + UBSan and runs it):
// it launches nothing and touches no device memory, so it runs on a machine without a GPU.  Two builds that print the
// same text resolve these descriptors alike.
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include "offt_hipk.h"

static const int LENGTHS[] = {32, 64, 128, 256, 512, 1024, 2048, 96, 192, 320, 384, 640, 768, 1000, 100, 896, 1536, 1, 7, 1019, 4096, 8192, 10007};

static offt_pass_desc desc(int n, int prec, int inc, int outc, int ncols) {
  offt_pass_desc d;
  memset(&d, 0, sizeof d);
  d.n = n; d.precision = prec; d.direction = -1; d.ncols = ncols; d.nb1 = 4; d.nb2 = 1; d.scale = 1.0; d.variant = -1;
  d.in_contig = inc; d.out_contig = outc;
  d.in_axis_stride = inc ? 1 : ncols + (ncols & 1); d.in_col_stride = inc ? 2 * n : 1;
  d.out_axis_stride = outc ? 1 : ncols + (ncols & 1); d.out_col_stride = outc ? 2 * n : 1;
  d.in_b1_stride = d.out_b1_stride = 2LL * n * 64;
  return d;
}

int main() {
  static const char tab[64] = "";
  for (int n : LENGTHS)
    for (int prec : {OFFT_PREC_F64, OFFT_PREC_F32}) {
      const int count = offt_hipk_variant_count(n, prec);
      printf("n=%d prec=%d fast=%d count=%d\n", n, prec, offt_hipk_has_fast_path(n, prec), count);
      for (int v : {-1, 0, 1, 2, 3, 57, 100, 200, 201}) {
        int e = -9, cols = -9;
        const int id = offt_hipk_variant_info(n, prec, v, &e, &cols);
        printf(" variant %d: id=%d e=%d cols=%d %s\n", v, id, e, cols, offt_hipk_variant_name(n, prec, v));
      }
      for (int half = 0; half <= 8; ++half)
        for (int flav = 0; flav < 4; ++flav)
          for (int real = 0; real <= 2; ++real)
            for (int ncols : {64, 63})
              for (int bits = 0; bits < 16; ++bits) {  // no_pairs, in_split, tw4, out_keep
                offt_pass_desc d = desc(n, prec, flav < 2, (flav & 1) == 0, ncols);
                d.half = half; d.real_input = real;
                d.no_pairs = bits & 1;
                if (bits & 2) { d.in_split = 8; d.in_block_stride = 4096; }
                d.tw4 = (bits & 4) ? tab : nullptr;
                d.out_keep = (bits & 8) != 0;
                printf(" half=%d flav=%d real=%d ncols=%d bits=%d: %s has_half=%d keeps=%d\n", half, flav, real, ncols, bits, offt_hipk_kernel_name(&d),
                       offt_hipk_has_half(&d), offt_hipk_keeps_output(&d));
              }
      for (int half : {0, 1, 3})
        for (int mixed = 0; mixed < 4; ++mixed)
          for (int kind = 0; kind <= 2; ++kind)
            for (int bits = 0; bits < 16; ++bits) {  // filter axis stride 2, strided input, real input, in_split
              offt_pass_desc d = desc(n, prec, !(bits & 2), 1, 64);
              d.half = half; d.real_input = (bits & 4) ? 1 : 0;
              if (bits & 8) { d.in_split = 8; d.in_block_stride = 4096; }
              offt_filter_desc f;
              memset(&f, 0, sizeof f);
              f.kind = kind; f.mixed = mixed; f.axis_stride = (bits & 1) ? 2 : 1; f.col_stride = n; f.b1_stride = 64LL * n;
              printf(" conv half=%d mixed=%d kind=%d bits=%d: %s %d | %s %d\n", half, mixed, kind, bits, offt_hipk_conv_kernel_name(&d, &f),
                     offt_hipk_conv_has_fused(&d, &f), offt_hipk_conv_oop_kernel_name(&d, &f), offt_hipk_conv_has_fused_oop(&d, &f));
            }
    }
  // the queries refuse null descriptors instead of reading them
  printf("null: %d %d %s %d %s\n", offt_hipk_has_half(nullptr), offt_hipk_conv_has_fused(nullptr, nullptr), offt_hipk_conv_kernel_name(nullptr, nullptr),
         offt_hipk_conv_has_fused_oop(nullptr, nullptr), offt_hipk_conv_oop_kernel_name(nullptr, nullptr));
  return 0;
}
