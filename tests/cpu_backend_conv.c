/*
 * cpu_backend_conv.c -- TEST INFRASTRUCTURE ONLY.
 *
 * The CPU descriptor interpreter of cpu_backend.c with the two spectral-convolution entries of offt_backend filled:
 * conv_pass (the fused forward-pass . filter . inverse-pass launch) and pointwise (the multiply of the unfused route),
 * both interpreted with the oracle's 1-D FFT.  Its pass entry also takes real-output lines (real_input = 2, the c2r z
 * pass), so that r2c plans convolve on the CPU too; every other descriptor goes to cpu_backend.c.  Built into
 * tests/libcpubackend_conv.so (tests/test_convolve.py), never into the library.
 */
#include <stdlib.h>
#include <string.h>
#include "offt_backend.h"
#include "oracle.h"

const offt_backend *cpu_backend_table(void);

static offt_backend g_table;
static long g_conv_count = 0, g_pointwise_count = 0;

static void ld(const void *p, int f32, long long i, double *re, double *im) {
  if (f32) { *re = ((const float *)p)[2 * i]; *im = ((const float *)p)[2 * i + 1]; }
  else { *re = ((const double *)p)[2 * i]; *im = ((const double *)p)[2 * i + 1]; }
}
static void st(void *p, int f32, long long i, double re, double im) {
  if (f32) { ((float *)p)[2 * i] = (float)re; ((float *)p)[2 * i + 1] = (float)im; }
  else { ((double *)p)[2 * i] = re; ((double *)p)[2 * i + 1] = im; }
}
static double ldh(const void *p, int f32, long long i) { return f32 ? ((const float *)p)[i] : ((const double *)p)[i]; }

static long long split_off(int k, int split, int nfloor, long long blk, long long axis, const long long *tab) {
  if (split == 0 && nfloor == 0) return (long long)k * axis;
  int a, r;
  if (nfloor > 0 && k >= split * nfloor) { int kk = k - split * nfloor; a = nfloor + kk / (split + 1); r = kk % (split + 1); }
  else { a = k / split; r = k % split; }
  return (tab ? tab[a] : (long long)a * blk) + (long long)r * axis;
}

/* real-output line (offt_hipk.h, real_input = 2): n/2+1 complex values in, their conjugate-symmetric extension
 * transformed (inverse), the n real parts at the head of the output row */
static int c2r_pass(const offt_pass_desc *d, const void *in, void *out) {
  if (d->n < 1 || d->ncols < 1 || d->nb1 < 1 || d->nb2 < 1) return 0;
  const int n = d->n, f32 = d->precision == OFFT_PREC_F32;
  orc_fft_plan *pl = orc_fft_plan_create(n);
  double *line = (double *)malloc(sizeof(double) * 2 * (size_t)n), *scr = (double *)malloc(sizeof(double) * 6 * (size_t)n + 64);
  for (int b2 = 0; b2 < d->nb2; b2++)
    for (int b1 = 0; b1 < d->nb1; b1++)
      for (int c = 0; c < d->ncols; c++) {
        long long ib = (long long)b1 * d->in_b1_stride + (long long)b2 * d->in_b2_stride + (long long)c * d->in_col_stride;
        long long ob = (long long)b1 * d->out_b1_stride + (long long)b2 * d->out_b2_stride + (long long)c * d->out_col_stride;
        for (int k = 0; k < n; k++) {
          const int m = k <= n / 2 ? k : n - k;
          double re, im;
          ld(in, f32, ib + split_off(m, d->in_split, d->in_split_nfloor, d->in_block_stride, d->in_axis_stride, d->in_block_tab), &re, &im);
          if (k > n / 2) im = -im;
          line[2 * k] = re; line[2 * k + 1] = -im; /* inverse = conj(F(conj(.))) */
        }
        orc_fft_execute(pl, line, 1, 0, 1, scr);
        for (int k = 0; k < n; k++) {
          if (f32) ((float *)out)[2 * ob + k] = (float)(line[2 * k] * d->scale);
          else ((double *)out)[2 * ob + k] = line[2 * k] * d->scale;
        }
      }
  free(line); free(scr); orc_fft_plan_destroy(pl);
  return 0;
}

static int conv_cb_pass(const offt_pass_desc *d, const void *in, void *out, void *stream) {
  if (d->real_input == 2) return c2r_pass(d, in, out);
  return cpu_backend_table()->pass(d, in, out, stream);
}

/* fused launch: lines through the in_* side, forward FFT, times H at the filter strides, inverse FFT, scale, back in place */
static int conv_cb_conv_pass(const offt_pass_desc *d, const offt_filter_desc *f, const void *filter, void *data, void *stream) {
  (void)stream;
  g_conv_count++;
  if (d->n < 1 || d->ncols < 1 || d->nb1 < 1 || d->nb2 < 1) return 0;
  if (d->real_input || d->in_split || d->in_split_nfloor || (f->kind != 0 && f->kind != 1)) return -1;
  const int n = d->n, f32 = d->precision == OFFT_PREC_F32;
  orc_fft_plan *pl = orc_fft_plan_create(n);
  double *line = (double *)malloc(sizeof(double) * 2 * (size_t)n), *scr = (double *)malloc(sizeof(double) * 6 * (size_t)n + 64);
  for (int b2 = 0; b2 < d->nb2; b2++)
    for (int b1 = 0; b1 < d->nb1; b1++)
      for (int c = 0; c < d->ncols; c++) {
        const long long ib = (long long)b1 * d->in_b1_stride + (long long)b2 * d->in_b2_stride + (long long)c * d->in_col_stride;
        const long long fb = (long long)b1 * f->b1_stride + (long long)b2 * f->b2_stride + (long long)c * f->col_stride;
        for (int k = 0; k < n; k++) ld(data, f32, ib + (long long)k * d->in_axis_stride, &line[2 * k], &line[2 * k + 1]);
        orc_fft_execute(pl, line, 1, 0, 1, scr);
        for (int k = 0; k < n; k++) {
          const long long o = fb + (long long)k * f->axis_stride;
          double hr, hi = 0.0;
          if (f->kind == 1) ld(filter, f32, o, &hr, &hi);
          else hr = ldh(filter, f32, o);
          const double xr = line[2 * k], xi = line[2 * k + 1];
          line[2 * k] = xr * hr - xi * hi;
          line[2 * k + 1] = -(xr * hi + xi * hr); /* conjugated: the inverse as conj(F(conj(.))) */
        }
        orc_fft_execute(pl, line, 1, 0, 1, scr);
        for (int k = 0; k < n; k++)
          st(data, f32, ib + (long long)k * d->in_axis_stride, line[2 * k] * d->scale, -line[2 * k + 1] * d->scale);
      }
  free(line); free(scr); orc_fft_plan_destroy(pl);
  return 0;
}

static int conv_cb_pointwise(void *data, const void *filter, int precision, int kind, int n0, int n1, int n2, long long s0, long long s1,
                             long long s2, void *stream) {
  (void)stream;
  g_pointwise_count++;
  if (kind != 0 && kind != 1) return -1;
  const int f32 = precision == OFFT_PREC_F32;
  for (int i0 = 0; i0 < n0; i0++)
    for (int i1 = 0; i1 < n1; i1++)
      for (int i2 = 0; i2 < n2; i2++) {
        const long long o = (long long)i0 * s0 + (long long)i1 * s1 + (long long)i2 * s2;
        double xr, xi, hr, hi = 0.0;
        ld(data, f32, o, &xr, &xi);
        if (kind == 1) ld(filter, f32, o, &hr, &hi);
        else hr = ldh(filter, f32, o);
        st(data, f32, o, xr * hr - xi * hi, xr * hi + xi * hr);
      }
  return 0;
}

const offt_backend *cpu_backend_conv_table(void) {
  g_table = *cpu_backend_table();
  g_table.pass = conv_cb_pass;
  g_table.conv_pass = conv_cb_conv_pass;
  g_table.pointwise = conv_cb_pointwise;
  return &g_table;
}
/* the plain table with only the multiply filled: every convolve takes the unfused route */
const offt_backend *cpu_backend_conv_table_unfused(void) {
  cpu_backend_conv_table();
  g_table.conv_pass = NULL;
  return &g_table;
}
/* the plain table with neither entry (as tests/cpu_backend.c fills it): convolve is refused */
const offt_backend *cpu_backend_conv_table_none(void) {
  cpu_backend_conv_table();
  g_table.conv_pass = NULL;
  g_table.pointwise = NULL;
  return &g_table;
}
long cpu_backend_conv_count(void) { return g_conv_count; }
long cpu_backend_pointwise_count(void) { return g_pointwise_count; }
