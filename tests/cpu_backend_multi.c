/*
 * cpu_backend_multi.c -- TEST INFRASTRUCTURE ONLY.
 *
 * The CPU backend chain (cpu_backend.c, _conv.c, _pad.c, _padreal.c) with the two entries of the multi-output convolution
 * filled: conv_pass_oop (the fused launch that stores somewhere other than where it loaded) and pointwise_oop (the multiply
 * with a separate destination).  Neither ever writes its source: the tests compare it afterwards.  The out-of-place fused
 * launch with half = 3 touches the lower half of its lines only, on both sides.  Every entry the multi-output call uses
 * is logged (kind, n, direction, ncols, nb1, half, real_input), so that the tests can read the route off the launches:
 * forward passes run once, one out-of-place launch per output and plane group, no multiply on the fused route.
 * Built into tests/libcpubackend_multi.so (tests/test_convolve_multi.py), never into the library.
 */
#include <stdlib.h>
#include <string.h>
#include "offt_backend.h"
#include "oracle.h"

const offt_backend *cpu_backend_padreal_table(void);
const offt_backend *cpu_backend_conv_table(void);
const offt_backend *cpu_backend_conv_table_none(void);

static offt_backend g_base;                       /* the chain below this file: what the logging entries call */
static offt_backend g_full, g_old, g_unfused;     /* one static per table: asking for one never changes another that is installed */

enum { K_PASS = 0, K_CONV = 1, K_CONV_OOP = 2, K_POINTWISE = 3, K_POINTWISE_OOP = 4, K_MEMCPY = 5, K_COUNT = 6 };
static long g_count[K_COUNT];
#define LOG_MAX 256
static int g_log[LOG_MAX][7], g_nlog = 0;
static void note(int kind, const offt_pass_desc *d) {
  g_count[kind]++;
  if (g_nlog < LOG_MAX) {
    int *r = g_log[g_nlog++];
    memset(r, 0, sizeof g_log[0]);
    r[0] = kind;
    if (d) { r[1] = d->n; r[2] = d->direction; r[3] = d->ncols; r[4] = d->nb1; r[5] = d->half; r[6] = d->real_input; }
  }
}

static void ld(const void *p, int f32, long long i, double *re, double *im) {
  if (f32) { *re = ((const float *)p)[2 * i]; *im = ((const float *)p)[2 * i + 1]; }
  else { *re = ((const double *)p)[2 * i]; *im = ((const double *)p)[2 * i + 1]; }
}
static void st(void *p, int f32, long long i, double re, double im) {
  if (f32) { ((float *)p)[2 * i] = (float)re; ((float *)p)[2 * i + 1] = (float)im; }
  else { ((double *)p)[2 * i] = re; ((double *)p)[2 * i + 1] = im; }
}

static int multi_pass(const offt_pass_desc *d, const void *in, void *out, void *stream) {
  note(K_PASS, d);
  return g_base.pass(d, in, out, stream);
}
static int multi_conv_pass(const offt_pass_desc *d, const offt_filter_desc *f, const void *filter, void *data, void *stream) {
  note(K_CONV, d);
  return g_base.conv_pass(d, f, filter, data, stream);
}
static int multi_pointwise(void *data, const void *filter, int precision, int kind, int n0, int n1, int n2, long long s0, long long s1,
                           long long s2, void *stream) {
  note(K_POINTWISE, NULL);
  return g_base.pointwise(data, filter, precision, kind, n0, n1, n2, s0, s1, s2, stream);
}
static int multi_memcpy_dd(void *dst, const void *src, size_t bytes, void *stream) {
  note(K_MEMCPY, NULL);
  return g_base.memcpy_dd(dst, src, bytes, stream);
}

/* offt_hipk_conv_pass_oop on host memory: lines through the in_* side of `src`, forward FFT, times H, inverse FFT, scale,
 * stored at the same offsets of `dst`; half = 3: only indices < n/2 are loaded and stored */
static int multi_conv_pass_oop(const offt_pass_desc *d, const offt_filter_desc *f, const void *filter, const void *src, void *dst,
                               void *stream) {
  (void)stream;
  note(K_CONV_OOP, d);
  if (src == dst) return -1;
  if ((d->half && d->half != 3) || (d->half && (d->n & 1)) || d->real_input || d->in_split || d->in_split_nfloor ||
      (f->kind != 0 && f->kind != 1))
    return -1;
  if (d->n < 1 || d->ncols < 1 || d->nb1 < 1 || d->nb2 < 1) return 0;
  const int n = d->n, f32 = d->precision == OFFT_PREC_F32, nio = d->half ? n / 2 : n;
  orc_fft_plan *pl = orc_fft_plan_create(n);
  double *line = (double *)malloc(sizeof(double) * 2 * (size_t)n), *scr = (double *)malloc(sizeof(double) * 6 * (size_t)n + 64);
  for (int b2 = 0; b2 < d->nb2; b2++)
    for (int b1 = 0; b1 < d->nb1; b1++)
      for (int c = 0; c < d->ncols; c++) {
        const long long ib = (long long)b1 * d->in_b1_stride + (long long)b2 * d->in_b2_stride + (long long)c * d->in_col_stride;
        const long long fb = (long long)b1 * f->b1_stride + (long long)b2 * f->b2_stride + (long long)c * f->col_stride;
        memset(line, 0, sizeof(double) * 2 * (size_t)n);
        for (int k = 0; k < nio; k++) ld(src, f32, ib + (long long)k * d->in_axis_stride, &line[2 * k], &line[2 * k + 1]);
        orc_fft_execute(pl, line, 1, 0, 1, scr);
        for (int k = 0; k < n; k++) {
          const long long o = fb + (long long)k * f->axis_stride;
          double hr, hi = 0.0;
          if (f->kind == 1) ld(filter, f32, o, &hr, &hi);
          else hr = f32 ? ((const float *)filter)[o] : ((const double *)filter)[o];
          const double xr = line[2 * k], xi = line[2 * k + 1];
          line[2 * k] = xr * hr - xi * hi;
          line[2 * k + 1] = -(xr * hi + xi * hr); /* conjugated: the inverse as conj(F(conj(.))) */
        }
        orc_fft_execute(pl, line, 1, 0, 1, scr);
        for (int k = 0; k < nio; k++)
          st(dst, f32, ib + (long long)k * d->in_axis_stride, line[2 * k] * d->scale, -line[2 * k + 1] * d->scale);
      }
  free(line); free(scr); orc_fft_plan_destroy(pl);
  return 0;
}

static int multi_pointwise_oop(const void *in, void *out, const void *filter, int precision, int kind, int n0, int n1, int n2,
                               long long s0, long long s1, long long s2, void *stream) {
  (void)stream;
  note(K_POINTWISE_OOP, NULL);
  if ((kind != 0 && kind != 1) || in == out) return -1;
  const int f32 = precision == OFFT_PREC_F32;
  for (int i0 = 0; i0 < n0; i0++)
    for (int i1 = 0; i1 < n1; i1++)
      for (int i2 = 0; i2 < n2; i2++) {
        const long long o = (long long)i0 * s0 + (long long)i1 * s1 + (long long)i2 * s2;
        double xr, xi, hr, hi = 0.0;
        ld(in, f32, o, &xr, &xi);
        if (kind == 1) ld(filter, f32, o, &hr, &hi);
        else hr = f32 ? ((const float *)filter)[o] : ((const double *)filter)[o];
        st(out, f32, o, xr * hr - xi * hi, xr * hi + xi * hr);
      }
  return 0;
}

/* the logging entries over the chain below; the two new entries stay NULL (what every older backend looks like to the library) */
static void make(offt_backend *t) {
  g_base = *cpu_backend_padreal_table();
  *t = g_base;
  t->pass = multi_pass;
  t->conv_pass = multi_conv_pass;
  t->pointwise = multi_pointwise;
  t->memcpy_dd = multi_memcpy_dd;
}
const offt_backend *cpu_backend_multi_table_old(void) { make(&g_old); return &g_old; }
const offt_backend *cpu_backend_multi_table(void) {
  make(&g_full);
  g_full.conv_pass_oop = multi_conv_pass_oop;
  g_full.pointwise_oop = multi_pointwise_oop;
  return &g_full;
}
/* the multiply with a separate destination, but no out-of-place fused launch: no fused multi route */
const offt_backend *cpu_backend_multi_table_unfused(void) {
  make(&g_unfused);
  g_unfused.pointwise_oop = multi_pointwise_oop;
  return &g_unfused;
}
long cpu_backend_multi_count(int kind) { return kind >= 0 && kind < K_COUNT ? g_count[kind] : -1; }
void cpu_backend_multi_log_reset(void) { g_nlog = 0; }
int cpu_backend_multi_log(int i, int *rec7) {
  if (i < 0 || i >= g_nlog) return -1;
  memcpy(rec7, g_log[i], sizeof g_log[i]);
  return 0;
}
