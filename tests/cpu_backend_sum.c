/*
 * cpu_backend_sum.c -- TEST INFRASTRUCTURE ONLY.
 *
 * The CPU backend chain (cpu_backend.c, _conv.c, _pad.c, _padreal.c) with the two entries of the multi-input convolution
 * filled: conv_pass_sum (the fused launch that gathers several sources into one destination) and pointwise_sum (the
 * multiply-and-sum sweep).  Both read every source of a line / an element before they store it, so the destination may be
 * one of the sources, and neither writes any other source.  The fused launch with half = 3 touches the lower half of its
 * lines only, on both sides.  Every entry the multi-input call uses is logged (kind, n, direction, ncols, nb1, half,
 * real_input, nin), so that the tests can read the route off the launches.
 * Built into tests/libcpubackend_sum.so (tests/test_convolve_sum.py), never into the library.
 */
#include <stdlib.h>
#include <string.h>
#include "offt_backend.h"
#include "oracle.h"

const offt_backend *cpu_backend_padreal_table(void);

static offt_backend g_base;                    /* the chain below this file: what the logging entries call */
static offt_backend g_full, g_nofused, g_old;  /* one static per table: asking for one never changes another that is installed */

enum { K_PASS = 0, K_CONV = 1, K_CONV_SUM = 2, K_POINTWISE = 3, K_POINTWISE_SUM = 4, K_MEMCPY = 5, K_ZERO = 6, K_COUNT = 7 };
static long g_count[K_COUNT];
#define LOG_MAX 512
#define REC 8
static int g_log[LOG_MAX][REC], g_nlog = 0;
static void note(int kind, const offt_pass_desc *d, int nin) {
  g_count[kind]++;
  if (g_nlog < LOG_MAX) {
    int *r = g_log[g_nlog++];
    memset(r, 0, sizeof g_log[0]);
    r[0] = kind;
    if (d) { r[1] = d->n; r[2] = d->direction; r[3] = d->ncols; r[4] = d->nb1; r[5] = d->half; r[6] = d->real_input; }
    r[7] = nin;
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

static int sum_pass(const offt_pass_desc *d, const void *in, void *out, void *stream) {
  note(K_PASS, d, 0);
  return g_base.pass(d, in, out, stream);
}
static int sum_conv_pass(const offt_pass_desc *d, const offt_filter_desc *f, const void *filter, void *data, void *stream) {
  note(K_CONV, d, 1);
  return g_base.conv_pass(d, f, filter, data, stream);
}
static int sum_pointwise(void *data, const void *filter, int precision, int kind, int n0, int n1, int n2, long long s0, long long s1,
                         long long s2, void *stream) {
  note(K_POINTWISE, NULL, 1);
  return g_base.pointwise(data, filter, precision, kind, n0, n1, n2, s0, s1, s2, stream);
}
static int sum_memcpy_dd(void *dst, const void *src, size_t bytes, void *stream) {
  note(K_MEMCPY, NULL, 0);
  return g_base.memcpy_dd(dst, src, bytes, stream);
}
static int sum_zero_outside(void *buf, int precision, int n0, int n1, int n2, int k0, int k1, int k2, long long s0, long long s1, long long s2,
                            void *stream) {
  note(K_ZERO, NULL, 0);
  return g_base.zero_outside(buf, precision, n0, n1, n2, k0, k1, k2, s0, s1, s2, stream);
}

/* offt_hipk_conv_pass_sum on host memory: per line, every source through the in_* side, forward FFT, times H_k, added in the
 * order k = 0 ... nin-1; inverse FFT of the sum, scale, stored at the same offsets of `dst`; half = 3: only indices < n/2
 * are loaded and stored */
static int sum_conv_pass_sum(const offt_pass_desc *d, const offt_filter_desc *f, int nin, const void *const *filters, const void *const *srcs,
                             void *dst, void *stream) {
  (void)stream;
  note(K_CONV_SUM, d, nin);
  if (nin < 1 || nin > OFFT_HIPK_CONV_MAX_IN || !filters || !srcs || !dst) return -1;
  if ((d->half && d->half != 3) || (d->half && (d->n & 1)) || d->real_input || d->in_split || d->in_split_nfloor ||
      (f->kind != 0 && f->kind != 1))
    return -1;
  if (d->n < 1 || d->ncols < 1 || d->nb1 < 1 || d->nb2 < 1) return 0;
  const int n = d->n, f32 = d->precision == OFFT_PREC_F32, nio = d->half ? n / 2 : n;
  orc_fft_plan *pl = orc_fft_plan_create(n);
  double *line = (double *)malloc(sizeof(double) * 2 * (size_t)n), *acc = (double *)malloc(sizeof(double) * 2 * (size_t)n),
         *scr = (double *)malloc(sizeof(double) * 6 * (size_t)n + 64);
  for (int b2 = 0; b2 < d->nb2; b2++)
    for (int b1 = 0; b1 < d->nb1; b1++)
      for (int c = 0; c < d->ncols; c++) {
        const long long ib = (long long)b1 * d->in_b1_stride + (long long)b2 * d->in_b2_stride + (long long)c * d->in_col_stride;
        const long long fb = (long long)b1 * f->b1_stride + (long long)b2 * f->b2_stride + (long long)c * f->col_stride;
        memset(acc, 0, sizeof(double) * 2 * (size_t)n);
        for (int k = 0; k < nin; k++) {
          memset(line, 0, sizeof(double) * 2 * (size_t)n);
          for (int i = 0; i < nio; i++) ld(srcs[k], f32, ib + (long long)i * d->in_axis_stride, &line[2 * i], &line[2 * i + 1]);
          orc_fft_execute(pl, line, 1, 0, 1, scr);
          for (int i = 0; i < n; i++) {
            const long long o = fb + (long long)i * f->axis_stride;
            double hr, hi = 0.0;
            if (f->kind == 1) ld(filters[k], f32, o, &hr, &hi);
            else hr = f32 ? ((const float *)filters[k])[o] : ((const double *)filters[k])[o];
            const double xr = line[2 * i], xi = line[2 * i + 1];
            acc[2 * i] += xr * hr - xi * hi;
            acc[2 * i + 1] += xr * hi + xi * hr;
          }
        }
        for (int i = 0; i < n; i++) acc[2 * i + 1] = -acc[2 * i + 1]; /* conjugated: the inverse as conj(F(conj(.))) */
        orc_fft_execute(pl, acc, 1, 0, 1, scr);
        for (int i = 0; i < nio; i++) st(dst, f32, ib + (long long)i * d->in_axis_stride, acc[2 * i] * d->scale, -acc[2 * i + 1] * d->scale);
      }
  free(line); free(acc); free(scr); orc_fft_plan_destroy(pl);
  return 0;
}

static int sum_pointwise_sum(int nin, const void *const *ins, const void *const *filters, void *out, int precision, int kind, int n0, int n1,
                             int n2, long long s0, long long s1, long long s2, void *stream) {
  (void)stream;
  note(K_POINTWISE_SUM, NULL, nin);
  if ((kind != 0 && kind != 1) || nin < 1 || nin > OFFT_HIPK_CONV_MAX_IN || !ins || !filters || !out) return -1;
  const int f32 = precision == OFFT_PREC_F32;
  for (int i0 = 0; i0 < n0; i0++)
    for (int i1 = 0; i1 < n1; i1++)
      for (int i2 = 0; i2 < n2; i2++) {
        const long long o = (long long)i0 * s0 + (long long)i1 * s1 + (long long)i2 * s2;
        double ar = 0.0, ai = 0.0;
        for (int k = 0; k < nin; k++) {
          double xr, xi, hr, hi = 0.0;
          ld(ins[k], f32, o, &xr, &xi);
          if (kind == 1) ld(filters[k], f32, o, &hr, &hi);
          else hr = f32 ? ((const float *)filters[k])[o] : ((const double *)filters[k])[o];
          ar += xr * hr - xi * hi;
          ai += xr * hi + xi * hr;
        }
        st(out, f32, o, ar, ai);
      }
  return 0;
}

/* the logging entries over the chain below; the two new entries stay NULL (what every older backend looks like to the library) */
static void make(offt_backend *t) {
  g_base = *cpu_backend_padreal_table();
  *t = g_base;
  t->pass = sum_pass;
  t->conv_pass = sum_conv_pass;
  t->pointwise = sum_pointwise;
  t->memcpy_dd = sum_memcpy_dd;
  t->zero_outside = sum_zero_outside;
  t->conv_pass_sum = NULL;
  t->pointwise_sum = NULL;
}
/* neither entry: the call is refused */
const offt_backend *cpu_backend_sum_table_old(void) { make(&g_old); return &g_old; }
const offt_backend *cpu_backend_sum_table(void) {
  make(&g_full);
  g_full.conv_pass_sum = sum_conv_pass_sum;
  g_full.pointwise_sum = sum_pointwise_sum;
  return &g_full;
}
/* the multiply-and-sum sweep, but no gather launch: no fused multi-input route */
const offt_backend *cpu_backend_sum_table_nofused(void) {
  make(&g_nofused);
  g_nofused.pointwise_sum = sum_pointwise_sum;
  return &g_nofused;
}
long cpu_backend_sum_count(int kind) { return kind >= 0 && kind < K_COUNT ? g_count[kind] : -1; }
void cpu_backend_sum_log_reset(void) { g_nlog = 0; }
int cpu_backend_sum_log_len(void) { return g_nlog; }
int cpu_backend_sum_log(int i, int *rec8) {
  if (i < 0 || i >= g_nlog) return -1;
  memcpy(rec8, g_log[i], sizeof g_log[i]);
  return 0;
}
