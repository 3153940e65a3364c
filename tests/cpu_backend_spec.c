/*
 * cpu_backend_spec.c -- TEST INFRASTRUCTURE ONLY.
 *
 * The CPU backend chain (cpu_backend.c, _conv.c, _pad.c, _padreal.c, _multi.c) with the two entries of the filtered
 * transforms filled: filt_pass_fwd (the forward x pass with the filter on its stores, in place) and filt_pass_inv (the
 * inverse x pass with the filter on its loads, src -> dst; dst may be src, and src is never written otherwise: the tests
 * compare it afterwards).  Both address their lines through the in_* side of the descriptor and ignore its direction.
 * Every entry the two calls use is logged (kind, n, direction, ncols, nb1, half, real_input, out_keep, src == dst), so that
 * the tests can read the route off the launches.
 * Built into tests/libcpubackend_spec.so (tests/test_spectral_filtered.py), never into the library.
 */
#include <stdlib.h>
#include <string.h>
#include "offt_backend.h"
#include "oracle.h"

const offt_backend *cpu_backend_multi_table(void);
const offt_backend *cpu_backend_conv_table_none(void);

static offt_backend g_base;                    /* the chain below this file: what the logging entries call */
static offt_backend g_full, g_nofilt, g_old;   /* one static per table: asking for one never changes another that is installed */

enum { K_PASS = 0, K_FILT_FWD = 1, K_FILT_INV = 2, K_POINTWISE = 3, K_POINTWISE_OOP = 4, K_MEMCPY = 5, K_ZERO = 6, K_COUNT = 7 };
static long g_count[K_COUNT];
#define LOG_MAX 512
#define REC 9
static int g_log[LOG_MAX][REC], g_nlog = 0;
static void note(int kind, const offt_pass_desc *d, int same) {
  g_count[kind]++;
  if (g_nlog < LOG_MAX) {
    int *r = g_log[g_nlog++];
    memset(r, 0, sizeof g_log[0]);
    r[0] = kind;
    if (d) { r[1] = d->n; r[2] = d->direction; r[3] = d->ncols; r[4] = d->nb1; r[5] = d->half; r[6] = d->real_input; r[7] = d->out_keep; }
    r[8] = same;
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

static int spec_pass(const offt_pass_desc *d, const void *in, void *out, void *stream) {
  note(K_PASS, d, in == out);
  return g_base.pass(d, in, out, stream);
}
static int spec_pointwise(void *data, const void *filter, int precision, int kind, int n0, int n1, int n2, long long s0, long long s1,
                          long long s2, void *stream) {
  note(K_POINTWISE, NULL, 1);
  return g_base.pointwise(data, filter, precision, kind, n0, n1, n2, s0, s1, s2, stream);
}
static int spec_pointwise_oop(const void *in, void *out, const void *filter, int precision, int kind, int n0, int n1, int n2,
                              long long s0, long long s1, long long s2, void *stream) {
  note(K_POINTWISE_OOP, NULL, 0);
  return g_base.pointwise_oop(in, out, filter, precision, kind, n0, n1, n2, s0, s1, s2, stream);
}
static int spec_memcpy_dd(void *dst, const void *src, size_t bytes, void *stream) {
  note(K_MEMCPY, NULL, 0);
  return g_base.memcpy_dd(dst, src, bytes, stream);
}
static int spec_zero_outside(void *buf, int precision, int n0, int n1, int n2, int k0, int k1, int k2, long long s0, long long s1, long long s2,
                             void *stream) {
  note(K_ZERO, NULL, 0);
  return g_base.zero_outside(buf, precision, n0, n1, n2, k0, k1, k2, s0, s1, s2, stream);
}

/* the two launches on host memory.  inv = 0: line -> FFT -> times H -> times scale, stored where it came from.  inv = 1: line
 * times H, conjugated, FFT, conjugated, times scale (the unnormalised inverse), stored at the same offsets of `dst`. */
static int filt_lines(const offt_pass_desc *d, const offt_filter_desc *f, const void *filter, const void *src, void *dst, int inv) {
  if (!filter || !src || !dst) return -1;
  if (d->half || d->real_input || d->in_split || d->in_split_nfloor || (f->kind != 0 && f->kind != 1)) return -1;
  if (d->n < 1 || d->ncols < 1 || d->nb1 < 1 || d->nb2 < 1) return 0;
  const int n = d->n, f32 = d->precision == OFFT_PREC_F32;
  orc_fft_plan *pl = orc_fft_plan_create(n);
  double *line = (double *)malloc(sizeof(double) * 2 * (size_t)n), *scr = (double *)malloc(sizeof(double) * 6 * (size_t)n + 64);
  for (int b2 = 0; b2 < d->nb2; b2++)
    for (int b1 = 0; b1 < d->nb1; b1++)
      for (int c = 0; c < d->ncols; c++) {
        const long long ib = (long long)b1 * d->in_b1_stride + (long long)b2 * d->in_b2_stride + (long long)c * d->in_col_stride;
        const long long fb = (long long)b1 * f->b1_stride + (long long)b2 * f->b2_stride + (long long)c * f->col_stride;
        for (int k = 0; k < n; k++) ld(src, f32, ib + (long long)k * d->in_axis_stride, &line[2 * k], &line[2 * k + 1]);
        if (!inv) orc_fft_execute(pl, line, 1, 0, 1, scr);
        for (int k = 0; k < n; k++) {
          const long long o = fb + (long long)k * f->axis_stride;
          double hr, hi = 0.0;
          if (f->kind == 1) ld(filter, f32, o, &hr, &hi);
          else hr = f32 ? ((const float *)filter)[o] : ((const double *)filter)[o];
          const double xr = line[2 * k], xi = line[2 * k + 1];
          line[2 * k] = xr * hr - xi * hi;
          line[2 * k + 1] = xr * hi + xi * hr;
          if (inv) line[2 * k + 1] = -line[2 * k + 1]; /* conjugated: the inverse as conj(F(conj(.))) */
        }
        if (inv) orc_fft_execute(pl, line, 1, 0, 1, scr);
        for (int k = 0; k < n; k++)
          st(dst, f32, ib + (long long)k * d->in_axis_stride, line[2 * k] * d->scale, (inv ? -line[2 * k + 1] : line[2 * k + 1]) * d->scale);
      }
  free(line); free(scr); orc_fft_plan_destroy(pl);
  return 0;
}

static int spec_filt_pass_fwd(const offt_pass_desc *d, const offt_filter_desc *f, const void *filter, void *data, void *stream) {
  (void)stream;
  note(K_FILT_FWD, d, 1);
  return filt_lines(d, f, filter, data, data, 0);
}
static int spec_filt_pass_inv(const offt_pass_desc *d, const offt_filter_desc *f, const void *filter, const void *src, void *dst, void *stream) {
  (void)stream;
  note(K_FILT_INV, d, src == dst);
  return filt_lines(d, f, filter, src, dst, 1);
}

/* the logging entries over the chain below; the two new entries stay NULL (what every older backend looks like) */
static void make(offt_backend *t) {
  g_base = *cpu_backend_multi_table();
  *t = g_base;
  t->pass = spec_pass;
  t->pointwise = spec_pointwise;
  t->pointwise_oop = spec_pointwise_oop;
  t->memcpy_dd = spec_memcpy_dd;
  t->zero_outside = spec_zero_outside;
  t->filt_pass_fwd = NULL;
  t->filt_pass_inv = NULL;
}
const offt_backend *cpu_backend_spec_table(void) {
  make(&g_full);
  g_full.filt_pass_fwd = spec_filt_pass_fwd;
  g_full.filt_pass_inv = spec_filt_pass_inv;
  return &g_full;
}
/* a table from before the two entries: the generic route, with the out-of-place multiply */
const offt_backend *cpu_backend_spec_table_nofilt(void) { make(&g_nofilt); return &g_nofilt; }
/* ... and from before pointwise_oop as well: copy, then multiply in place */
const offt_backend *cpu_backend_spec_table_old(void) { make(&g_old); g_old.pointwise_oop = NULL; return &g_old; }
/* no multiply at all: both calls are refused */
const offt_backend *cpu_backend_spec_table_none(void) { return cpu_backend_conv_table_none(); }
long cpu_backend_spec_count(int kind) { return kind >= 0 && kind < K_COUNT ? g_count[kind] : -1; }
void cpu_backend_spec_log_reset(void) { g_nlog = 0; }
int cpu_backend_spec_log_len(void) { return g_nlog; }
int cpu_backend_spec_log(int i, int *rec9) {
  if (i < 0 || i >= g_nlog) return -1;
  memcpy(rec9, g_log[i], sizeof g_log[i]);
  return 0;
}
