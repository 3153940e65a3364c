/*
 * cpu_backend_prod.c -- TEST INFRASTRUCTURE ONLY.
 *
 * The CPU backend chain (cpu_backend.c, _conv.c, _pad.c, _padreal.c) with the two entries of the pseudo-spectral product
 * filled: prod_pass (the fused launch: inverse z pass of one or two sources, their product, forward z pass) and
 * pointwise_prod (the multiply sweep of the generic route).  Both read a line / an element from every source before they
 * store it, so the destination may be either source.  Every entry the call uses is logged (kind, n, direction, ncols, nb1,
 * half, real_input, sources), so that the tests can read the route off the launches.
 * Built into tests/libcpubackend_prod.so (tests/test_product.py), never into the library.
 */
#include <stdlib.h>
#include <string.h>
#include "offt_backend.h"
#include "oracle.h"

const offt_backend *cpu_backend_padreal_table(void);

static offt_backend g_base;                    /* the chain below this file: what the logging entries call */
static offt_backend g_full, g_nofused, g_old;  /* one static per table: asking for one never changes another that is installed */

enum { K_PASS = 0, K_PROD = 1, K_POINTWISE_PROD = 2, K_ZERO = 3, K_COUNT = 4 };
static long g_count[K_COUNT];
#define LOG_MAX 512
#define REC 8
static int g_log[LOG_MAX][REC], g_nlog = 0;
static void note(int kind, const offt_pass_desc *d, int nsrc) {
  g_count[kind]++;
  if (g_nlog < LOG_MAX) {
    int *r = g_log[g_nlog++];
    memset(r, 0, sizeof g_log[0]);
    r[0] = kind;
    if (d) { r[1] = d->n; r[2] = d->direction; r[3] = d->ncols; r[4] = d->nb1; r[5] = d->half; r[6] = d->real_input; }
    r[7] = nsrc;
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

static int prod_pass_log(const offt_pass_desc *d, const void *in, void *out, void *stream) {
  note(K_PASS, d, 0);
  return g_base.pass(d, in, out, stream);
}
static int prod_zero_outside(void *buf, int precision, int n0, int n1, int n2, int k0, int k1, int k2, long long s0, long long s1, long long s2,
                             void *stream) {
  note(K_ZERO, NULL, 0);
  return g_base.zero_outside(buf, precision, n0, n1, n2, k0, k1, k2, s0, s1, s2, stream);
}

/* offt_hipk_prod_pass on host memory: per line, each source through the in_* side, the unnormalised inverse DFT (as
 * conj(F(conj(.)))), the product of the two (the square of the one), the forward DFT, scale, stored at the same offsets
 * of `dst` */
static int prod_prod_pass(const offt_pass_desc *d, const void *src0, const void *src1, void *dst, void *stream) {
  (void)stream;
  note(K_PROD, d, src1 && src1 != src0 ? 2 : 1);
  if (!src0 || !dst) return -1;
  if (d->half || d->real_input || d->in_split || d->in_split_nfloor || d->tw4) return -1;
  if (d->n < 1 || d->ncols < 1 || d->nb1 < 1 || d->nb2 < 1) return 0;
  const int n = d->n, f32 = d->precision == OFFT_PREC_F32, two = src1 && src1 != src0;
  orc_fft_plan *pl = orc_fft_plan_create(n);
  double *la = (double *)malloc(sizeof(double) * 2 * (size_t)n), *lb = (double *)malloc(sizeof(double) * 2 * (size_t)n),
         *scr = (double *)malloc(sizeof(double) * 6 * (size_t)n + 64);
  for (int b2 = 0; b2 < d->nb2; b2++)
    for (int b1 = 0; b1 < d->nb1; b1++)
      for (int c = 0; c < d->ncols; c++) {
        const long long ib = (long long)b1 * d->in_b1_stride + (long long)b2 * d->in_b2_stride + (long long)c * d->in_col_stride;
        for (int i = 0; i < n; i++) {
          ld(src0, f32, ib + (long long)i * d->in_axis_stride, &la[2 * i], &la[2 * i + 1]);
          la[2 * i + 1] = -la[2 * i + 1];
        }
        orc_fft_execute(pl, la, 1, 0, 1, scr); /* la = conj(inverse of source 0) */
        if (two) {
          for (int i = 0; i < n; i++) {
            ld(src1, f32, ib + (long long)i * d->in_axis_stride, &lb[2 * i], &lb[2 * i + 1]);
            lb[2 * i + 1] = -lb[2 * i + 1];
          }
          orc_fft_execute(pl, lb, 1, 0, 1, scr);
        } else memcpy(lb, la, sizeof(double) * 2 * (size_t)n);
        for (int i = 0; i < n; i++) { /* conj(la) conj(lb): the product of the two fields */
          const double ar = la[2 * i], ai = -la[2 * i + 1], br = lb[2 * i], bi = -lb[2 * i + 1];
          la[2 * i] = ar * br - ai * bi;
          la[2 * i + 1] = ar * bi + ai * br;
        }
        orc_fft_execute(pl, la, 1, 0, 1, scr);
        for (int i = 0; i < n; i++) st(dst, f32, ib + (long long)i * d->in_axis_stride, la[2 * i] * d->scale, la[2 * i + 1] * d->scale);
      }
  free(la); free(lb); free(scr); orc_fft_plan_destroy(pl);
  return 0;
}

/* offt_hipk_pointwise_prod on host memory: complex elements, or with OFFT_HIPK_PROD_REAL real scalars */
static int prod_pointwise_prod(const void *x, const void *y, void *out, int precision, int n0, int n1, int n2, long long s0, long long s1,
                               long long s2, void *stream) {
  (void)stream;
  note(K_POINTWISE_PROD, NULL, y && y != x ? 2 : 1);
  if (!x || !out) return -1;
  const int real = (precision & OFFT_HIPK_PROD_REAL) != 0, f32 = (precision & ~OFFT_HIPK_PROD_REAL) == OFFT_PREC_F32;
  if (!y) y = x;
  for (int i0 = 0; i0 < n0; i0++)
    for (int i1 = 0; i1 < n1; i1++)
      for (int i2 = 0; i2 < n2; i2++) {
        const long long o = (long long)i0 * s0 + (long long)i1 * s1 + (long long)i2 * s2;
        if (real) {
          if (f32) ((float *)out)[o] = ((const float *)x)[o] * ((const float *)y)[o];
          else ((double *)out)[o] = ((const double *)x)[o] * ((const double *)y)[o];
        } else {
          double xr, xi, yr, yi;
          ld(x, f32, o, &xr, &xi);
          ld(y, f32, o, &yr, &yi);
          st(out, f32, o, xr * yr - xi * yi, xr * yi + xi * yr);
        }
      }
  return 0;
}

/* the logging entries over the chain below; the two new entries stay NULL (what every older backend looks like to the library) */
static void make(offt_backend *t) {
  g_base = *cpu_backend_padreal_table();
  *t = g_base;
  t->pass = prod_pass_log;
  t->zero_outside = prod_zero_outside;
  t->prod_pass = NULL;
  t->pointwise_prod = NULL;
}
/* neither entry: the call is refused */
const offt_backend *cpu_backend_prod_table_old(void) { make(&g_old); return &g_old; }
const offt_backend *cpu_backend_prod_table(void) {
  make(&g_full);
  g_full.prod_pass = prod_prod_pass;
  g_full.pointwise_prod = prod_pointwise_prod;
  return &g_full;
}
/* the multiply sweep, but no fused launch: no fused route */
const offt_backend *cpu_backend_prod_table_nofused(void) {
  make(&g_nofused);
  g_nofused.pointwise_prod = prod_pointwise_prod;
  return &g_nofused;
}
/* one descriptor on host arrays (descriptor-level parity tests against the HIP kernel) */
int cpu_backend_prod_run(const offt_pass_desc *d, const void *src0, const void *src1, void *dst) { return prod_prod_pass(d, src0, src1, dst, NULL); }
long cpu_backend_prod_count(int kind) { return kind >= 0 && kind < K_COUNT ? g_count[kind] : -1; }
void cpu_backend_prod_log_reset(void) { g_nlog = 0; }
int cpu_backend_prod_log_len(void) { return g_nlog; }
int cpu_backend_prod_log(int i, int *rec8) {
  if (i < 0 || i >= g_nlog) return -1;
  memcpy(rec8, g_log[i], sizeof g_log[i]);
  return 0;
}
