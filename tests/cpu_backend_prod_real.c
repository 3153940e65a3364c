/*
 * cpu_backend_prod_real.c -- TEST INFRASTRUCTURE ONLY.
 *
 * The product backend of cpu_backend_prod.c with prod_pass_real filled: the fused launch of the pseudo-spectral product on
 * a real-input plan, whose lines are half spectra.  It is written from the DEFINITION, one source at a time -- the Hermitian
 * extension of the n/2+1 stored values with the imaginary parts of elements 0 and n/2 dropped, the oracle's inverse DFT, the
 * real part, the product of the two real fields, the oracle's forward DFT, the elements k <= n/2 -- and does NOT pack the two
 * spectra into one transform as the kernel does, so that the two are independent statements of the same thing.
 * Both sources' lines are read before the line of `dst` is stored, so the destination may be either source.
 * Every launch is logged (kind 4, n, direction, ncols, nb1, half, real_input, sources, and how many launches
 * cpu_backend_prod.c had logged before it: its place among the plain passes).
 * Built into tests/libcpubackend_prod_real.so (tests/test_product_real.py), never into the library.
 */
#include <stdlib.h>
#include <string.h>
#include "offt_backend.h"
#include "oracle.h"

const offt_backend *cpu_backend_prod_table(void);
int cpu_backend_prod_log_len(void);

static offt_backend g_real;

enum { K_PROD_REAL = 4 };
#define LOG_MAX 256
#define REC 9
static int g_log[LOG_MAX][REC], g_nlog = 0;
static long g_count = 0;

static double ldr(const void *p, int f32, long long i, int im) {
  return f32 ? (double)((const float *)p)[2 * i + im] : ((const double *)p)[2 * i + im];
}

/* the unnormalised real inverse of the half spectrum at `src` (element k at ib + k * pitch) into fld[n] */
static void real_inverse(const orc_fft_plan *pl, const void *src, int f32, long long ib, long long pitch, int n, double *line, double *scr,
                         double *fld) {
  for (int k = 0; k < n; k++) {
    const int m = k <= n / 2 ? k : n - k;
    double re = ldr(src, f32, ib + (long long)m * pitch, 0), im = ldr(src, f32, ib + (long long)m * pitch, 1);
    if (k > n / 2) im = -im;                     /* conj(X[n - k]) */
    if (k == 0 || 2 * k == n) im = 0.0;          /* real by symmetry: what is stored there has no effect */
    line[2 * k] = re;
    line[2 * k + 1] = -im;                       /* the inverse as conj(F(conj(.))) */
  }
  orc_fft_execute(pl, line, 1, 0, 1, scr);
  for (int k = 0; k < n; k++) fld[k] = line[2 * k]; /* the real part; the imaginary one is rounding */
}

static int prod_real_pass(const offt_pass_desc *d, const void *src0, const void *src1, void *dst, void *stream) {
  (void)stream;
  const int two = src1 && src1 != src0;
  g_count++;
  if (g_nlog < LOG_MAX) {
    int *r = g_log[g_nlog++];
    r[0] = K_PROD_REAL; r[1] = d->n; r[2] = d->direction; r[3] = d->ncols; r[4] = d->nb1; r[5] = d->half; r[6] = d->real_input;
    r[7] = two ? 2 : 1; r[8] = cpu_backend_prod_log_len();
  }
  if (!src0 || !dst) return -1;
  if (d->real_input != 2 || d->half || d->in_contig || d->in_split || d->in_split_nfloor || d->tw4) return -1;
  if (d->n < 2 || (d->n & 1) || d->ncols < 1 || d->nb1 < 1 || d->nb2 < 1) return 0;
  const int n = d->n, f32 = d->precision == OFFT_PREC_F32;
  orc_fft_plan *pl = orc_fft_plan_create(n);
  double *line = (double *)malloc(sizeof(double) * 2 * (size_t)n), *fa = (double *)malloc(sizeof(double) * (size_t)n),
         *fb = (double *)malloc(sizeof(double) * (size_t)n), *scr = (double *)malloc(sizeof(double) * 6 * (size_t)n + 64);
  for (int b2 = 0; b2 < d->nb2; b2++)
    for (int b1 = 0; b1 < d->nb1; b1++)
      for (int c = 0; c < d->ncols; c++) {
        const long long ib = (long long)b1 * d->in_b1_stride + (long long)b2 * d->in_b2_stride + (long long)c * d->in_col_stride;
        real_inverse(pl, src0, f32, ib, d->in_axis_stride, n, line, scr, fa);
        if (two) real_inverse(pl, src1, f32, ib, d->in_axis_stride, n, line, scr, fb);
        for (int k = 0; k < n; k++) {
          line[2 * k] = fa[k] * (two ? fb[k] : fa[k]);
          line[2 * k + 1] = 0.0;
        }
        orc_fft_execute(pl, line, 1, 0, 1, scr);
        for (int k = 0; k <= n / 2; k++) {
          const long long o = ib + (long long)k * d->in_axis_stride;
          if (f32) { ((float *)dst)[2 * o] = (float)(line[2 * k] * d->scale); ((float *)dst)[2 * o + 1] = (float)(line[2 * k + 1] * d->scale); }
          else { ((double *)dst)[2 * o] = line[2 * k] * d->scale; ((double *)dst)[2 * o + 1] = line[2 * k + 1] * d->scale; }
        }
      }
  free(line); free(fa); free(fb); free(scr); orc_fft_plan_destroy(pl);
  return 0;
}

/* the full product table with the real-row launch; cpu_backend_prod_table() itself is the table of a backend older than it */
const offt_backend *cpu_backend_prod_real_table(void) {
  g_real = *cpu_backend_prod_table();
  g_real.prod_pass_real = prod_real_pass;
  return &g_real;
}
/* one descriptor on host arrays */
int cpu_backend_prod_real_run(const offt_pass_desc *d, const void *src0, const void *src1, void *dst) { return prod_real_pass(d, src0, src1, dst, NULL); }
long cpu_backend_prod_real_count(void) { return g_count; }
void cpu_backend_prod_real_log_reset(void) { g_nlog = 0; }
int cpu_backend_prod_real_log(int i, int *rec9) {
  if (i < 0 || i >= g_nlog) return -1;
  memcpy(rec9, g_log[i], sizeof g_log[i]);
  return 0;
}
