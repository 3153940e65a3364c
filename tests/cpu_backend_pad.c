/*
 * cpu_backend_pad.c -- TEST INFRASTRUCTURE ONLY.
 *
 * The CPU convolution backend of cpu_backend_conv.c with zero-padded half lines (offt_pass_desc::half) interpreted and the
 * zero_outside entry of offt_backend filled, so that half-box plans (offt_hip_set_half_box) run on the CPU on both of
 * their routes.  A pass with half bit 1 never dereferences input indices >= n/2, one with bit 2 never dereferences output
 * indices >= n/2, the fused launch with half = 3 touches the lower half of its lines only: the tests fill the padding with
 * NaN, and a read of it would show.  It records the batch counts of the last launches for the schedule assertions.  Every
 * other descriptor goes to cpu_backend_conv.c.  Built into tests/libcpubackend_pad.so, never into the library.
 */
#include <stdlib.h>
#include <string.h>
#include "offt_backend.h"
#include "oracle.h"

const offt_backend *cpu_backend_conv_table(void);

static offt_backend g_table;
static const offt_backend *g_conv;
static long g_zero_count = 0, g_half_count = 0;

/* ring of the last launches: n, ncols, nb1, nb2, half, 0 = pass / 1 = conv_pass */
#define LOG_MAX 64
static int g_log[LOG_MAX][6], g_nlog = 0;
static void log_launch(const offt_pass_desc *d, int conv) {
  if (g_nlog < LOG_MAX) {
    int *r = g_log[g_nlog++];
    r[0] = d->n; r[1] = d->ncols; r[2] = d->nb1; r[3] = d->nb2; r[4] = d->half; r[5] = conv;
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

static int pad_pass(const offt_pass_desc *d, const void *in, void *out, void *stream) {
  log_launch(d, 0);
  if (!d->half) return g_conv->pass(d, in, out, stream);
  g_half_count++;
  if (d->n < 1 || d->ncols < 1 || d->nb1 < 1 || d->nb2 < 1) return 0;
  if ((d->n & 1) || d->real_input || d->in_split || d->in_split_nfloor || d->out_split || d->out_split_nfloor || d->half > 2) return -1;
  const int n = d->n, f32 = d->precision == OFFT_PREC_F32;
  const int nin = (d->half & 1) ? n / 2 : n, nout = (d->half & 2) ? n / 2 : n;
  orc_fft_plan *pl = orc_fft_plan_create(n);
  double *line = (double *)malloc(sizeof(double) * 2 * (size_t)n), *scr = (double *)malloc(sizeof(double) * 6 * (size_t)n + 64);
  for (int b2 = 0; b2 < d->nb2; b2++)
    for (int b1 = 0; b1 < d->nb1; b1++)
      for (int c = 0; c < d->ncols; c++) {
        const long long ib = (long long)b1 * d->in_b1_stride + (long long)b2 * d->in_b2_stride + (long long)c * d->in_col_stride;
        const long long ob = (long long)b1 * d->out_b1_stride + (long long)b2 * d->out_b2_stride + (long long)c * d->out_col_stride;
        memset(line, 0, sizeof(double) * 2 * (size_t)n);
        for (int k = 0; k < nin; k++) {
          ld(in, f32, ib + (long long)k * d->in_axis_stride, &line[2 * k], &line[2 * k + 1]);
          if (d->direction > 0) line[2 * k + 1] = -line[2 * k + 1];
        }
        orc_fft_execute(pl, line, 1, 0, 1, scr);
        for (int k = 0; k < nout; k++)
          st(out, f32, ob + (long long)k * d->out_axis_stride, line[2 * k] * d->scale,
             (d->direction > 0 ? -line[2 * k + 1] : line[2 * k + 1]) * d->scale);
      }
  free(line); free(scr); orc_fft_plan_destroy(pl);
  return 0;
}

static int pad_conv_pass(const offt_pass_desc *d, const offt_filter_desc *f, const void *filter, void *data, void *stream) {
  log_launch(d, 1);
  if (!d->half) return g_conv->conv_pass(d, f, filter, data, stream);
  g_half_count++;
  if (d->half != 3 || (d->n & 1) || d->real_input || d->in_split || d->in_split_nfloor || (f->kind != 0 && f->kind != 1)) return -1;
  if (d->ncols < 1 || d->nb1 < 1 || d->nb2 < 1) return 0;
  const int n = d->n, f32 = d->precision == OFFT_PREC_F32;
  orc_fft_plan *pl = orc_fft_plan_create(n);
  double *line = (double *)malloc(sizeof(double) * 2 * (size_t)n), *scr = (double *)malloc(sizeof(double) * 6 * (size_t)n + 64);
  for (int b2 = 0; b2 < d->nb2; b2++)
    for (int b1 = 0; b1 < d->nb1; b1++)
      for (int c = 0; c < d->ncols; c++) {
        const long long ib = (long long)b1 * d->in_b1_stride + (long long)b2 * d->in_b2_stride + (long long)c * d->in_col_stride;
        const long long fb = (long long)b1 * f->b1_stride + (long long)b2 * f->b2_stride + (long long)c * f->col_stride;
        memset(line, 0, sizeof(double) * 2 * (size_t)n);
        for (int k = 0; k < n / 2; k++) ld(data, f32, ib + (long long)k * d->in_axis_stride, &line[2 * k], &line[2 * k + 1]);
        orc_fft_execute(pl, line, 1, 0, 1, scr);
        for (int k = 0; k < n; k++) {
          const long long o = fb + (long long)k * f->axis_stride;
          double hr, hi = 0.0;
          if (f->kind == 1) ld(filter, f32, o, &hr, &hi);
          else hr = f32 ? ((const float *)filter)[o] : ((const double *)filter)[o];
          const double xr = line[2 * k], xi = line[2 * k + 1];
          line[2 * k] = xr * hr - xi * hi;
          line[2 * k + 1] = -(xr * hi + xi * hr);
        }
        orc_fft_execute(pl, line, 1, 0, 1, scr);
        for (int k = 0; k < n / 2; k++)
          st(data, f32, ib + (long long)k * d->in_axis_stride, line[2 * k] * d->scale, -line[2 * k + 1] * d->scale);
      }
  free(line); free(scr); orc_fft_plan_destroy(pl);
  return 0;
}

/* offt_hipk_zero_outside on host memory */
static int pad_zero_outside(void *buf, int precision, int n0, int n1, int n2, int k0, int k1, int k2, long long s0, long long s1,
                            long long s2, void *stream) {
  (void)stream;
  g_zero_count++;
  const int real = (precision & OFFT_HIPK_ZERO_REAL) != 0, f32 = (precision & ~OFFT_HIPK_ZERO_REAL) == OFFT_PREC_F32;
  const size_t esz = (f32 ? 4 : 8) * (real ? 1 : 2);
  if (k0 < 0 || k1 < 0 || k2 < 0 || k0 > n0 || k1 > n1 || k2 > n2) return -1;
  for (int i0 = 0; i0 < n0; i0++)
    for (int i1 = 0; i1 < n1; i1++)
      for (int i2 = (i0 < k0 && i1 < k1) ? k2 : 0; i2 < n2; i2++)
        memset((char *)buf + (size_t)((long long)i0 * s0 + (long long)i1 * s1 + (long long)i2 * s2) * esz, 0, esz);
  return 0;
}

const offt_backend *cpu_backend_pad_table(void) {
  g_conv = cpu_backend_conv_table();
  g_table = *g_conv;
  g_table.pass = pad_pass;
  g_table.conv_pass = pad_conv_pass;
  g_table.zero_outside = pad_zero_outside;
  return &g_table;
}
/* the same without the fused launch: every convolve takes the unfused route */
const offt_backend *cpu_backend_pad_table_unfused(void) {
  cpu_backend_pad_table();
  g_table.conv_pass = NULL;
  return &g_table;
}
/* ... and without zero_outside: half-box is refused */
const offt_backend *cpu_backend_pad_table_nozero(void) {
  cpu_backend_pad_table();
  g_table.zero_outside = NULL;
  return &g_table;
}
long cpu_backend_pad_zero_count(void) { return g_zero_count; }
long cpu_backend_pad_half_count(void) { return g_half_count; }
void cpu_backend_pad_log_reset(void) { g_nlog = 0; }
int cpu_backend_pad_log(int i, int *rec6) {
  if (i < 0 || i >= g_nlog) return -1;
  memcpy(rec6, g_log[i], sizeof g_log[i]);
  return 0;
}
