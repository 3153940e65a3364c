/*
 * cpu_backend_padreal.c -- TEST INFRASTRUCTURE ONLY.
 *
 * The pad backend of cpu_backend_pad.c with the two real ends of a half-box chain interpreted as well, so that real-input
 * half-box plans with OFFT_HIP_OPT_HALF_R2C set run their pruned route on the CPU:
 *   real_input = 1 with half = 1, contiguous in / strided out: reads the reals n < n/2 of a row, stores n/2+1 complex values;
 *   real_input = 2 with half = 2, strided in / contiguous out: reads n/2+1 complex values, stores the reals n < n/2 of a row.
 * It never dereferences real input indices >= n/2, real output indices >= n/2 or complex outputs above n/2: the tests fill
 * the padding with NaN, and a read of it would show.  Every other real form with a half bit is refused (-1), every other
 * descriptor goes to cpu_backend_pad.c.  It keeps a launch log of its own, which sees every launch, the refused included.
 * Built into tests/libcpubackend_padreal.so, never into the library.
 */
#include <stdlib.h>
#include <string.h>
#include "offt_backend.h"
#include "oracle.h"

const offt_backend *cpu_backend_pad_table(void);

static offt_backend g_table;
static const offt_backend *g_pad;
static long g_real_half_count = 0;

/* ring of the last launches: n, ncols, nb1, nb2, half, 0 = pass / 1 = conv_pass, real_input */
#define LOG_MAX 64
static int g_log[LOG_MAX][7], g_nlog = 0;
static void log_launch(const offt_pass_desc *d, int conv) {
  if (g_nlog < LOG_MAX) {
    int *r = g_log[g_nlog++];
    r[0] = d->n; r[1] = d->ncols; r[2] = d->nb1; r[3] = d->nb2; r[4] = d->half; r[5] = conv; r[6] = d->real_input;
  }
}

static int real_half_pass(const offt_pass_desc *d, const void *in, void *out) {
  const int r2c = d->real_input == 1 && d->half == 1 && d->in_contig && !d->out_contig && d->in_axis_stride == 1 && d->direction <= 0;
  const int c2r = d->real_input == 2 && d->half == 2 && !d->in_contig && d->out_contig && d->out_axis_stride == 1;
  g_real_half_count++;
  if (!r2c && !c2r) return -1;
  if ((d->n & 1) || d->tw4 || d->in_split || d->in_split_nfloor || d->out_split || d->out_split_nfloor) return -1;
  if (d->ncols < 1 || d->nb1 < 1 || d->nb2 < 1) return 0;
  const int n = d->n, f32 = d->precision == OFFT_PREC_F32;
  orc_fft_plan *pl = orc_fft_plan_create(n);
  double *line = (double *)malloc(sizeof(double) * 2 * (size_t)n), *scr = (double *)malloc(sizeof(double) * 6 * (size_t)n + 64);
  for (int b2 = 0; b2 < d->nb2; b2++)
    for (int b1 = 0; b1 < d->nb1; b1++)
      for (int c = 0; c < d->ncols; c++) {
        const long long ib = (long long)b1 * d->in_b1_stride + (long long)b2 * d->in_b2_stride + (long long)c * d->in_col_stride;
        const long long ob = (long long)b1 * d->out_b1_stride + (long long)b2 * d->out_b2_stride + (long long)c * d->out_col_stride;
        memset(line, 0, sizeof(double) * 2 * (size_t)n);
        if (r2c) {
          for (int k = 0; k < n / 2; k++) line[2 * k] = f32 ? ((const float *)in)[2 * ib + k] : ((const double *)in)[2 * ib + k];
          orc_fft_execute(pl, line, 1, 0, 1, scr);
          for (int k = 0; k <= n / 2; k++) {
            const long long o = ob + (long long)k * d->out_axis_stride;
            const double re = line[2 * k] * d->scale, im = line[2 * k + 1] * d->scale;
            if (f32) { ((float *)out)[2 * o] = (float)re; ((float *)out)[2 * o + 1] = (float)im; }
            else { ((double *)out)[2 * o] = re; ((double *)out)[2 * o + 1] = im; }
          }
        } else {
          for (int k = 0; k < n; k++) {
            const int m = k <= n / 2 ? k : n - k;
            const long long o = ib + (long long)m * d->in_axis_stride;
            double re, im;
            if (f32) { re = ((const float *)in)[2 * o]; im = ((const float *)in)[2 * o + 1]; }
            else { re = ((const double *)in)[2 * o]; im = ((const double *)in)[2 * o + 1]; }
            if (k > n / 2) im = -im;
            line[2 * k] = re; line[2 * k + 1] = -im; /* inverse = conj(F(conj(.))) */
          }
          orc_fft_execute(pl, line, 1, 0, 1, scr);
          for (int k = 0; k < n / 2; k++) {
            if (f32) ((float *)out)[2 * ob + k] = (float)(line[2 * k] * d->scale);
            else ((double *)out)[2 * ob + k] = line[2 * k] * d->scale;
          }
        }
      }
  free(line); free(scr); orc_fft_plan_destroy(pl);
  return 0;
}

static int padreal_pass(const offt_pass_desc *d, const void *in, void *out, void *stream) {
  log_launch(d, 0);
  if (d->half && d->real_input) return real_half_pass(d, in, out);
  return g_pad->pass(d, in, out, stream);
}

static int padreal_conv_pass(const offt_pass_desc *d, const offt_filter_desc *f, const void *filter, void *data, void *stream) {
  log_launch(d, 1);
  return g_pad->conv_pass(d, f, filter, data, stream);
}

/* (cpu_backend_pad.c keeps ONE table: copy it before asking for its next form) */
static const offt_backend *make(const offt_backend *pad) {
  static offt_backend pad_copy;
  pad_copy = *pad;
  g_pad = &pad_copy;
  g_table = pad_copy;
  g_table.pass = padreal_pass;
  g_table.conv_pass = padreal_conv_pass;
  return &g_table;
}
const offt_backend *cpu_backend_padreal_table(void) { return make(cpu_backend_pad_table()); }
/* the same without the fused launch: every convolve takes the unfused route */
const offt_backend *cpu_backend_padreal_table_unfused(void) {
  make(cpu_backend_pad_table());
  g_table.conv_pass = NULL;
  return &g_table;
}
long cpu_backend_padreal_real_half_count(void) { return g_real_half_count; }
void cpu_backend_padreal_log_reset(void) { g_nlog = 0; }
int cpu_backend_padreal_log(int i, int *rec7) {
  if (i < 0 || i >= g_nlog) return -1;
  memcpy(rec7, g_log[i], sizeof g_log[i]);
  return 0;
}
