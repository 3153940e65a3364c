/*
 * cpu_backend_padreal_mixed.c -- TEST INFRASTRUCTURE ONLY.
 *
 * The padreal backend of cpu_backend_padreal.c with bit 4 of offt_pass_desc::half understood, so that real-input half-box
 * plans with a mixed-radix z length and OFFT_HIP_OPT_HALF_R2C_MIXED set run their pruned route on the CPU.  Bit 4 is a
 * permission on the two real forms ("real rows may run on a mixed-radix half-line kernel") and changes nothing a pass
 * computes: a real descriptor with half = 5 or 6 is handed on with the bit masked, i.e. as half = 1 or 2, and the padreal
 * backend never dereferences the padding of such a pass.  The bit anywhere else -- on a complex descriptor, or without bit
 * 1 or 2 -- is refused (-1), as the kernel launcher refuses it.  Every other descriptor goes on as it is.  The launch log
 * kept here records what the HOST sent (half = 5 / 6 included) and sees every launch, the refused included.
 * Built into tests/libcpubackend_padreal_mixed.so, never into the library.
 */
#include <string.h>
#include "offt_backend.h"

const offt_backend *cpu_backend_padreal_table(void);
const offt_backend *cpu_backend_padreal_table_unfused(void);

static offt_backend g_table;
static offt_backend g_inner;

/* ring of the last launches: n, ncols, nb1, nb2, half, 0 = pass / 1 = conv_pass, real_input */
#define LOG_MAX 64
static int g_log[LOG_MAX][7], g_nlog = 0;
static void log_launch(const offt_pass_desc *d, int conv) {
  if (g_nlog < LOG_MAX) {
    int *r = g_log[g_nlog++];
    r[0] = d->n; r[1] = d->ncols; r[2] = d->nb1; r[3] = d->nb2; r[4] = d->half; r[5] = conv; r[6] = d->real_input;
  }
}

static int mixed_pass(const offt_pass_desc *d, const void *in, void *out, void *stream) {
  log_launch(d, 0);
  if (!(d->half & 4)) return g_inner.pass(d, in, out, stream);
  if (!d->real_input || (d->half & ~7) || !(d->half & 3)) return -1;
  offt_pass_desc m = *d;
  m.half &= 3;
  return g_inner.pass(&m, in, out, stream);
}

static int mixed_conv_pass(const offt_pass_desc *d, const offt_filter_desc *f, const void *filter, void *data, void *stream) {
  log_launch(d, 1);
  return g_inner.conv_pass(d, f, filter, data, stream);
}

/* (the backends below keep ONE table each: copy it before asking for its next form) */
static const offt_backend *make(const offt_backend *inner) {
  g_inner = *inner;
  g_table = g_inner;
  g_table.pass = mixed_pass;
  g_table.conv_pass = g_inner.conv_pass ? mixed_conv_pass : NULL;
  return &g_table;
}
const offt_backend *cpu_backend_padreal_mixed_table(void) { return make(cpu_backend_padreal_table()); }
/* the same without the fused launch: every convolve takes the unfused route */
const offt_backend *cpu_backend_padreal_mixed_table_unfused(void) { return make(cpu_backend_padreal_table_unfused()); }
void cpu_backend_padreal_mixed_log_reset(void) { g_nlog = 0; }
int cpu_backend_padreal_mixed_log(int i, int *rec7) {
  if (i < 0 || i >= g_nlog) return -1;
  memcpy(rec7, g_log[i], sizeof g_log[i]);
  return 0;
}
