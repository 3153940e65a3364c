/*
 * cpu_backend_pipeline.c -- TEST INFRASTRUCTURE ONLY.
 *
 * The CPU backend of cpu_backend.c with the entry of the pipelined plane groups, offt_backend::pass_pair: a backend without
 * workgroups runs the two passes one after the other (y, then x -- they are independent, so the order cannot matter), and
 * a log of every pass and pass_pair the host issues, so that a test can read the schedule
 *   y(0) | {x(0), y(1)} | ... | {x(G-2), y(G-1)} | x(G-1)
 * off it (tests/test_zgroup_pipeline.py).  Built into tests/libcpubackend_pipeline.so, never into the library.
 */
#include <stdlib.h>
#include <string.h>
#include "offt_backend.h"

const offt_backend *cpu_backend_table(void);

/* kind 0: pass (n, nb1, out_keep, out_contig of the descriptor; the second half zero), 1: pass_pair (y, then x) */
typedef struct prec { int kind, n, nb1, out_keep, out_contig, n2, nb1_2, out_keep2; long long out_off, out_off2; } prec;
static offt_backend g_base, g_table;
static prec *g_log = NULL;
static long g_nlog = 0, g_caplog = 0;
static const char *g_origin = NULL; /* offsets in the log are bytes from here (the caller's array) */

static prec *put(void) {
  if (g_nlog == g_caplog) { g_caplog = g_caplog ? 2 * g_caplog : 256; g_log = (prec *)realloc(g_log, (size_t)g_caplog * sizeof(prec)); }
  prec *e = &g_log[g_nlog++];
  memset(e, 0, sizeof *e);
  return e;
}
static int pp_pass(const offt_pass_desc *d, const void *in, void *out, void *stream) {
  prec *e = put();
  e->kind = 0; e->n = d->n; e->nb1 = d->nb1; e->out_keep = d->out_keep; e->out_contig = d->out_contig;
  e->out_off = (long long)((const char *)out - g_origin);
  return g_base.pass(d, in, out, stream);
}
static int pp_pass_pair(const offt_pass_desc *dy, const void *iny, void *outy, const offt_pass_desc *dx, const void *inx, void *outx, void *stream) {
  prec *e = put();
  e->kind = 1; e->n = dy->n; e->nb1 = dy->nb1; e->out_keep = dy->out_keep; e->out_contig = dy->out_contig;
  e->n2 = dx->n; e->nb1_2 = dx->nb1; e->out_keep2 = dx->out_keep;
  e->out_off = (long long)((const char *)outy - g_origin); e->out_off2 = (long long)((const char *)outx - g_origin);
  const int rc = g_base.pass(dy, iny, outy, stream);
  return rc ? rc : g_base.pass(dx, inx, outx, stream);
}

const offt_backend *cpu_backend_pipeline_table(void) {
  g_base = *cpu_backend_table();
  g_table = g_base;
  g_table.pass = pp_pass;
  g_table.pass_pair = pp_pass_pair;
  return &g_table;
}
void cpu_backend_pipeline_reset(const void *origin) { g_nlog = 0; g_origin = (const char *)origin; }
long cpu_backend_pipeline_len(void) { return g_nlog; }
int cpu_backend_pipeline_rec_bytes(void) { return (int)sizeof(prec); }
void cpu_backend_pipeline_copy_log(void *dst) { memcpy(dst, g_log, (size_t)g_nlog * sizeof(prec)); }
