/*
 * cpu_backend_streams.c -- TEST INFRASTRUCTURE ONLY.
 *
 * The CPU backend of cpu_backend_spec.c (the most complete interpreter) with the two entries of the multi-input convolution
 * taken from cpu_backend_sum.c, and with a log of everything the host issues: every launch (pass, the fused convolution and
 * filtered launches, the multiplies, memcpy, zero_outside, a2a, flag signal / wait) WITH ITS STREAM, and every event_record,
 * stream_wait and stream_sync.  Everything still executes synchronously in issue order, so the answers stay checkable; the
 * log is what tests/_stream_graph.py rebuilds happens-before from (tests/test_streams.py).
 * With access recording on (cpu_backend_streams_record_access) every launch also reports the memory it reads and writes,
 * as the addresses of 4-byte granules, worked out from its descriptor: the hazard check needs them.  Filters and twiddle
 * tables are never written by a launch and are left out.  Where a half-line or real-row descriptor touches less than the
 * full line the set is the full line's (a superset: it can only make the hazard check stricter).
 * The log is process-wide and guarded by a mutex; a rank that is a thread names itself with cpu_backend_streams_set_rank.
 * Built into tests/libcpubackend_streams.so, never into the library.
 */
#include <pthread.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "offt_backend.h"

const offt_backend *cpu_backend_spec_table(void);
const offt_backend *cpu_backend_sum_table(void);

enum { S_PASS = 0, S_CONV = 1, S_CONV_OOP = 2, S_CONV_SUM = 3, S_FILT_FWD = 4, S_FILT_INV = 5, S_POINTWISE = 6, S_POINTWISE_OOP = 7,
       S_POINTWISE_SUM = 8, S_MEMCPY = 9, S_ZERO = 10, S_A2A = 11, S_FLAG_SIGNAL = 12, S_FLAG_WAIT = 13,
       S_EVENT_RECORD = 20, S_STREAM_WAIT = 21, S_STREAM_SYNC = 22, S_MARK = 30 };

typedef struct srec {
  int kind, rank;
  unsigned long long stream, event, value; /* event: the event of a record / wait, the flag word of a signal / wait; value: a flag's, a mark's */
  int n, direction, ncols, nb1, half, real_input, out_keep, same;
  long long r_off, r_len, w_off, w_len;    /* the launch's read and write sets inside the granule pool */
} srec;

static offt_backend g_base, g_table;
static pthread_mutex_t g_mu = PTHREAD_MUTEX_INITIALIZER;
static srec *g_log = NULL;
static long g_nlog = 0, g_caplog = 0;
static uint64_t *g_pool = NULL;
static long long g_npool = 0, g_cappool = 0;
static int g_access = 0;
static _Thread_local int g_rank = 0;

typedef struct gset { uint64_t *v; long long n, cap; } gset;
static void gs_add(gset *s, const void *base, long long scalar, int ssz, int nscalars) {
  if (!g_access) return;
  const uint64_t a = ((uint64_t)(uintptr_t)base + (uint64_t)(scalar * ssz)) / 4;
  const int ng = nscalars * ssz / 4;
  if (s->n + ng > s->cap) { s->cap = 2 * s->cap + ng + 1024; s->v = (uint64_t *)realloc(s->v, (size_t)s->cap * sizeof(uint64_t)); }
  for (int i = 0; i < ng; i++) s->v[s->n++] = a + (uint64_t)i;
}
static void gs_bytes(gset *s, const void *base, size_t bytes) {
  if (!g_access) return;
  for (size_t i = 0; i < bytes / 4; i++) gs_add(s, base, (long long)i, 4, 1);
}

/* append one operation; the sets are copied into the pool and freed */
static void put(int kind, void *stream, void *event, unsigned long long value, const offt_pass_desc *d, int same, gset *r, gset *w) {
  pthread_mutex_lock(&g_mu);
  if (g_nlog == g_caplog) { g_caplog = g_caplog ? 2 * g_caplog : 1024; g_log = (srec *)realloc(g_log, (size_t)g_caplog * sizeof(srec)); }
  srec *e = &g_log[g_nlog++];
  memset(e, 0, sizeof *e);
  e->kind = kind; e->rank = g_rank;
  e->stream = (unsigned long long)(uintptr_t)stream; e->event = (unsigned long long)(uintptr_t)event; e->value = value;
  if (d) { e->n = d->n; e->direction = d->direction; e->ncols = d->ncols; e->nb1 = d->nb1; e->half = d->half; e->real_input = d->real_input; e->out_keep = d->out_keep; }
  e->same = same;
  gset *ss[2] = {r, w};
  for (int k = 0; k < 2; k++) {
    const long long n = ss[k] ? ss[k]->n : 0;
    if (g_npool + n > g_cappool) { g_cappool = 2 * g_cappool + n + 4096; g_pool = (uint64_t *)realloc(g_pool, (size_t)g_cappool * sizeof(uint64_t)); }
    if (n) memcpy(g_pool + g_npool, ss[k]->v, (size_t)n * sizeof(uint64_t));
    if (k == 0) { e->r_off = g_npool; e->r_len = n; } else { e->w_off = g_npool; e->w_len = n; }
    g_npool += n;
  }
  pthread_mutex_unlock(&g_mu);
  if (r) free(r->v);
  if (w) free(w->v);
}

static long long split_off(int k, int split, int nfloor, long long blk, long long axis, const long long *tab) {
  if (split == 0 && nfloor == 0) return (long long)k * axis;
  int a, r;
  if (nfloor > 0 && k >= split * nfloor) { int kk = k - split * nfloor; a = nfloor + kk / (split + 1); r = kk % (split + 1); }
  else { a = k / split; r = k % split; }
  return (tab ? tab[a] : (long long)a * blk) + (long long)r * axis;
}

/* the lines of a descriptor's input side (side 0) or output side (side 1), complex elements 0 .. cnt-1 of each */
static void desc_lines(gset *s, const offt_pass_desc *d, const void *base, int side, int cnt) {
  if (!g_access || !base || d->n < 1 || d->ncols < 1 || d->nb1 < 1 || d->nb2 < 1) return;
  const int ssz = d->precision == OFFT_PREC_F32 ? 4 : 8;
  for (int b2 = 0; b2 < d->nb2; b2++)
    for (int b1 = 0; b1 < d->nb1; b1++)
      for (int c = 0; c < d->ncols; c++) {
        const long long lb = side == 0 ? (long long)b1 * d->in_b1_stride + (long long)b2 * d->in_b2_stride + (long long)c * d->in_col_stride
                                       : (long long)b1 * d->out_b1_stride + (long long)b2 * d->out_b2_stride + (long long)c * d->out_col_stride;
        for (int k = 0; k < cnt; k++) {
          const long long o = lb + (side == 0 ? split_off(k, d->in_split, d->in_split_nfloor, d->in_block_stride, d->in_axis_stride, d->in_block_tab)
                                              : split_off(k, d->out_split, d->out_split_nfloor, d->out_block_stride, d->out_axis_stride, d->out_block_tab));
          gs_add(s, base, 2 * o, ssz, 2);
        }
      }
}
/* the n real scalars at the head of every row of a side (real_input 1: the input side, 2: the output side) */
static void desc_real_rows(gset *s, const offt_pass_desc *d, const void *base, int side) {
  if (!g_access || !base || d->n < 1 || d->ncols < 1 || d->nb1 < 1 || d->nb2 < 1) return;
  const int ssz = d->precision == OFFT_PREC_F32 ? 4 : 8;
  for (int b2 = 0; b2 < d->nb2; b2++)
    for (int b1 = 0; b1 < d->nb1; b1++)
      for (int c = 0; c < d->ncols; c++) {
        const long long lb = side == 0 ? (long long)b1 * d->in_b1_stride + (long long)b2 * d->in_b2_stride + (long long)c * d->in_col_stride
                                       : (long long)b1 * d->out_b1_stride + (long long)b2 * d->out_b2_stride + (long long)c * d->out_col_stride;
        gs_add(s, base, 2 * lb, ssz, d->n);
      }
}
static void box(gset *s, const void *base, int precision, int n0, int n1, int n2, long long s0, long long s1, long long s2) {
  if (!g_access || !base) return;
  const int ssz = precision == OFFT_PREC_F32 ? 4 : 8;
  for (int i0 = 0; i0 < n0; i0++)
    for (int i1 = 0; i1 < n1; i1++)
      for (int i2 = 0; i2 < n2; i2++) gs_add(s, base, 2 * ((long long)i0 * s0 + (long long)i1 * s1 + (long long)i2 * s2), ssz, 2);
}

static int st_pass(const offt_pass_desc *d, const void *in, void *out, void *stream) {
  gset r = {0}, w = {0};
  if (d->real_input == 1) desc_real_rows(&r, d, in, 0); else desc_lines(&r, d, in, 0, d->real_input == 2 ? d->n / 2 + 1 : d->n);
  if (d->real_input == 2) desc_real_rows(&w, d, out, 1); else desc_lines(&w, d, out, 1, d->real_input == 1 ? d->n / 2 + 1 : d->n);
  put(S_PASS, stream, NULL, 0, d, in == out, &r, &w);
  return g_base.pass(d, in, out, stream);
}
static int st_conv_pass(const offt_pass_desc *d, const offt_filter_desc *f, const void *filter, void *data, void *stream) {
  gset r = {0}, w = {0};
  desc_lines(&r, d, data, 0, d->n); desc_lines(&w, d, data, 0, d->n);
  put(S_CONV, stream, NULL, 0, d, 1, &r, &w);
  return g_base.conv_pass(d, f, filter, data, stream);
}
static int st_conv_pass_oop(const offt_pass_desc *d, const offt_filter_desc *f, const void *filter, const void *src, void *dst, void *stream) {
  gset r = {0}, w = {0};
  desc_lines(&r, d, src, 0, d->n); desc_lines(&w, d, dst, 0, d->n);
  put(S_CONV_OOP, stream, NULL, 0, d, src == dst, &r, &w);
  return g_base.conv_pass_oop(d, f, filter, src, dst, stream);
}
static int st_conv_pass_sum(const offt_pass_desc *d, const offt_filter_desc *f, int nin, const void *const *filters, const void *const *srcs,
                            void *dst, void *stream) {
  gset r = {0}, w = {0};
  for (int k = 0; k < nin && srcs; k++) desc_lines(&r, d, srcs[k], 0, d->n);
  desc_lines(&w, d, dst, 0, d->n);
  put(S_CONV_SUM, stream, NULL, (unsigned long long)nin, d, 0, &r, &w);
  return g_base.conv_pass_sum(d, f, nin, filters, srcs, dst, stream);
}
static int st_filt_pass_fwd(const offt_pass_desc *d, const offt_filter_desc *f, const void *filter, void *data, void *stream) {
  gset r = {0}, w = {0};
  desc_lines(&r, d, data, 0, d->n); desc_lines(&w, d, data, 0, d->n);
  put(S_FILT_FWD, stream, NULL, 0, d, 1, &r, &w);
  return g_base.filt_pass_fwd(d, f, filter, data, stream);
}
static int st_filt_pass_inv(const offt_pass_desc *d, const offt_filter_desc *f, const void *filter, const void *src, void *dst, void *stream) {
  gset r = {0}, w = {0};
  desc_lines(&r, d, src, 0, d->n); desc_lines(&w, d, dst, 0, d->n);
  put(S_FILT_INV, stream, NULL, 0, d, src == dst, &r, &w);
  return g_base.filt_pass_inv(d, f, filter, src, dst, stream);
}
static int st_pointwise(void *data, const void *filter, int precision, int kind, int n0, int n1, int n2, long long s0, long long s1, long long s2,
                        void *stream) {
  gset r = {0}, w = {0};
  box(&r, data, precision, n0, n1, n2, s0, s1, s2); box(&w, data, precision, n0, n1, n2, s0, s1, s2);
  put(S_POINTWISE, stream, NULL, 0, NULL, 1, &r, &w);
  return g_base.pointwise(data, filter, precision, kind, n0, n1, n2, s0, s1, s2, stream);
}
static int st_pointwise_oop(const void *in, void *out, const void *filter, int precision, int kind, int n0, int n1, int n2, long long s0,
                            long long s1, long long s2, void *stream) {
  gset r = {0}, w = {0};
  box(&r, in, precision, n0, n1, n2, s0, s1, s2); box(&w, out, precision, n0, n1, n2, s0, s1, s2);
  put(S_POINTWISE_OOP, stream, NULL, 0, NULL, 0, &r, &w);
  return g_base.pointwise_oop(in, out, filter, precision, kind, n0, n1, n2, s0, s1, s2, stream);
}
static int st_pointwise_sum(int nin, const void *const *ins, const void *const *filters, void *out, int precision, int kind, int n0, int n1,
                            int n2, long long s0, long long s1, long long s2, void *stream) {
  gset r = {0}, w = {0};
  for (int k = 0; k < nin && ins; k++) box(&r, ins[k], precision, n0, n1, n2, s0, s1, s2);
  box(&w, out, precision, n0, n1, n2, s0, s1, s2);
  put(S_POINTWISE_SUM, stream, NULL, (unsigned long long)nin, NULL, 0, &r, &w);
  return g_base.pointwise_sum(nin, ins, filters, out, precision, kind, n0, n1, n2, s0, s1, s2, stream);
}
static int st_memcpy_dd(void *dst, const void *src, size_t bytes, void *stream) {
  gset r = {0}, w = {0};
  gs_bytes(&r, src, bytes); gs_bytes(&w, dst, bytes);
  put(S_MEMCPY, stream, NULL, 0, NULL, 0, &r, &w);
  return g_base.memcpy_dd(dst, src, bytes, stream);
}
static int st_zero_outside(void *buf, int precision, int n0, int n1, int n2, int k0, int k1, int k2, long long s0, long long s1, long long s2,
                           void *stream) {
  gset w = {0};
  const int real = (precision & OFFT_HIPK_ZERO_REAL) != 0, ssz = (precision & ~OFFT_HIPK_ZERO_REAL) == OFFT_PREC_F32 ? 4 : 8;
  for (int i0 = 0; i0 < n0 && g_access; i0++)
    for (int i1 = 0; i1 < n1; i1++)
      for (int i2 = (i0 < k0 && i1 < k1) ? k2 : 0; i2 < n2; i2++) {
        const long long o = (long long)i0 * s0 + (long long)i1 * s1 + (long long)i2 * s2;
        gs_add(&w, buf, real ? o : 2 * o, ssz, real ? 1 : 2);
      }
  put(S_ZERO, stream, NULL, 0, NULL, 0, NULL, &w);
  return g_base.zero_outside(buf, precision, n0, n1, n2, k0, k1, k2, s0, s1, s2, stream);
}
static int st_a2a(void *ctx, int which, int npeers, const int *peer, const void *const *sendp, const size_t *sendbytes, void *const *recvp,
                  const size_t *recvbytes, void *stream) {
  gset r = {0}, w = {0};
  for (int a = 0; a < npeers; a++) { gs_bytes(&r, sendp[a], sendbytes[a]); gs_bytes(&w, recvp[a], recvbytes[a]); }
  put(S_A2A, stream, NULL, (unsigned long long)which, NULL, 0, &r, &w);
  return g_base.a2a(ctx, which, npeers, peer, sendp, sendbytes, recvp, recvbytes, stream);
}
/* one log line per flag word; a wait is logged once it has come back, so that the signal it saw stands ahead of it */
static int st_flag_signal(int n, unsigned long long *const *addr, unsigned long long value, void *stream) {
  for (int i = 0; i < n; i++) put(S_FLAG_SIGNAL, stream, (void *)addr[i], value, NULL, 0, NULL, NULL);
  return g_base.flag_signal(n, addr, value, stream);
}
static int st_flag_wait(int n, unsigned long long *const *addr, unsigned long long value, unsigned long long *status, double timeout_s, void *stream) {
  const int rc = g_base.flag_wait(n, addr, value, status, timeout_s, stream);
  for (int i = 0; i < n; i++) put(S_FLAG_WAIT, stream, (void *)addr[i], value, NULL, 0, NULL, NULL);
  return rc;
}
static int st_event_record(void *e, void *s) { put(S_EVENT_RECORD, s, e, 0, NULL, 0, NULL, NULL); return g_base.event_record(e, s); }
static int st_stream_wait(void *s, void *e) { put(S_STREAM_WAIT, s, e, 0, NULL, 0, NULL, NULL); return g_base.stream_wait(s, e); }
static int st_stream_sync(void *s) { put(S_STREAM_SYNC, s, NULL, 0, NULL, 0, NULL, NULL); return g_base.stream_sync(s); }

const offt_backend *cpu_backend_streams_table(void) {
  const offt_backend *sum = cpu_backend_sum_table();
  g_base = *cpu_backend_spec_table();
  g_base.conv_pass_sum = sum->conv_pass_sum;
  g_base.pointwise_sum = sum->pointwise_sum;
  g_table = g_base;
  g_table.pass = st_pass;
  g_table.conv_pass = st_conv_pass;
  g_table.conv_pass_oop = st_conv_pass_oop;
  g_table.conv_pass_sum = st_conv_pass_sum;
  g_table.filt_pass_fwd = st_filt_pass_fwd;
  g_table.filt_pass_inv = st_filt_pass_inv;
  g_table.pointwise = st_pointwise;
  g_table.pointwise_oop = st_pointwise_oop;
  g_table.pointwise_sum = st_pointwise_sum;
  g_table.memcpy_dd = st_memcpy_dd;
  g_table.zero_outside = st_zero_outside;
  g_table.a2a = st_a2a;
  g_table.flag_signal = st_flag_signal;
  g_table.flag_wait = st_flag_wait;
  g_table.event_record = st_event_record;
  g_table.stream_wait = st_stream_wait;
  g_table.stream_sync = st_stream_sync;
  return &g_table;
}
/* a stream of the caller's (what a test hands to offt_hip_set_stream) */
void *cpu_backend_streams_new_stream(void) { return g_base.stream_create ? g_base.stream_create() : malloc(8); }
void cpu_backend_streams_free_stream(void *s) { free(s); }
/* a mark on a stream: where the caller's stream stands (value 1: a call is entered, 2: it has returned) */
void cpu_backend_streams_mark(void *stream, unsigned long long value) { put(S_MARK, stream, NULL, value, NULL, 0, NULL, NULL); }
void cpu_backend_streams_set_rank(int rank) { g_rank = rank; }
void cpu_backend_streams_record_access(int on) { g_access = on; }
void cpu_backend_streams_reset(void) {
  pthread_mutex_lock(&g_mu);
  g_nlog = 0; g_npool = 0;
  pthread_mutex_unlock(&g_mu);
}
long cpu_backend_streams_len(void) { return g_nlog; }
int cpu_backend_streams_rec_bytes(void) { return (int)sizeof(srec); }
/* copy the whole log (cpu_backend_streams_len records of cpu_backend_streams_rec_bytes bytes each) */
void cpu_backend_streams_copy_log(void *dst) { memcpy(dst, g_log, (size_t)g_nlog * sizeof(srec)); }
/* copy `len` granule addresses from offset `off` of the pool (the r_off / w_off of a record) */
void cpu_backend_streams_copy_access(long long off, long long len, unsigned long long *dst) {
  memcpy(dst, g_pool + off, (size_t)len * sizeof(uint64_t));
}
