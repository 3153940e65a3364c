/*
 * cpu_backend_chains.c -- TEST INFRASTRUCTURE ONLY.
 *
 * The CPU backend of cpu_backend.c with offt_backend::pass_pair (y, then x, as cpu_backend_pipeline.c runs it) and STREAMS
 * THAT MEAN SOMETHING, for the two-chain plane groups of execute_single (OFFT_HIP_OPT_ZGROUP_CHAINS,
 * tests/test_zgroup_chains.py):
 *
 *   - every pass, pass_pair, event_record, stream_wait and stream_sync is logged with the stream it was issued on (streams
 *     and events are numbered in the order they were created) and, for a launch, the offset of its output from the caller's
 *     array, from which the test reads the plane range;
 *   - in replay mode nothing runs when it is issued: the operations queue up per stream, and stream_sync(s) runs what the
 *     event edges ALLOW in an order picked to expose a missing edge --
 *       policy 1 (lazy):   only what s needs: its own queue, and another stream's only as far as a wait of s asks for.  What
 *                          nobody waited for has not run when the sync returns (a missing JOIN leaves the second chain's
 *                          planes untouched);
 *       policy 2 (eager):  every other stream runs ahead as far as its waits let it before s takes each step (a missing FORK
 *                          lets the second chain transform planes the launch ahead of the pair has not written yet).
 *     A wait captures the record of its event that was issued last before it, as a stream wait on a device does.  `drop`
 *     names one wait of the log, by its ordinal among the waits, that the replay ignores: the negative control.
 *
 * Built into tests/libcpubackend_chains.so, never into the library.
 */
#include <stdlib.h>
#include <string.h>
#include "offt_backend.h"

const offt_backend *cpu_backend_table(void);

enum { K_PASS = 0, K_PAIR = 1, K_RECORD = 2, K_WAIT = 3, K_SYNC = 4 };
/* the log: kind, stream number, event number (record / wait), n and nb1 of the (first) pass, of the second one of a pair */
typedef struct crec { int kind, stream, event, n, nb1, n2, nb1_2, out_keep; long long out_off, out_off2; } crec;
typedef struct cstream { int id; } cstream;
typedef struct cevent { int id, gen; long last_record; } cevent; /* last_record: queue index of the latest record issued in log `gen` */
/* a queued operation of the replay */
typedef struct cop {
  int kind, stream, done, wait_ordinal;
  long dep; /* K_WAIT: queue index of the record it waits for (-1: the event was never recorded, nothing to wait for) */
  offt_pass_desc d1, d2;
  const void *in1, *in2;
  void *out1, *out2;
} cop;

static offt_backend g_base, g_table;
static crec *g_log = NULL;
static long g_nlog = 0, g_caplog = 0;
static cop *g_q = NULL;
static long g_nq = 0, g_capq = 0;
static const char *g_origin = NULL;
static int g_policy = 0, g_drop = -1, g_gen = 0, g_nstream = 0, g_nevent = 0, g_nwait = 0, g_stuck = 0;

static crec *put(int kind, void *stream) {
  if (g_nlog == g_caplog) { g_caplog = g_caplog ? 2 * g_caplog : 256; g_log = (crec *)realloc(g_log, (size_t)g_caplog * sizeof(crec)); }
  crec *e = &g_log[g_nlog++];
  memset(e, 0, sizeof *e);
  e->kind = kind; e->stream = stream ? ((cstream *)stream)->id : -1; e->event = -1;
  return e;
}
static cop *enqueue(int kind, void *stream) {
  if (g_nq == g_capq) { g_capq = g_capq ? 2 * g_capq : 256; g_q = (cop *)realloc(g_q, (size_t)g_capq * sizeof(cop)); }
  cop *o = &g_q[g_nq++];
  memset(o, 0, sizeof *o);
  o->kind = kind; o->stream = stream ? ((cstream *)stream)->id : -1; o->dep = -1; o->wait_ordinal = -1;
  return o;
}

/* ---- replay ---- */
static int run_op(cop *o) {
  int rc = 0;
  if (o->kind == K_PASS) rc = g_base.pass(&o->d1, o->in1, o->out1, NULL);
  else if (o->kind == K_PAIR) { rc = g_base.pass(&o->d1, o->in1, o->out1, NULL); if (!rc) rc = g_base.pass(&o->d2, o->in2, o->out2, NULL); }
  o->done = 1;
  return rc;
}
static int blocked(const cop *o) { return o->kind == K_WAIT && o->dep >= 0 && o->wait_ordinal != g_drop && !g_q[o->dep].done; }
static long head_of(int stream) { /* the oldest operation of the stream that has not run */
  for (long i = 0; i < g_nq; i++) if (!g_q[i].done && g_q[i].stream == stream) return i;
  return -1;
}
/* lazy: the stream's queue up to and including operation `upto`, other streams only where a wait asks */
static int run_lazy(int stream, long upto, int depth) {
  if (depth > 64) { g_stuck = 1; return -1; }
  for (long i = 0; i <= upto && i < g_nq; i++) {
    cop *o = &g_q[i];
    if (o->done || o->stream != stream) continue;
    if (blocked(o) && run_lazy(g_q[o->dep].stream, o->dep, depth + 1)) return -1;
    if (run_op(o)) return -1;
  }
  return 0;
}
/* eager: every other stream as far as it gets, then one step of `stream`, until its queue is empty */
static int run_eager(int stream) {
  for (;;) {
    for (int t = g_nstream - 1; t >= 0; t--) {
      if (t == stream) continue;
      for (long h; (h = head_of(t)) >= 0 && !blocked(&g_q[h]);) if (run_op(&g_q[h])) return -1;
    }
    const long h = head_of(stream);
    if (h < 0) return 0;
    if (blocked(&g_q[h])) { g_stuck = 1; return -1; } /* the others ran as far as they could: a cycle */
    if (run_op(&g_q[h])) return -1;
  }
}

/* ---- the table ---- */
static void *cc_stream_create(void) { cstream *s = (cstream *)calloc(1, sizeof *s); s->id = g_nstream++; return s; }
static void *cc_event_create(void) { cevent *e = (cevent *)calloc(1, sizeof *e); e->id = g_nevent++; e->last_record = -1; return e; }
static double cc_event_ms(void *a, void *b) { (void)a; (void)b; return 0.0; }
static int cc_event_record(void *e, void *s) {
  put(K_RECORD, s)->event = ((cevent *)e)->id;
  if (g_policy) { enqueue(K_RECORD, s); ((cevent *)e)->last_record = g_nq - 1; ((cevent *)e)->gen = g_gen; }
  return 0;
}
static int cc_stream_wait(void *s, void *e) {
  put(K_WAIT, s)->event = ((cevent *)e)->id;
  if (g_policy) { cop *o = enqueue(K_WAIT, s); o->dep = ((cevent *)e)->gen == g_gen ? ((cevent *)e)->last_record : -1; o->wait_ordinal = g_nwait; }
  g_nwait++;
  return 0;
}
static int cc_stream_sync(void *s) {
  put(K_SYNC, s);
  if (!g_policy) return 0;
  return g_policy == 1 ? run_lazy(((cstream *)s)->id, g_nq - 1, 0) : run_eager(((cstream *)s)->id);
}
static int cc_pass(const offt_pass_desc *d, const void *in, void *out, void *stream) {
  crec *e = put(K_PASS, stream);
  e->n = d->n; e->nb1 = d->nb1; e->out_keep = d->out_keep;
  e->out_off = (long long)((const char *)out - g_origin);
  if (!g_policy) return g_base.pass(d, in, out, stream);
  cop *o = enqueue(K_PASS, stream);
  o->d1 = *d; o->in1 = in; o->out1 = out;
  return 0;
}
static int cc_pass_pair(const offt_pass_desc *dy, const void *iny, void *outy, const offt_pass_desc *dx, const void *inx, void *outx, void *stream) {
  crec *e = put(K_PAIR, stream);
  e->n = dy->n; e->nb1 = dy->nb1; e->out_keep = dy->out_keep; e->n2 = dx->n; e->nb1_2 = dx->nb1;
  e->out_off = (long long)((const char *)outy - g_origin); e->out_off2 = (long long)((const char *)outx - g_origin);
  if (!g_policy) {
    const int rc = g_base.pass(dy, iny, outy, stream);
    return rc ? rc : g_base.pass(dx, inx, outx, stream);
  }
  cop *o = enqueue(K_PAIR, stream);
  o->d1 = *dy; o->in1 = iny; o->out1 = outy; o->d2 = *dx; o->in2 = inx; o->out2 = outx;
  return 0;
}

const offt_backend *cpu_backend_chains_table(void) {
  g_base = *cpu_backend_table();
  g_table = g_base;
  g_table.pass = cc_pass;
  g_table.pass_pair = cc_pass_pair;
  g_table.stream_create = cc_stream_create; /* (destroyed with free(), as the base table does) */
  g_table.event_create = cc_event_create;
  g_table.event_record = cc_event_record;
  g_table.stream_wait = cc_stream_wait;
  g_table.stream_sync = cc_stream_sync;
  g_table.event_ms = cc_event_ms;
  return &g_table;
}
/* a new log; policy 0 runs everything as it is issued, 1 / 2 replay at stream_sync; drop: ordinal of a wait to ignore, -1: none */
void cpu_backend_chains_reset(const void *origin, int policy, int drop) {
  g_nlog = 0; g_nq = 0; g_nwait = 0; g_stuck = 0; g_gen++;
  g_origin = (const char *)origin; g_policy = policy; g_drop = drop;
}
/* run whatever the replay left queued, in the order it was issued (before the buffers go away); returns how many there were */
long cpu_backend_chains_flush(void) {
  long left = 0;
  for (long i = 0; i < g_nq; i++) if (!g_q[i].done) { left += g_q[i].kind <= K_PAIR; run_op(&g_q[i]); }
  g_nq = 0; g_policy = 0;
  return left;
}
int cpu_backend_chains_stuck(void) { return g_stuck; }
long cpu_backend_chains_len(void) { return g_nlog; }
int cpu_backend_chains_rec_bytes(void) { return (int)sizeof(crec); }
void cpu_backend_chains_copy_log(void *dst) { memcpy(dst, g_log, (size_t)g_nlog * sizeof(crec)); }
