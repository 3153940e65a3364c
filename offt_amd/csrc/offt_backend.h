/*
 * offt_backend.h -- the handful of device operations the host pipeline needs,
 * as a table of C function pointers.  The library ships exactly ONE table:
 * HIP kernels + HIP streams/events + RCCL (k_hip_backend in offt_host.c).
 *
 * offt_hip_test_set_backend() (compiled only with -DOFFT_TEST_SEAMS, i.e. into
 * tests/liboffthip_test.so, never into the product) exists so that the CPU-only test-suite can run
 * the real host logic (decomposition, pass descriptors, tile ring, exchange
 * schedule) in world_size-2 `gloo` processes with a descriptor interpreter
 * that lives under tests/ -- the library itself contains no CPU FFT and never
 * installs another table on its own.
 */
#ifndef OFFT_BACKEND_H
#define OFFT_BACKEND_H
#include <stddef.h>
#include "offt_hipk.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct offt_backend {
  void *(*dmalloc)(size_t bytes);
  void (*dfree)(void *p);
  int (*prepare)(int n, int precision);
  int (*pass)(const offt_pass_desc *d, const void *in, void *out, void *stream);
  void *(*stream_create)(void);
  void (*stream_destroy)(void *s);
  void *(*event_create)(void);
  void (*event_destroy)(void *e);
  int (*event_record)(void *e, void *s);
  int (*stream_wait)(void *s, void *e);
  int (*stream_sync)(void *s);
  double (*event_ms)(void *a, void *b);
  /* all-to-all of one tile: which = 1 (row group, p2 peers) or 2 (column group,
   * p1 peers); peer a sends sendbytes[a] from sendp[a], receives recvbytes[a]
   * into recvp[a]; peer index == rank inside the group */
  int (*a2a)(void *ctx, int which, int npeers, const int *peer, const void *const *sendp,
             const size_t *sendbytes, void *const *recvp, const size_t *recvbytes, void *stream);
  int (*memcpy_dd)(void *dst, const void *src, size_t bytes, void *stream);
  /* host -> device copy of a small table, synchronous (plan time) */
  int (*upload)(void *dst, const void *src, size_t bytes);
  /* ---- direct-store exchange (offt_host.c, "p2p") ----
   * peer_open: collective over exchange group `which` (1 row / 2 column / 0 world) of npeers members, this rank being
   * member `self`: every member offers the allocation `local` and gets in peers[a] an address valid HERE for member a's
   * (peers[self] = local).  Non-zero: this backend cannot map peer memory (the plan falls back to the staged exchange). */
  int (*peer_open)(void *ctx, int which, int npeers, int self, void *local, size_t bytes, void **peers);
  void (*peer_close)(void *ctx, int npeers, int self, void **peers);
  /* zeroed 64-bit words that peers write and this rank polls / a status word the host can read while a kernel may still write it */
  void *(*flag_alloc)(size_t bytes, int host_visible);
  void (*flag_free)(void *p, int host_visible);
  /* offt_hipk_flag_signal / offt_hipk_flag_wait (offt_hipk.h) */
  int (*flag_signal)(int n, unsigned long long *const *addr, unsigned long long value, void *stream);
  int (*flag_wait)(int n, unsigned long long *const *addr, unsigned long long value, unsigned long long *status, double timeout_s, void *stream);
  /* ---- spectral convolution (offt_hip_execute_convolve) ----
   * conv_pass: offt_hipk_conv_pass -- the fused forward-pass . filter . inverse-pass launch; NULL: every convolve takes
   * the unfused route.  pointwise: offt_hipk_pointwise -- the multiply of that route; NULL: convolve is refused. */
  int (*conv_pass)(const offt_pass_desc *fwd, const offt_filter_desc *f, const void *filter, void *data, void *stream);
  int (*pointwise)(void *data, const void *filter, int precision, int kind, int n0, int n1, int n2, long long s0, long long s1,
                   long long s2, void *stream);
  /* ---- half box (offt_hip_set_half_box) ----
   * zero_outside: offt_hipk_zero_outside -- clear a strided block outside a kept sub-box (the fallback route: every plan
   * whose passes cannot skip the padding themselves); NULL: half-box is refused on this backend. */
  int (*zero_outside)(void *buf, int precision, int n0, int n1, int n2, int k0, int k1, int k2, long long s0, long long s1, long long s2,
                      void *stream);
  /* ---- multi-output convolution (offt_hip_execute_convolve_multi); appended, so that a table written before them leaves
   * both NULL ----
   * conv_pass_oop: offt_hipk_conv_pass_oop -- the fused launch from `src` into `dst`; NULL: no fused multi-output route.
   * pointwise_oop: offt_hipk_pointwise_oop -- out = in * H; NULL: memcpy_dd followed by the in-place pointwise. */
  int (*conv_pass_oop)(const offt_pass_desc *fwd, const offt_filter_desc *f, const void *filter, const void *src, void *dst,
                       void *stream);
  int (*pointwise_oop)(const void *in, void *out, const void *filter, int precision, int kind, int n0, int n1, int n2, long long s0,
                       long long s1, long long s2, void *stream);
  /* ---- multi-input convolution (offt_hip_execute_convolve_sum); appended again, so that an older table leaves both NULL ----
   * conv_pass_sum: offt_hipk_conv_pass_sum -- the fused launch from nin sources into `dst`; NULL: no fused multi-input route.
   * pointwise_sum: offt_hipk_pointwise_sum -- out = sum_k in_k * H_k; NULL: the call is refused. */
  int (*conv_pass_sum)(const offt_pass_desc *fwd, const offt_filter_desc *f, int nin, const void *const *filters, const void *const *srcs,
                       void *dst, void *stream);
  int (*pointwise_sum)(int nin, const void *const *ins, const void *const *filters, void *out, int precision, int kind, int n0, int n1,
                       int n2, long long s0, long long s1, long long s2, void *stream);
  /* ---- filtered forward / inverse (offt_hip_execute_forward_filtered, offt_hip_execute_inverse_filtered); appended once more,
   * so that an older table leaves both NULL and gets the generic route ----
   * filt_pass_fwd: offt_hipk_filt_pass_fwd -- the forward x pass with the filter on its stores, in place.
   * filt_pass_inv: offt_hipk_filt_pass_inv -- the inverse x pass with the filter on its loads, src -> dst (dst may be src). */
  int (*filt_pass_fwd)(const offt_pass_desc *d, const offt_filter_desc *f, const void *filter, void *data, void *stream);
  int (*filt_pass_inv)(const offt_pass_desc *d, const offt_filter_desc *f, const void *filter, const void *src, void *dst, void *stream);
  /* ---- shell-binned spectra (offt_hip_spectrum_shells); appended at the end, so that every older table leaves it NULL and
   * the call is refused there ----
   * spectrum_shells: offt_hipk_spectrum_shells -- the sweep and the fixed-order sum of its partials (`partials`: device
   * memory of offt_hipk_spectrum_shells_partials bytes, a backend without workgroups ignores it). */
  int (*spectrum_shells)(const void *a, const void *b, int precision, int r2c, const int n[3], const long long stride[3], const int start[3],
                         const int N[3], const int kmul[3], int nbins, double *sums, long long *counts, void *partials,
                         long long partials_bytes, void *stream);
  /* ---- pipelined plane groups (execute_single, OFFT_HIP_OPT_ZGROUP_PIPELINE); appended, so that every older table leaves it
   * NULL and its plans alternate their launches as before ----
   * pass_pair: offt_hipk_fft_pass_pair -- two independent passes as one launch: `dy` from iny to outy and `dx` from inx to
   * outx.  A backend without workgroups runs the two one after the other. */
  int (*pass_pair)(const offt_pass_desc *dy, const void *iny, void *outy, const offt_pass_desc *dx, const void *inx, void *outx, void *stream);
  /* ---- pseudo-spectral product (offt_hip_execute_product); appended at the end, so that every older table leaves both NULL ----
   * prod_pass: offt_hipk_prod_pass -- the fused launch: inverse pass of src0 and src1 (NULL: src0 squared), their product,
   * forward pass, into `dst`; NULL: no fused route.
   * pointwise_prod: offt_hipk_pointwise_prod -- out = x * y; NULL: the call is refused. */
  int (*prod_pass)(const offt_pass_desc *d, const void *src0, const void *src1, void *dst, void *stream);
  int (*pointwise_prod)(const void *x, const void *y, void *out, int precision, int n0, int n1, int n2, long long s0, long long s1, long long s2,
                        void *stream);
  /* ---- ... of real fields on a real-input plan (OFFT_HIP_OPT_PROD_REAL); appended at the end, so that every older table
   * leaves it NULL and its r2c plans keep the generic route ----
   * prod_pass_real: offt_hipk_prod_real_pass -- the fused launch over lines that are half spectra: `d` is the real-output z
   * pass of the inverse (real_input = 2, n the real length, n/2+1 complex values a line through the in_* side). */
  int (*prod_pass_real)(const offt_pass_desc *d, const void *src0, const void *src1, void *dst, void *stream);
} offt_backend;

void offt_hip_test_set_backend(const offt_backend *b, int rank, int size);
/* the HIP backend itself with conv_pass_sum withheld (a table for offt_hip_test_set_backend): the generic multi-input route
 * on the device, for timing it against the fused one */
const offt_backend *offt_hip_test_hip_backend_no_conv_sum(void);
/* ... and with filt_pass_fwd and filt_pass_inv withheld: the generic route of the two filtered calls on the device */
const offt_backend *offt_hip_test_hip_backend_no_filt(void);
/* ... and with prod_pass and prod_pass_real withheld: the generic route of the pseudo-spectral product on the device */
const offt_backend *offt_hip_test_hip_backend_no_prod(void);

/* keep the HIP backend but route the exchange through `fn` (called with the comm stream
 * drained; device pointers): several test ranks can then share one GPU */
typedef int (*offt_test_transport_fn)(int which, int npeers, const int *peer, const void *const *sendp,
                                      const size_t *sendbytes, void *const *recvp, const size_t *recvbytes);
void offt_hip_test_set_transport(offt_test_transport_fn fn, int rank, int size);
/* ... the same, but ASYNCHRONOUS: `fn` is called without draining the stream and gets it as its last argument; it has to
 * enqueue the copies itself (ordered by events between the ranks' streams), so that the schedules' own event edges between
 * compute and comm streams are all that orders kernels and exchanges -- as with RCCL.  Set after offt_hip_test_set_transport. */
typedef int (*offt_test_transport_async_fn)(int which, int npeers, const int *peer, const void *const *sendp, const size_t *sendbytes,
                                            void *const *recvp, const size_t *recvbytes, void *stream);
void offt_hip_test_set_transport_async(offt_test_transport_async_fn fn);
/* several ranks as threads of ONE process (one GPU, or the CPU backend): hipIpc cannot open a handle in the process that
 * made it, so peer_open goes through `fn` (same arguments as offt_backend::peer_open without ctx), which hands out the
 * other threads' pointers; `hook` is called before every wait the direct-store schedule enqueues -- a barrier among the
 * rank threads there guarantees that every signal a wait depends on is already enqueued (streams of one process may
 * share a hardware queue, where a wait kernel ahead of the signal it waits for would never end). */
typedef int (*offt_test_peer_open_fn)(int which, int npeers, int self, void *local, size_t bytes, void **peers);
typedef void (*offt_test_hook_fn)(void);
void offt_hip_test_set_p2p(offt_test_peer_open_fn fn, offt_test_hook_fn hook);
/* p1 of the plan whose exchange is in progress on this thread: with it a transport maps (which, group member) to a
 * world rank -- which 1 = row group (rank_x * p2 + member), 2 = column group (member * p2 + rank_y), 0 = world   */
int offt_hip_test_current_p1(void);
/* 1 if `po` does not use the direct-store exchange, or if all of that exchange's state -- peer mappings, flag groups, slot
 * counters, per-block tables -- was made for the buffers the plan holds now; 0 (reason in offt_hip_last_error()) if any of
 * it describes buffers that were rebuilt since */
struct _offt_plan;
int offt_hip_test_p2p_consistent(const struct _offt_plan *po);

#ifdef __cplusplus
}
#endif
#endif
