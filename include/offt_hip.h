/*
 * offt_hip.h -- MI355X-specific extensions around the offt.h boundary.
 *
 * The reference binds ranks through MPI_COMM_WORLD inside offt_3d_init
 * (offt-compute.c:3315-3316) and exchanges tiles with MPI_Ialltoall
 * (offt-compute.c:835-900).  Here one process drives one GPU and the exchange
 * is an RCCL all-to-all over xGMI, so the world (rank, size, RCCL unique id) is
 * handed in through this C ABI by whatever launcher is in use (torchrun +
 * torch.distributed store, MPI_Bcast, a file): plain pointers and sizes only.
 *
 * Everything in this header is an extension: callers that only use offt.h get
 * the reference's behaviour (single process == world of one rank).
 */
#ifndef OFFT_HIP_INCLUDE
#define OFFT_HIP_INCLUDE

#include "offt.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OFFT_HIP_UNIQUE_ID_BYTES 128

/* ---- world bootstrap (replaces MPI_Comm_size/rank, offt-compute.c:3315) ---- */
/* rank 0 creates the RCCL unique id; the launcher ships the 128 bytes around. */
int offt_hip_get_unique_id(void *id128);
/* declare this process as `rank` of `size`; id128 may be NULL when size == 1.
 * Must precede offt_3d_init.  Binds the process to `device` (hipSetDevice).    */
int offt_hip_set_world(int rank, int size, const void *id128, int device);
/* tear the world down (destroys the RCCL communicator)                         */
int offt_hip_finalize_world(void);
int offt_hip_world_rank(void);
int offt_hip_world_size(void);
/* number of ranks that answer on the world communicator (an ncclAllReduce of ones); -1 on failure.  Collective.    */
int offt_hip_world_count(void);
/* xGMI link probe on the world communicator: grouped ncclSend/ncclRecv of `bytes` per peer, `reps` repetitions after
 * one warm-up.  mode 0 = all-to-all among all ranks, mode 1 = ring shift by `shift` (one link per direction).
 * Returns this rank's seconds per repetition, negative on failure.  Collective.                                     */
double offt_hip_link_probe(int mode, int shift, long long bytes, int reps);

/* ---- plan extensions -------------------------------------------------------- */
#define OFFT_HIP_F64 0
#define OFFT_HIP_F32 1
/* Same arguments as offt_3d_init plus the arithmetic type (the reference is
 * double only, Appendix F of SURVEY.md).  With OFFT_HIP_F32 `in`/`out` point at
 * interleaved float pairs.                                                      */
struct _offt_plan *offt_3d_init_ex(int Nx, int Ny, int Nz, void *in, void *out, int is_r2c,
                                   int fftw_flag, int is_oned, int is_a2a, int is_equalxy,
                                   int is_notest, int ah_strategy, int max_loop, int tuning_mode,
                                   int is_W0, int extrapolation_window,
                                   struct _offt_params *custom_params, int precision);
/* direction: -1 forward (what offt_3d_execute does), +1 inverse (unnormalised,
 * FFTW_BACKWARD convention).  The inverse consumes the forward's OUTPUT layout
 * (ostart/osize/ostride) and produces the INPUT layout (istart/isize/istride).
 * On a real-input plan (is_r2c = 1) the inverse is complex-to-real: Nz/2+1 complex
 * values along z in, real rows out (element (x,y,z) at scalar index
 * z + 2*istride[1]*y + 2*istride[0]*x), numpy.fft.irfftn(X, s=(Nx,Ny,Nz)) * Nx*Ny*Nz for
 * even and odd Nz.  As with FFTW, the imaginary parts of the z = 0 plane (and of z = Nz/2,
 * Nz even) have no effect; the input is consumed and the one or two scalars after each
 * row's Nz reals are undefined afterwards.  offt_hip_set_output_scale applies to the
 * z pass, which runs last. */
void offt_3d_execute_dir(struct _offt_plan *po, void *in, void *out, int direction);
/* spectral convolution, in place: `data` (device memory) holds this rank's block in the INPUT layout
 * (istart/isize/istride; real rows for an r2c plan) and receives  scale * N * ifftn(H * fftn(x))  (complex plan) or
 * scale * N * irfftn(H * rfftn(x), s=(Nx,Ny,Nz))  (r2c plan) in the same layout, N = Nx*Ny*Nz, scale =
 * offt_hip_set_output_scale (applied once, on the final store).  `filter` (device memory) holds H for this rank's part of
 * the spectrum, laid out exactly like the forward's OUTPUT block (ostart/osize/ostride, offsets in complex elements; the
 * Nz/2+1 half spectrum for r2c plans): one complex value per element, or (REAL) one scalar of the plan's precision per
 * complex slot, at the same element index.  The forward transform of a kernel g with the same plan is such an H.
 * Collective on several ranks; honours offt_hip_set_stream / offt_hip_set_async like offt_3d_execute_dir.  0 on success;
 * -1 with t[ALL] = 99999999 and offt_hip_last_error() on failure, and for a NULL or host-memory filter, host-memory data or
 * an unknown filter_kind.  offt_hip_last_device_seconds covers the whole call; offt_hip_last_pass_seconds reports zeros. */
#define OFFT_HIP_FILTER_REAL    0   /* one scalar of the plan's precision per spectrum element */
#define OFFT_HIP_FILTER_COMPLEX 1   /* one complex value per spectrum element                  */
int offt_hip_execute_convolve(struct _offt_plan *po, void *data, const void *filter, int filter_kind);
/* 1 if this plan's convolve runs the fused route (one launch for forward-pass . filter . inverse-pass), 0 otherwise: one
 * rank, an x extent that is a power of two from 64 to 1024 or, with OFFT_HIP_OPT_CONV_MIXED, one of the mixed-radix lengths
 * listed there */
int offt_hip_convolve_fused(const struct _offt_plan *po);
/* spectral convolution with several outputs: ONE forward transform of `data`, then for k = 0 ... nout-1
 *   outs[k] = scale * N * ifftn(filters[k] * fftn(x))   (irfftn / rfftn for an r2c plan)
 * in the INPUT layout, exactly as offt_hip_execute_convolve leaves `data` -- the force components of a particle-mesh code
 * from one density, the potential and the field of a Hockney solver.  filters[k] is laid out like the forward's OUTPUT block;
 * all filters share one filter_kind.  `data` is consumed: its contents are undefined afterwards, unless one outs[k] is `data`
 * itself (at most one may be) -- that output is computed last and `data` holds it.  Every other outs[k] is a device buffer of
 * its own of offt_hip_local_bytes(po) bytes that overlaps neither `data` nor another output.  The output scale applies once
 * per output; stream, async, half box, OFFT_HIP_OPT_CONV_MIXED and OFFT_HIP_OPT_ZGROUP_MIB are honoured as in the
 * single-output call (a mixed-radix x extent takes the generic route here -- forward, then a multiply and an inverse per
 * output -- unless OFFT_HIP_OPT_CONV_MULTI_MIXED is set as well).  Collective on several ranks.  0 on success; -1 with t[ALL] = 99999999 and offt_hip_last_error() for nout < 1 or
 * nout > OFFT_HIP_CONV_MAX_OUT, a NULL or host-memory outs[k] or filters[k], two equal outs entries, an unknown
 * filter_kind, host-memory data, a failed communicator.  With nout == 1 and outs[0] == data the call IS
 * offt_hip_execute_convolve: the same bits.  offt_hip_last_device_seconds covers the whole call;
 * offt_hip_last_pass_seconds reports zeros. */
#define OFFT_HIP_CONV_MAX_OUT 8
int offt_hip_execute_convolve_multi(struct _offt_plan *po, void *data, int nout, void *const *outs, const void *const *filters,
                                    int filter_kind);
/* 1 if outputs other than `data` run the fused multi-output route: the forward's z and y passes once, then per output one
 * out-of-place launch (forward x pass . filter . inverse x pass, data -> outs[k]) and the inverse's y and z passes -- one
 * rank, the default z-y-x layout, an x extent that is a power of two from 64 to 1024 or, with OFFT_HIP_OPT_CONV_MIXED and
 * OFFT_HIP_OPT_CONV_MULTI_MIXED both set, one of the mixed-radix lengths listed there; 0: the generic route */
int offt_hip_convolve_multi_fused(const struct _offt_plan *po);
/* spectral convolution with several inputs: nin forward transforms, ONE inverse:
 *   out = scale * N * ifftn( sum_k filters[k] * fftn(x_k) )   (irfftn / rfftn for an r2c plan)
 * -- the transpose of offt_hip_execute_convolve_multi: the inverse Laplacian of the divergence of a vector field (pressure
 * projection), the potential of several charge species with a shape function each, multi-channel correlation.  ins[k] is this
 * rank's block of input k in the INPUT layout and follows the rules of `data` in the single-output call (real rows on an r2c
 * plan, the half box); filters[k] is laid out like the forward's OUTPUT block, all filters share one filter_kind; `out`
 * receives the result in the INPUT layout and may be any one of the ins[k] or a device buffer of its own of
 * offt_hip_local_bytes(po) bytes.  EVERY ins[k] is consumed: its contents are undefined afterwards, unless it is `out`.  The
 * terms are added in the order k = 0 ... nin-1 on every route (a call is reproducible bit for bit); the output scale applies
 * once, on the final store.  Stream, async, half box and OFFT_HIP_OPT_ZGROUP_MIB are honoured as in
 * offt_hip_execute_convolve_multi; a plan whose x extent is no power of two takes the generic route unless
 * OFFT_HIP_OPT_CONV_MIXED and OFFT_HIP_OPT_CONV_SUM_MIXED are both set.  Collective on several ranks.  0 on success; -1 with t[ALL] = 99999999 and
 * offt_hip_last_error(), and nothing launched, for nin < 1 or nin > OFFT_HIP_CONV_MAX_IN, NULL ins or filters arrays, a NULL
 * or host-memory ins[k], filters[k] or out, two equal ins entries, an unknown filter_kind, a backend without the
 * multiply-and-sum, a failed communicator.  With nin == 1 and out == ins[0] the call IS offt_hip_execute_convolve: the same
 * bits.  offt_hip_last_device_seconds covers the whole call; offt_hip_last_pass_seconds reports zeros. */
#define OFFT_HIP_CONV_MAX_IN 8
int offt_hip_execute_convolve_sum(struct _offt_plan *po, int nin, void *const *ins, const void *const *filters, int filter_kind, void *out);
/* 1 if the call runs the fused multi-input route: the forward's z and y passes per input, then ONE launch that runs the
 * forward x pass of every input, multiplies, sums in registers and runs the inverse x pass (all ins -> out), and the
 * inverse's y and z passes once -- one rank, the default z-y-x layout, an x extent that is a power of two from 64 to 1024
 * or, with OFFT_HIP_OPT_CONV_MIXED and OFFT_HIP_OPT_CONV_SUM_MIXED both set, one of the mixed-radix lengths listed there;
 * 0: the generic route (a forward per input, one multiply-and-sum sweep, one inverse) */
int offt_hip_convolve_sum_fused(const struct _offt_plan *po);
/* Filtered forward and filtered inverse: the two halves of a convolve as calls of their own, for a solver that keeps its
 * state as a spectrum (pseudo-spectral Navier-Stokes, Cahn-Hilliard, spectral field solves).  Filters are laid out and
 * typed as for offt_hip_execute_convolve.
 * Forward: data (input layout) becomes H . fftn(data) in the forward's OUTPUT layout, in place -- what offt_3d_execute
 * followed by a multiply with H leaves, offt_hip_set_output_scale included (a dealiasing mask or projector on the
 * nonlinear term).
 * Inverse: outs[k] = unnormalised inverse transform of filters[k] . spec, k = 0 ... nout-1, each in the INPUT layout with
 * the output scale on its final store (real values for an r2c plan) -- the velocity and its derivatives, i k_j u^, from
 * one stored spectrum.  spec is in the forward's output layout and is NOT written, unless it is one of outs[]: at most
 * one may be, and the library makes it last whatever its position.  Every outs[k] has offt_hip_local_bytes bytes;
 * 1 <= nout <= OFFT_HIP_CONV_MAX_OUT.
 * With scale 1, inverse_filtered(forward_filtered(x, H1), [H2]) equals offt_hip_execute_convolve(x, H1 . H2) to rounding.
 * On one rank, in the z-y-x layout, with a power-of-two x extent from 64 to 1024 and no half box, the x pass carries the
 * multiply where OFFT_HIP_OPT_SPEC_FUSED is set (off by default), and with OFFT_HIP_OPT_SPEC_MIXED set as well also with a mixed-radix x
 * extent that has a filtered kernel pair; every other plan transforms and multiplies in separate launches.  Stream, async,
 * offt_hip_last_device_seconds and OFFT_HIP_OPT_ZGROUP_MIB are honoured as in offt_hip_execute_convolve_multi.
 * Collective on several ranks.  0 on success; -1 with t[ALL] = 99999999 and offt_hip_last_error(), and nothing launched,
 * for a NULL or host-memory argument, a bad nout, two equal outs entries, an unknown filter_kind, a backend without the
 * multiply, a failed communicator. */
int offt_hip_execute_forward_filtered(struct _offt_plan *po, void *data, const void *filter, int filter_kind);
int offt_hip_execute_inverse_filtered(struct _offt_plan *po, const void *spec, int nout, void *const *outs, const void *const *filters,
                                      int filter_kind);
/* 1 if both calls take the fused route on this plan, else 0 */
int offt_hip_spectral_fused(const struct _offt_plan *po);
/* Shell-binned power and cross spectra of a stored spectrum: the isotropic P(|k|) of a density or velocity field, or the
 * cross spectrum of two fields, from this rank's block in the forward's OUTPUT layout (the Nz/2+1 half spectrum of an r2c
 * plan), without the spectrum leaving the device.  a and b (NULL: b = a) are device memory in the plan's precision; neither
 * is written.
 * On axis i, global index g has the signed wavenumber k_i = g if 2 g <= N_i, else g - N_i; K2 = (kmul[0] k_x)^2 +
 * (kmul[1] k_y)^2 + (kmul[2] k_z)^2 in 64-bit integers (kmul NULL: {1,1,1}; a 2N x N x N grid of one spacing: {1,2,2}).
 * The shell of a mode is the nearest integer to sqrt(K2), the s with (2s-1)^2 <= 4 K2 < (2s+1)^2, decided in integer
 * arithmetic: membership is exact.  Modes of shells >= nbins are left out.
 * sums[s] = sum over the shell of w Re(A conj(B)), counts[s] = sum of w (counts may be NULL): device arrays of nbins entries,
 * overwritten.  w = 1; on an r2c plan w = 2 where 0 < k_z and 2 k_z != Nz, so that both arrays equal what the full spectrum
 * of the real field gives.  Every element is converted to double before its product, and every term is formed and added in
 * double, single-precision plans included; the order of the additions depends on the plan and nbins only, so that two calls
 * with the same inputs give the same bits.
 * LOCAL, not collective: on several ranks each rank gets the partial sums of its own block (zeros for an empty block), and
 * adding them across ranks is the caller's.  Stream, async and offt_hip_last_device_seconds as for
 * offt_hip_execute_forward_filtered; offt_hip_last_pass_seconds reports zeros.
 * 0 on success; -1 with t[ALL] = 99999999 and offt_hip_last_error(), and nothing launched, for a NULL or host-memory a or
 * sums, a host-memory b or counts, nbins < 1 or > OFFT_HIP_SHELLS_MAX_BINS, a kmul entry below 1, a backend without the
 * entry. */
#define OFFT_HIP_SHELLS_MAX_BINS 4096
int offt_hip_spectrum_shells(struct _offt_plan *po, const void *a, const void *b, const int kmul[3], int nbins, double *sums,
                             long long *counts);
/* Pseudo-spectral product: two stored spectra to physical space, multiplied point by point, the product back -- the
 * nonlinear term (u . grad u, phi^2) of a solver that keeps its state as a spectrum.  a and b (device memory) each hold this
 * rank's block of a spectrum in the forward's OUTPUT layout (ostart/osize/ostride; the Nz/2+1 half spectrum of an r2c plan);
 * `out` receives, in the same layout,
 *   scale * F( Finv(A) (.) Finv(B) )
 * with Finv the library's UNNORMALISED inverse and F its unnormalised forward: with N = Nx*Ny*Nz, in numpy terms
 *   scale * N^2 * fftn(ifftn(A) * ifftn(B))                  (complex plan: the complex product)
 *   scale * N^2 * rfftn(irfftn(A, s) * irfftn(B, s))         (r2c plan: the product of the real fields)
 * scale = offt_hip_set_output_scale, applied once, on the final store; every inner pass runs with scale 1.  The intermediate
 * fields are the unnormalised inverses: N times larger than normalised ones, which in single precision is that much closer
 * to the largest float -- scale the spectra down before the call where N * max|field| could approach 3e38.
 * b == NULL or b == a squares the field (one inverse).  `out` may be a, b, or a device buffer of its own of
 * offt_hip_local_bytes(po) bytes that overlaps neither input.  a and b are consumed: their contents are undefined afterwards
 * unless they are `out`.  On an r2c plan the imaginary parts of the plane z = 0 (and z = Nz/2, Nz even) have no effect, as with
 * any c2r inverse -- on the fused route too (OFFT_HIP_OPT_PROD_REAL), which drops them before it packs the two spectra into
 * one transform.  On a half-box plan the product is formed inside the box and its zero-padded spectrum is returned.
 * Stream, async, offt_hip_wait and offt_hip_last_device_seconds (the whole call) as in offt_hip_execute_convolve_sum;
 * offt_hip_last_pass_seconds reports zeros.  Collective on several ranks.  0 on success; -1 with t[ALL] = 99999999 and
 * offt_hip_last_error(), and nothing launched, for a NULL or host-memory a or out, a host-memory b, a backend without the
 * multiply, a failed communicator. */
int offt_hip_execute_product(struct _offt_plan *po, void *a, void *b, void *out);
/* 1 if the call runs the fused route: the inverse's x and y passes per input, ONE launch that runs the inverse z pass of
 * both, multiplies in registers and runs the forward z pass (the physical field is never written), the forward's y and x
 * passes -- one rank, the default z-y-x layout, no half box, a z extent that is a power of two from 64 to 1024,
 * OFFT_HIP_OPT_PROD_FUSED set, and on a real-input (r2c) plan OFFT_HIP_OPT_PROD_REAL as well (the launch then works on the
 * half-spectrum lines and yields both real fields from one complex inverse); 0: the generic route (an inverse per input, one
 * multiply sweep, one forward) */
int offt_hip_product_fused(const struct _offt_plan *po);
/* Zero-padded input: the data lives in the box [0,Nx/2) x [0,Ny/2) x [0,Nz/2) (global indices) of the INPUT layout.
 * Forward: whatever else the input block holds is ignored (treated as zero, need not be initialised); the output is the
 *   full spectrum of the zero-padded field, in the usual output layout.
 * Inverse: only the box of the result is defined afterwards; the rest of the block is undefined.
 * Convolve: box in, box out -- the aperiodic convolution when the kernel's support fits.
 * Real-input (r2c) plans: the box is the reals z < Nz/2 of the rows x < Nx/2, y < Ny/2; the forward's output is the usual
 *   Nz/2+1 half spectrum, and the inverse defines the reals of the box only (the scalars behind a row's reals stay
 *   undefined, as after any c2r inverse).  Such a plan clears the padding and runs the ordinary schedule unless
 *   OFFT_HIP_OPT_HALF_R2C is set: then its passes skip the padding like a complex plan's.
 * Extents that are no powers of two: such a plan clears the padding and runs the ordinary schedule unless
 *   OFFT_HIP_OPT_HALF_MIXED is set and every extent has a half-line kernel.  A real-input plan with such an extent needs
 *   OFFT_HIP_OPT_HALF_R2C, OFFT_HIP_OPT_HALF_MIXED and OFFT_HIP_OPT_HALF_R2C_MIXED, all three.
 * -1 (plan unchanged, text in offt_hip_last_error) if an extent is odd.  Collective on several ranks. */
int offt_hip_set_half_box(struct _offt_plan *po, int on);
/* 1: every pass of this plan skips the padding (half-line kernels); 0: the library clears the padding and runs the
 * ordinary schedule.  The results are the same. */
int offt_hip_half_box_pruned(const struct _offt_plan *po);
/* run on a caller-owned hipStream_t (NULL = the plan's own stream)             */
void offt_hip_set_stream(struct _offt_plan *po, void *stream);
/* 0: offt_3d_execute returns after the GPU finished (timers valid, reference
 *    behaviour); 1: returns after enqueueing (caller synchronises the stream);
 *    no timing events are recorded then, so back-to-back small transforms pay
 *    for the kernel launches only.                                              */
void offt_hip_set_async(struct _offt_plan *po, int async);
/* asynchronous mode: wait for everything enqueued on the plan so far.  Like the end of a synchronous execute the wait
 * is bounded (OFFT_EXEC_TIMEOUT) and polls the RCCL communicators for asynchronous errors; returns 0, or -1 with
 * t[ALL] = 99999999 and the text in offt_hip_last_error().                                                        */
int offt_hip_wait(struct _offt_plan *po);
/* plan-level options.  Each has an environment variable of the same meaning that is read ONCE, by offt_3d_init, as the
 * default; after that a plan's behaviour does not depend on the process environment.  Options marked (collective) rebuild
 * the plan's exchange buffers: every rank of the world calls them with the same value.  0 on success. */
#define OFFT_HIP_OPT_ZGROUP_MIB 0      /* single rank: MiB per group of the alternating y / x launches; 0 off, -1 library rule (OFFT_ZGROUP_MIB) */
#define OFFT_HIP_OPT_ZGROUP_STREAMS 1  /* ... 2 = consumer launches on a second stream (OFFT_ZGROUP_STREAMS) */
#define OFFT_HIP_OPT_SLAB_CHUNK_MIB 2  /* (collective) slab schedule: largest z-chunk in MiB (OFFT_SLAB_CHUNK_MIB) */
#define OFFT_HIP_OPT_COMM_STREAMS 3    /* pencil schedule: 2 = row and column exchanges on two streams (OFFT_COMM_STREAMS) */
#define OFFT_HIP_OPT_F32_PAIRS 4       /* single precision: 0 = never the column-pair kernels (OFFT_F32_PAIRS) */
#define OFFT_HIP_OPT_K1_STREAMS 5      /* slab schedule: 2 = FFTz launches of consecutive x-tiles on two streams (OFFT_K1_STREAMS) */
#define OFFT_HIP_OPT_SELF_BYPASS 6     /* (collective) 0 = a rank's own block goes through the exchange like any other (OFFT_SELF_BYPASS) */
#define OFFT_HIP_OPT_MIN_MSG 7         /* (collective) bytes a per-peer message is merged up to (OFFT_MIN_MSG) */
#define OFFT_HIP_OPT_EXEC_TIMEOUT_S 8  /* bound of the final wait of a multi-rank execute (OFFT_EXEC_TIMEOUT) */
#define OFFT_HIP_OPT_P2P_TIMEOUT_S 9   /* bound of one flag wait of the direct-store exchange (OFFT_P2P_TIMEOUT) */
#define OFFT_HIP_OPT_HALF_R2C 10       /* half box on a real-input (r2c) plan: 1 = its passes skip the padding where every pass has a
                                          half-line kernel, 0 (default) = always clear and run the ordinary schedule.  Set before or
                                          after offt_hip_set_half_box: a half box that is on changes route at once (OFFT_HALF_R2C) */
#define OFFT_HIP_OPT_HALF_MIXED 11     /* half box on a plan with an extent that is no power of two: 1 = its passes skip the padding where
                                          every pass has a half-line kernel (96, 192, 320, 384, 640, 768, 1000 points in double, 384,
                                          640, 768, 1000 in single precision, next to the powers of two from 64 to 1024; complex plans -- real-input
                                          ones need OFFT_HIP_OPT_HALF_R2C_MIXED as well),
                                          0 (default) = always clear and run the ordinary schedule.  Set before or after
                                          offt_hip_set_half_box, like OFFT_HIP_OPT_HALF_R2C (OFFT_HALF_MIXED) */
#define OFFT_HIP_OPT_CONV_MIXED 12     /* convolve on a plan whose x extent is no power of two: 1 = the fused route (one launch for the
                                          forward's last pass, the filter and the inverse's first pass) where that extent has a fused
                                          mixed-radix kernel (96, 192, 320, 384, 640, 768, 1000 points in double, 384, 640, 768, 1000 in
                                          single precision; complex and r2c plans, one rank; with OFFT_HIP_OPT_HALF_MIXED also a pruned
                                          half box), 0 (default) = forward, multiply, inverse.  Read by every convolve; the results
                                          agree to rounding (OFFT_CONV_MIXED) */
#define OFFT_HIP_OPT_HALF_R2C_MIXED 13 /* half box on a real-input (r2c) plan with an extent that is no power of two: 1 = together with
                                          OFFT_HIP_OPT_HALF_R2C and OFFT_HIP_OPT_HALF_MIXED (all three set) its passes skip the padding
                                          where every pass has a half-line kernel -- the lengths listed at OFFT_HIP_OPT_HALF_MIXED, real
                                          rows included; 0 (default) = such a plan always clears and runs the ordinary schedule, whatever
                                          the other two say.  Neither of those changes its meaning.  Set before or after
                                          offt_hip_set_half_box, like them (OFFT_HALF_R2C_MIXED) */
#define OFFT_HIP_OPT_CONV_MULTI_MIXED 14 /* multi-output convolve on a plan whose x extent is no power of two: 1 = together with
                                          OFFT_HIP_OPT_CONV_MIXED (both set) the fused multi-output route where that extent has an
                                          out-of-place fused mixed-radix kernel (the lengths listed at OFFT_HIP_OPT_CONV_MIXED; complex
                                          and r2c plans, one rank, the z-y-x layout; with OFFT_HIP_OPT_HALF_MIXED also a pruned half
                                          box), 0 (default) = one forward, then a multiply and an inverse per output.  Alone it changes
                                          nothing.  Read by every multi-output convolve; the results agree to rounding
                                          (OFFT_CONV_MULTI_MIXED) */
/* (15 is not assigned: offt_hip_set_option answers -1 for it, as for every unknown number) */
#define OFFT_HIP_OPT_CONV_SUM_MIXED 16 /* multi-input convolve on a plan whose x extent is no power of two: 1 = together with
                                          OFFT_HIP_OPT_CONV_MIXED (both set) the fused multi-input route where that extent has a
                                          mixed-radix gather kernel (the lengths listed at OFFT_HIP_OPT_CONV_MIXED; complex and r2c
                                          plans, one rank, the z-y-x layout; with OFFT_HIP_OPT_HALF_MIXED also a pruned half box),
                                          0 (default) = a forward per input, one multiply-and-sum sweep, one inverse.  Alone it
                                          changes nothing.  Read by every multi-input convolve; the results agree to rounding
                                          (OFFT_CONV_SUM_MIXED) */
/* (17 is not assigned either) */
#define OFFT_HIP_OPT_SPEC_FUSED 18     /* filtered forward / inverse: 1 = the x pass carries the multiply where the plan has that route
                                          (offt_hip_spectral_fused: one rank, z-y-x, a power-of-two x extent from 64 to 1024, no half
                                          box), 0 (default) = transform and multiply as separate launches.  Read by every filtered
                                          call; the results agree to rounding (OFFT_SPEC_FUSED) */
#define OFFT_HIP_OPT_ZGROUP_PIPELINE 19 /* single rank, forward z-y-x in double precision: 1 (default) = the x launch of one plane group and
                                          the y launch of the next are ONE launch (y(0) | {x(0), y(1)} | ... | x(G-1)) where the x and y
                                          extents are equal and 64, 128, 256, 512 or 1024 points; 0 = the launches alternate.  Equal
                                          bits either way; never with OFFT_HIP_OPT_ZGROUP_STREAMS = 2 (OFFT_ZGROUP_PIPELINE) */
#define OFFT_HIP_OPT_ZGROUP_PLANES 20  /* single rank, the forward z-y-x transform only (no convolve or filtered call reads it): planes
                                          per group of its y / x launches where they run in groups at all -- it turns nothing on, and
                                          OFFT_HIP_OPT_ZGROUP_MIB = 0 stays off; > 0 takes the place of the MiB count, 0 (default) =
                                          that count decides.  For groups finer than a MiB (OFFT_ZGROUP_PLANES) */
#define OFFT_HIP_OPT_SPEC_MIXED 21     /* filtered forward / inverse on a plan whose x extent is no power of two: 1 = together with
                                          OFFT_HIP_OPT_SPEC_FUSED (both set) the x pass carries the multiply where that extent has a
                                          mixed-radix filtered kernel pair (96, 192, 320, 384, 640, 768, 1000 points in double, 384, 640,
                                          768, 1000 in single precision; complex and r2c plans, one rank, the z-y-x layout, no half
                                          box), 0 (default) = such a plan transforms and multiplies in separate launches.  Alone it
                                          changes nothing.  Read by every filtered call; the results agree to rounding
                                          (OFFT_SPEC_MIXED) */
/* (22 is not assigned, like 15 and 17) */
#define OFFT_HIP_OPT_ZGROUP_CHAINS 23  /* the pipelined plane groups of OFFT_HIP_OPT_ZGROUP_PIPELINE (same plans, and only with it): 2 = two
                                          independent chains, the even groups on the plan's stream and the odd groups on a second
                                          stream of the library's (y(0) | {x(0), y(2)} | ... | x(G-2)  next to  y(1) | {x(1), y(3)} |
                                          ... | x(G-1)), forked behind the z pass and joined before the call returns or enqueues anything
                                          else; the groups are then half the usual size unless OFFT_HIP_OPT_ZGROUP_PLANES /
                                          OFFT_HIP_OPT_ZGROUP_MIB fix it, and a transform of fewer than 4 groups runs as one chain;
                                          1 = one chain.  The default is 2 where the library sizes the groups itself; a plan whose
                                          group size is fixed takes two chains only once this option (or OFFT_ZGROUP_CHAINS) is set.
                                          Equal bits either way; any other value is refused (OFFT_ZGROUP_CHAINS) */
#define OFFT_HIP_OPT_PROD_FUSED 24     /* pseudo-spectral product: 1 = the z passes of both inverses, the multiply and the forward's z
                                          pass are one launch where the plan has that route (offt_hip_product_fused), 0 (default) =
                                          an inverse per input, a multiply sweep, a forward.  Any non-zero value reads back as 1.  Read
                                          by every product call; the results agree to rounding (OFFT_PROD_FUSED) */
#define OFFT_HIP_OPT_PROD_REAL 25      /* pseudo-spectral product on a real-input (r2c) plan: 1 = together with OFFT_HIP_OPT_PROD_FUSED
                                          the fused route may run there too -- its one launch works on half-spectrum lines and takes
                                          both real inverses from one packed complex transform; 0 (default) = an r2c plan keeps the
                                          generic route whatever OFFT_HIP_OPT_PROD_FUSED says.  Without OFFT_HIP_OPT_PROD_FUSED it has
                                          no effect; a complex plan does not read it.  Any non-zero value reads back as 1.  Read by
                                          every product call; the results agree to rounding (OFFT_PROD_REAL) */
int offt_hip_set_option(struct _offt_plan *po, int option, long long value);
/* (Launchers that want an exchange-only / compute-only split of a multi-rank execute link the DIAGNOSTICS build,
 *  tools/liboffthip_diag.so = the product compiled with -DOFFT_BENCH_DIAGNOSTICS, which adds
 *  void offt_hip_set_debug_skip(po, mask): mask 1 leaves out the FFT passes, 2 the exchanges.  The product library does
 *  not contain it.) */
long long offt_hip_get_option(const struct _offt_plan *po, int option);
/* exchange of a multi-rank plan.  STAGED (default): the packing passes fill a send volume, grouped RCCL send/recv moves
 * it (the reference's pack + MPI_Ialltoall, offt-compute.c:1084-1109, 835-881); a rank's own block bypasses the exchange.
 * DIRECT: the packing passes store every block straight into its owner's receive volume (peer memory mapped through
 * hipIpc at plan time) and 64-bit flags replace the exchange -- no send volume, no copy kernels.  Collective: all ranks
 * call it with the same mode.  Returns the mode in use afterwards (DIRECT falls back to STAGED on all ranks together where
 * peer memory cannot be mapped), -1 on failure.  OFFT_EXCHANGE=p2p in the environment is the init-time default. */
#define OFFT_HIP_EXCHANGE_STAGED 0
#define OFFT_HIP_EXCHANGE_DIRECT 1
int offt_hip_set_exchange(struct _offt_plan *po, int mode);
int offt_hip_get_exchange(const struct _offt_plan *po);
/* select a static-sweep kernel variant per axis (0 = x, 1 = y, 2 = z); -1 default */
void offt_hip_set_variant(struct _offt_plan *po, int axis, int variant);
/* multiply the result by `scale` in the store of the last pass (1.0 = the reference's
 * unnormalised transform); free, it rides on the kernel's stores                  */
void offt_hip_set_output_scale(struct _offt_plan *po, double scale);
/* bytes the caller must allocate for in/out on this rank (run-fft.c:294-304)   */
long long offt_hip_local_bytes(const struct _offt_plan *po);
/* device time of the last execute in seconds, from hipEvents on the plan stream */
double offt_hip_last_device_seconds(const struct _offt_plan *po);
/* per-pass device seconds of the last execute: z, y, x passes (0 if fused away).  When two of the passes ran as
 * alternating launches over groups of planes (single rank: the y and x passes of the z-y-x layout), only their SUM was
 * measured and each of the two slots holds half of it: offt_hip_last_passes_paired() returns 0, or the two slots as
 * bits (1 = z, 2 = y, 4 = x). */
void offt_hip_last_pass_seconds(const struct _offt_plan *po, double t[3]);
int offt_hip_last_passes_paired(const struct _offt_plan *po);
/* how many launches of the last single-rank execute carried two passes in one grid (OFFT_HIP_OPT_ZGROUP_PIPELINE): 0 = the
 * plan did not take that route */
int offt_hip_last_pipelined_launches(const struct _offt_plan *po);
/* ... and in how many chains they ran (OFFT_HIP_OPT_ZGROUP_CHAINS): 2 = on two streams, 1 = on the plan's stream alone, 0 = the
 * last execute did not take the pipelined route.  The count above is over both chains */
int offt_hip_last_pipelined_chains(const struct _offt_plan *po);
/* last error text ("" if none); errors also go to stderr, like the reference's
 * printf-only error handling (offt-compute.c:702-704)                           */
const char *offt_hip_last_error(void);

/* ---- device helpers for harnesses and tests ---------------------------------- */
void *offt_hip_malloc(long long bytes);
void offt_hip_free(void *p);
int offt_hip_memcpy_h2d(void *dst, const void *src, long long bytes);
int offt_hip_memcpy_d2h(void *dst, const void *src, long long bytes);
int offt_hip_device_synchronize(void);
/* fill this rank's input block (istart/isize/istride) on the device:
 * kind 0 = harness ramp re = z + 10 y + 100 x (run-fft.c:46-61), 1 = seeded
 * position hash in [-1,1)                                */
int offt_hip_fill_input(struct _offt_plan *po, void *buf, int kind);

#ifdef __cplusplus
}
#endif
#endif
