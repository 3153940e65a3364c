/*
 * offt_hipk.h -- thin C ABI between the C host library (offt_host.c) and the
 * hand-written HIP kernels (offt_kernels.hip, offt_panel.hpp).  Plain pointers and sizes only.
 *
 * One "pass" = a batch of 1-D FFTs of length n along one axis of a strided
 * complex array, reading a panel [n x COLS] per workgroup, with independent
 * input and output addressing so that the local transposes and the pack /
 * unpack copies of the reference (offt-compute.c:905-2993, 523-653) are folded
 * into the load / store side of the butterfly kernel instead of being separate
 * sweeps over memory.
 */
#ifndef OFFT_HIPK_H
#define OFFT_HIPK_H

#ifdef __cplusplus
extern "C" {
#endif

#define OFFT_PREC_F64 0
#define OFFT_PREC_F32 1

typedef struct offt_pass_desc {
  int n;          /* FFT length along the axis                                   */
  int precision;  /* OFFT_PREC_F64 / OFFT_PREC_F32                               */
  int direction;  /* -1: forward exp(-2 pi i nk/N) (the reference's only mode),  */
                  /* +1: inverse, unnormalised                                   */
  int ncols;      /* number of columns (independent lines) per batch entry       */
  int nb1, nb2;   /* two outer batch dimensions                                  */
  /* all strides in complex elements */
  long long in_axis_stride, in_col_stride, in_b1_stride, in_b2_stride;
  long long out_axis_stride, out_col_stride, out_b1_stride, out_b2_stride;
  /* optional split of the axis index into per-peer blocks (fused unpack on the
   * load side / fused pack on the store side):
   *   idx k -> (k / split) * block_stride + (k % split) * axis_stride
   * split == 0 means "no split".  split_nfloor > 0 selects the reference's
   * uneven A2AV partition (offt-compute.c:132-144): the first split_nfloor
   * blocks hold `split` indices, the remaining ones `split + 1`.               */
  int in_split, in_split_nfloor;
  int out_split, out_split_nfloor;
  long long in_block_stride, out_block_stride;
  /* per-block base table on a split side (device memory; NULL = block b sits at b * block_stride): tab[b] is the
   * ELEMENT offset of axis block b relative to the launch's `in` / `out` pointer, for every block the axis has
   * (ceil(n / split) of them; the number of peers for an uneven split).  The reference packs peer a's share into block
   * a of ONE send buffer (offt-compute.c:1084-1109) which MPI then copies (835-881); with a table the blocks of one pass
   * may live in different allocations -- the self block where the next pass reads it, a peer's block in that peer's
   * receive volume (mapped through hipIpc) -- so the pack IS the exchange.  Offsets may be negative.                  */
  const long long *in_block_tab, *out_block_tab;
  /* coalescing hints: 1 = the FFT axis is the unit-stride dimension,
   *                   0 = the column dimension is the unit-stride dimension    */
  int in_contig, out_contig;
  int variant;    /* static-sweep variant id, -1 = default for this n           */
  double scale;   /* multiplied into the output (1.0 = unnormalised)            */
  /* 0: complex.
   * 1: real-to-complex z pass (fftw_plan_dft_r2c_1d, offt-compute.c:334-336, 960-961):
   * the input line holds n REAL values (unit stride, in_contig = 1, no split) at the
   * start of a row of n/2+1 complex slots; only output indices 0..n/2 are stored.
   * 2: complex-to-real z pass (the inverse of 1): the input line holds n/2+1 complex values
   * (usual in_* strides, split and table) and stands for its conjugate-symmetric extension
   * (the imaginary parts of index 0 and, n even, n/2 have no effect); the pass stores the n
   * REAL values of the transform at the start of a row whose out_* strides count complex
   * slots (out_contig = 1, out_axis_stride = 1, no split).  The row's last one or two
   * scalars (index >= n) are not written. */
  int real_input;
  /* cache hint: 1 = the output is read again right away by the next launch (the x pass over the group of z-planes the
   * y pass has just written): store with the default cache policy so that it stays in L2 / the memory-side Infinity
   * Cache, instead of the streaming (non-temporal) stores every other pass uses */
  int out_keep;
  /* single precision: 1 = do not use the column-pair kernels for this pass (plan option OFFT_HIP_OPT_F32_PAIRS) */
  int no_pairs;
  /* zero-padded half lines (n even).  Bit 1: axis indices >= n/2 of the INPUT line are zero and are not read.  Bit 2: only
   * output indices < n/2 are stored, the others are not written.  Kernels: power-of-two lines of 64 ... 1024 points
   * (fft_half_panel_k) and the mixed-radix lengths 96, 192, 320, 384, 640, 768, 1000 in double and 384, 640, 768, 1000 in
   * single precision (fft_half_panelx_k), complex, no split, in the four flavours of offt_hipk_has_half; a pass that asks
   * for a bit no kernel implements fails, it never runs the full line.  Together with real_input, two forms: real_input = 1
   * with bit 1 (the reals n >= n/2 of a row are zero and not read; contiguous in, strided out) and real_input = 2 with bit
   * 2 (the reals n >= n/2 of a row are not written; strided in, contiguous out).  Bit 4 (value 4) is a permission on these
   * two forms and nothing else: "real rows may run on a mixed-radix half-line kernel" (fft_half_r2c_panelx_k,
   * fft_half_c2r_panelx_k, the mixed-radix lengths above).  Without it a real row has a kernel at the power-of-two lengths
   * only; with it a power-of-two length resolves to the same kernel as without it.  Bits 1 and 2 keep their meaning; bit 4 on
   * a complex descriptor, or alone (half = 4), has no kernel.  (The field sits in what used to be alignment padding: no
   * other offset moves.) */
  int half;
  /* first sub-pass of a four-step line (set by the launcher itself, offt_kernels.hip): multiply output index k1 of column
   * j2 (tw4_b1 = 0) or of batch entry b1 = j2 (tw4_b1 = 1) by tw4[k1 * tw4_n2 + j2] = w_n^(k1 j2), a table of the long
   * length n = n1 n2 laid out [k1][j2] (the lanes of a wave are neighbouring columns j2: one 128-B line per 8 lanes, where
   * indexing the full-wave table by k1 j2 would touch a line per lane).  NULL otherwise.  Needs a kernel with the twiddles
   * on its stores (strided / strided, 32 ... 256 points). */
  const void *tw4;
  int tw4_b1;
  int tw4_n2;
} offt_pass_desc;
/* `half` took the four bytes of padding in front of tw4: the size and every older offset are what they were */
#ifdef __cplusplus
static_assert(sizeof(offt_pass_desc) == 192 && __builtin_offsetof(offt_pass_desc, tw4) == 176, "offt_pass_desc layout");
#else
_Static_assert(sizeof(offt_pass_desc) == 192 && __builtin_offsetof(offt_pass_desc, tw4) == 176, "offt_pass_desc layout");
#endif

/* Build device twiddle tables etc. for length n; call at plan time (allocates).  precision | OFFT_HIPK_PREP_C2R: also
 * the real-output (real_input = 2) kernels of a length whose panel kernel is compiled at plan time (the z length of a
 * real-input plan; every precompiled length has its real-output kernels already). */
#define OFFT_HIPK_PREP_C2R 0x200
int offt_hipk_prepare(int n, int precision);
/* Launch one pass on `stream` (a hipStream_t).  No allocation, no sync.        */
int offt_hipk_fft_pass(const offt_pass_desc *d, const void *in, void *out, void *stream);
/* Two passes as ONE launch on `stream` (fft_pair_yx_k): the workgroups of `dx` (contiguous in and out: the x pass of one
 * group of z-planes) next to those of `dy` (contiguous in, strided out, stored with the default cache policy whatever
 * dy->out_keep says: the y pass of the FOLLOWING group), interleaved in dispatch order.  The two must be independent -- neither
 * reads or writes what the other writes -- because nothing orders them inside the launch.  Each descriptor keeps its own
 * scale.  Forward double-precision complex lines without a split, half lines or four-step twiddles, both passes of the same
 * length: 64, 128, 256, 512 or 1024 points (one shape for both roles, so that neither loses occupancy to the other).  The two bodies are those of the kernels offt_hipk_fft_pass would launch for dy (with out_keep) and dx:
 * equal bits.  -1, nothing launched: no such kernel (a forced variant, another flavour, another length), a NULL pointer. */
int offt_hipk_fft_pass_pair(const offt_pass_desc *dy, const void *iny, void *outy, const offt_pass_desc *dx, const void *inx, void *outx,
                            void *stream);
/* 1 if offt_hipk_fft_pass_pair has a kernel for (dy, dx); a registry lookup, needs no device */
int offt_hipk_has_pass_pair(const offt_pass_desc *dy, const offt_pass_desc *dx);
/* "fft_pair_yx_k", or "no paired kernel" */
const char *offt_hipk_pair_kernel_name(const offt_pass_desc *dy, const offt_pass_desc *dx);
/* The grid offt_hipk_fft_pass_pair would launch, asked without launching (needs no device): the workgroups of either role
 * (*ny_blocks, *nx_blocks: column panels of the role's shape times nb1 times nb2) and how many blocks of EACH role are
 * dispatched in alternating runs (*both, a multiple of the run length; the rest of x, then the rest of y follow).  Any
 * pointer may be NULL.  Returns the run length in blocks (one period of the x role's XCD-aware order, or OFFT_PAIR_RUN), or
 * -1 where offt_hipk_has_pass_pair says 0. */
int offt_hipk_pass_pair_grid(const offt_pass_desc *dy, const offt_pass_desc *dx, long long *ny_blocks, long long *nx_blocks, long long *both);
/* The XCD-aware panel order every launch gives a grid of nblk workgroups (OFFT_XCD_REMAP): returns the run length G in
 * panels (a power of two; 0 = launch order) and in *lim (may be NULL) the number of leading blocks that are renumbered, a
 * multiple of 8 G -- the blocks behind it keep their index.  Needs no device. */
int offt_hipk_panel_order(long long nblk, long long *lim);
/* Workgroup size the any-length kernel (fft_mixed_k) runs lines of n points with (from its LDS footprint, or
 * OFFT_MIX_THREADS); 0: the line is too long for that kernel.  Needs no device. */
int offt_hipk_any_length_threads(int n, int precision);
/* 1 if the pass, with out_keep set, runs on a kernel whose stores stay cached (otherwise out_keep is ignored)          */
int offt_hipk_keeps_output(const offt_pass_desc *d);
/* 1 if a register/LDS Stockham panel kernel exists for (n, precision): powers of two up to 4096
 * and the swept 2^a 3^b 5^c lengths; 0 if the pass will run on the any-length kernel.        */
int offt_hipk_has_fast_path(int n, int precision);
/* number of sweep variants registered for (n, precision, in_contig, out_contig) */
int offt_hipk_variant_count(int n, int precision);
/* human-readable description of a variant, for sweep logs                      */
const char *offt_hipk_variant_name(int n, int precision, int variant);
/* panel shape of a variant (variant = -1: the default): elements per thread and columns
 * per workgroup; returns the variant id or -1 if (n, precision, variant) does not exist  */
int offt_hipk_variant_info(int n, int precision, int variant, int *elems_per_thread, int *cols);
/* name of the kernel symbol a descriptor resolves to as ONE launch (for rocprof matching): the direct layer of the
 * launcher's resolve().  A pass that is decomposed (four-step, lines through scratch) launches several kernels and is
 * named by the kernel that would take its descriptor alone.                      */
const char *offt_hipk_kernel_name(const offt_pass_desc *d);
/* How offt_hipk_fft_pass would run the descriptor: the launcher's own resolve(), asked without launching.  Unlike
 * offt_hipk_kernel_name it names the decomposing routes, and it says WHICH registry entry a panel pass gets -- a forced
 * d->variant that no entry of the flavour carries resolves to the flavour's default, and only this query shows it.
 * *variant_id (may be NULL): the registry id of the panel entry; 200 + id for a column-pair entry (VARIANT_PAIR0, the
 * range d->variant forces them with), 100 for the any-split instance of a power-of-two length (VARIANT_ANYSPLIT); -1 for
 * every route that is not a panel kernel.
 * *n1, *n2 (may be NULL): the factors of a four-step line, else 0.
 * OFFT_ROUTE_NONE: the pass launches nothing -- an empty batch, a half-line or four-step-twiddle descriptor no kernel
 * takes, a line too long for the any-length kernel.  Base pointers count as aligned (as for offt_hipk_kernel_name).  The
 * decomposing routes exist for a length only after offt_hipk_prepare; everything else is a registry lookup and needs
 * no device. */
enum {
  OFFT_ROUTE_NONE = 0,
  OFFT_ROUTE_PANEL = 1,            /* fft_panel_k / fft_panelx_k and their real, half-line and four-step-twiddle forms */
  OFFT_ROUTE_BLUESTEIN_PANEL = 2,  /* fft_bluestein_k */
  OFFT_ROUTE_ANY_LENGTH = 3,       /* fft_mixed_k */
  OFFT_ROUTE_FOUR_STEP = 4,        /* n = n1 n2: two sub-passes through scratch */
  OFFT_ROUTE_SCRATCH_LINES = 5     /* gathered into contiguous scratch lines (uneven blocks, real lines, long Bluestein) */
};
int offt_hipk_pass_route(const offt_pass_desc *d, int *variant_id, int *n1, int *n2);
/* 1 if a half-line kernel exists for the descriptor (d->half = 1 or 2): power-of-two lines of 64 ... 1024 points or one of
 * the mixed-radix lengths listed at offt_pass_desc::half (offt_hipk_kernel_name: "fft_half_panelx_k"), complex,
 * no split, no four-step twiddles, and one of the flavours contiguous-in / strided-out with bit 1, contiguous / contiguous
 * with bit 1 or bit 2, strided-in / contiguous-out with bit 2.  Real rows: real_input = 1 with bit 1 on contiguous-in /
 * strided-out and real_input = 2 with bit 2 on strided-in / contiguous-out, nothing else -- at the power-of-two lengths,
 * and with bit 4 of d->half set also at the mixed-radix ones ("fft_half_r2c_panelx_k", "fft_half_c2r_panelx_k"); bit 4
 * anywhere else: 0.  A registry lookup: needs no device. */
int offt_hipk_has_half(const offt_pass_desc *d);
/* ---- spectral convolution (offt_hip_execute_convolve) ------------------------------------------------------------------
 * A filter H laid out like a forward pass's OUTPUT: kind 0 = one real scalar of the pass's precision per complex slot
 * (scalar index = element index), 1 = one complex value per element.  Strides in complex elements. */
#define OFFT_FILTER_REAL 0
#define OFFT_FILTER_COMPLEX 1
typedef struct offt_filter_desc {
  int kind;
  /* a bit set.  Bit 1 (value 1) = a line length without a power-of-two fused kernel may run on the mixed-radix fused kernels
   * (fft_conv_panelx_k, fft_conv_half_panelx_k: 96, 192, 320, 384, 640, 768, 1000 points in double and 384, 640, 768, 1000 in
   * single precision), 0 = such a length has no fused kernel (plan option OFFT_HIP_OPT_CONV_MIXED).  Bit 2 (value 2) = such a
   * length may run the out-of-place kernel too (fft_conv_oop_panelx_k, fft_conv_oop_half_panelx_k, the same lengths;
   * offt_hipk_conv_pass_oop; plan option OFFT_HIP_OPT_CONV_MULTI_MIXED): it counts only together with bit 1 (mixed = 3), and
   * the in-place launch does not look at it.  Bit 3 (value 4) = such a length may run the multi-input gather kernel
   * (fft_conv_sum_panelx_k, fft_conv_sum_half_panelx_k, the same lengths; offt_hipk_conv_pass_sum; plan option
   * OFFT_HIP_OPT_CONV_SUM_MIXED): it too counts only together with bit 1 ((mixed & 5) == 5), and no other launch looks at
   * it.  Bit 4 (value 8) = a line length without a power-of-two filtered kernel may run on the mixed-radix filtered kernels
   * (fft_filt_fwd_panelx_k, fft_filt_inv_panelx_k, the same lengths; plan option OFFT_HIP_OPT_SPEC_MIXED): it stands alone
   * (it needs none of bits 1-3), only offt_hipk_filt_pass_fwd and offt_hipk_filt_pass_inv read it, and bits 1-3 mean
   * nothing to those two.  A power-of-two length resolves to the same kernel whatever the field says. */
  int mixed;
  long long axis_stride, col_stride, b1_stride, b2_stride;
} offt_filter_desc;
/* `mixed` took the four bytes of padding behind kind: the size and every older offset are what they were */
#ifdef __cplusplus
static_assert(sizeof(offt_filter_desc) == 40 && __builtin_offsetof(offt_filter_desc, axis_stride) == 8, "offt_filter_desc layout");
#else
_Static_assert(sizeof(offt_filter_desc) == 40 && __builtin_offsetof(offt_filter_desc, axis_stride) == 8, "offt_filter_desc layout");
#endif
/* One fused launch on the lines of `fwd` (the last pass of a forward transform): load through its in_* side, forward FFT,
 * times H read where the pass would store (f), inverse FFT (unnormalised), times fwd->scale, store through the same in_*
 * addressing -- in place on `data`.  fwd->out_keep: stores with the default cache policy where the kernel has a
 * cache-keeping twin (the power-of-two full-line kernels), ignored otherwise.  -1 if no fused kernel exists. */
/* fwd->half: 0, or 3 = zero-padded half lines: only indices < n/2 of every line are loaded and only those are stored
 * (the filter is read over the full line); any other non-zero value has no fused kernel. */
int offt_hipk_conv_pass(const offt_pass_desc *fwd, const offt_filter_desc *f, const void *filter, void *data, void *stream);
/* 1 if offt_hipk_conv_pass has a fused kernel for (fwd, f): power-of-two lines of 64 ... 1024 points or, with f->mixed,
 * one of the mixed-radix lengths listed at offt_filter_desc::mixed; contiguous lines (in_contig, no split, complex input)
 * and a unit-stride filter axis; the registry lookup needs no device */
int offt_hipk_conv_has_fused(const offt_pass_desc *fwd, const offt_filter_desc *f);
/* "fft_conv_panel_k", "fft_conv_half_panel_k" (fwd->half = 3), with f->mixed at a mixed-radix length "fft_conv_panelx_k",
 * "fft_conv_half_panelx_k" (fwd->half = 3), or "no fused kernel" (rocprof matching, tests) */
const char *offt_hipk_conv_kernel_name(const offt_pass_desc *fwd, const offt_filter_desc *f);
/* data[i0 s0 + i1 s1 + i2 s2] *= H at the same element index, over the box n0 x n1 x n2 (complex elements, in place);
 * kind as offt_filter_desc::kind.  Non-temporal, 16 B per lane along the smallest stride. */
int offt_hipk_pointwise(void *data, const void *filter, int precision, int kind, int n0, int n1, int n2,
                        long long s0, long long s1, long long s2, void *stream);
/* ---- multi-output convolution (offt_hip_execute_convolve_multi): the two operations that store somewhere other than where
 * they loaded, so that a spectrum can stay where it is while several filters are applied to it ----
 * offt_hipk_conv_pass with a separate destination: the lines of `src` (fwd's in_* addressing) convolved into `dst` at the
 * same offsets; `src` is not written.  fwd->half: 0 or 3, as there; fwd->out_keep: the cache-keeping twin (every instance
 * has one, the half-line ones too).  Power-of-two lines of 64 ... 1024 points; with bits 1 and 2 of f->mixed both set
 * (f->mixed = 3) also the mixed-radix lengths listed at offt_filter_desc::mixed, whose instances have no cache-keeping twin
 * (fwd->out_keep is ignored there, as by offt_hipk_conv_pass); with f->mixed 0, 1 or 2 such a length finds no kernel.
 * -1 if no such kernel exists, and for src == dst (that is offt_hipk_conv_pass). */
int offt_hipk_conv_pass_oop(const offt_pass_desc *fwd, const offt_filter_desc *f, const void *filter, const void *src, void *dst,
                            void *stream);
/* 1 if offt_hipk_conv_pass_oop has a kernel for (fwd, f); the registry lookup needs no device */
int offt_hipk_conv_has_fused_oop(const offt_pass_desc *fwd, const offt_filter_desc *f);
/* "fft_conv_oop_panel_k", "fft_conv_oop_half_panel_k" (fwd->half = 3), with f->mixed = 3 at a mixed-radix length
 * "fft_conv_oop_panelx_k", "fft_conv_oop_half_panelx_k" (fwd->half = 3), or "no fused kernel" */
const char *offt_hipk_conv_oop_kernel_name(const offt_pass_desc *fwd, const offt_filter_desc *f);
/* out[i0 s0 + i1 s1 + i2 s2] = in[same] * H[same] over the box n0 x n1 x n2: offt_hipk_pointwise with a separate destination
 * (in != out; `in` is not written).  Non-temporal, 16 B per lane along the smallest stride. */
int offt_hipk_pointwise_oop(const void *in, void *out, const void *filter, int precision, int kind, int n0, int n1, int n2,
                            long long s0, long long s1, long long s2, void *stream);
/* ---- multi-input convolution (offt_hip_execute_convolve_sum): several sources filtered and summed into one destination ----
 * offt_hipk_conv_pass with nin sources: the lines of every srcs[k] (fwd's in_* addressing) are transformed, multiplied by
 * filters[k] (all addressed by f) and added in the order k = 0 ... nin-1 in registers; ONE inverse transform of the sum,
 * times fwd->scale, is stored to `dst` at the same offsets.  `dst` may be one of the sources (a workgroup has loaded its lines
 * from every source before its only stores); no other source is written.  fwd->half: 0 or 3; fwd->out_keep: the cache-keeping
 * twin (every power-of-two instance has one).  Power-of-two lines of 64 ... 1024 points; with bits 1 and 3 of f->mixed
 * both set ((f->mixed & 5) == 5) also the mixed-radix lengths listed at offt_filter_desc::mixed, whose instances have no
 * cache-keeping twin (fwd->out_keep is ignored there); with any other f->mixed such a length finds no kernel.  -1, and
 * nothing launched, for nin < 1, nin > OFFT_HIPK_CONV_MAX_IN, a NULL pointer or no kernel. */
#define OFFT_HIPK_CONV_MAX_IN 8
int offt_hipk_conv_pass_sum(const offt_pass_desc *fwd, const offt_filter_desc *f, int nin, const void *const *filters,
                            const void *const *srcs, void *dst, void *stream);
/* 1 if offt_hipk_conv_pass_sum has a kernel for (fwd, f): pick_conv's conditions (contiguous lines, unit-stride filter axis,
 * no split, half 0 or 3) at a power of two or, with bits 1 and 3 of f->mixed, at one of the mixed-radix lengths; the
 * registry lookup needs no device */
int offt_hipk_conv_has_fused_sum(const offt_pass_desc *fwd, const offt_filter_desc *f);
/* "fft_conv_sum_panel_k", "fft_conv_sum_half_panel_k" (fwd->half = 3), with (f->mixed & 5) == 5 at a mixed-radix length
 * "fft_conv_sum_panelx_k", "fft_conv_sum_half_panelx_k" (fwd->half = 3), or "no fused kernel" */
const char *offt_hipk_conv_sum_kernel_name(const offt_pass_desc *fwd, const offt_filter_desc *f);
/* out[i0 s0 + i1 s1 + i2 s2] = sum_k ins[k][same] * filters[k][same] over the box n0 x n1 x n2, the terms added in the order
 * k = 0 ... nin-1: ONE sweep, non-temporal, 16 B per lane along the smallest stride.  `out` may be one of the inputs. */
int offt_hipk_pointwise_sum(int nin, const void *const *ins, const void *const *filters, void *out, int precision, int kind, int n0, int n1,
                            int n2, long long s0, long long s1, long long s2, void *stream);
/* ---- filtered forward and filtered inverse (offt_hip_execute_forward_filtered, offt_hip_execute_inverse_filtered): the two
 * halves of offt_hipk_conv_pass as launches of their own, for a caller whose state is a spectrum ----
 * `d` is the x pass of a forward transform: contiguous complex lines (in_contig, in_axis_stride 1, no split, no half lines),
 * addressed through its in_* side on both launches; `f` addresses the filter like that pass's output, axis stride 1.
 * Power-of-two lines of 64 ... 1024 points, each with a cache-keeping twin (d->out_keep); with bit 4 of f->mixed also the
 * mixed-radix lengths listed at offt_filter_desc::mixed, whose instances have no cache-keeping twin (d->out_keep is ignored
 * there); without that bit such a length finds no kernel, whatever bits 1-3 say.
 * offt_hipk_filt_pass_fwd: data = H . FFT(data) . d->scale along the lines, forward (exp(-i...)), in place.
 * offt_hipk_filt_pass_inv: dst = d->scale . IFFT(H . src) along the lines, unnormalised inverse (exp(+i...)) whatever
 * d->direction says, stored at the offsets it loaded from; `src` is not written unless dst == src, which is allowed.
 * -1 if no such kernel exists or a pointer is NULL. */
int offt_hipk_filt_pass_fwd(const offt_pass_desc *d, const offt_filter_desc *f, const void *filter, void *data, void *stream);
int offt_hipk_filt_pass_inv(const offt_pass_desc *d, const offt_filter_desc *f, const void *filter, const void *src, void *dst, void *stream);
/* 1 if BOTH launches have a kernel for (d, f); the registry lookup needs no device */
int offt_hipk_filt_has_fused(const offt_pass_desc *d, const offt_filter_desc *f);
/* "fft_filt_fwd_panel_k" / "fft_filt_inv_panel_k", with bit 4 of f->mixed at a mixed-radix length "fft_filt_fwd_panelx_k" /
 * "fft_filt_inv_panelx_k", or "no fused kernel" */
const char *offt_hipk_filt_fwd_kernel_name(const offt_pass_desc *d, const offt_filter_desc *f);
const char *offt_hipk_filt_inv_kernel_name(const offt_pass_desc *d, const offt_filter_desc *f);
/* ---- shell-binned power and cross spectra (offt_hip_spectrum_shells) ----
 * A read-only sweep over the strided box n[] x stride[] (complex elements of `precision`; arrays indexed by axis x, y, z) of
 * a spectrum whose local index 0 sits at global index start[] of a grid of N[] points (r2c: the box is part of the
 * N[2]/2+1 half spectrum, N[2] the full length, and modes off the planes k_z = 0 and 2 k_z = N[2] weigh 2).  With the signed
 * wavenumbers k_i and K2 = sum (kmul[i] k_i)^2, the shell of a mode is the s with (2s-1)^2 <= 4 K2 < (2s+1)^2, decided in
 * integers; sums[s] = sum of w Re(a conj(b)) over the shell (b NULL or a: |a|^2), counts[s] = sum of w (counts may be NULL),
 * both of nbins entries, overwritten; shells >= nbins are dropped.  start NULL: zeros; kmul NULL: ones.  Every term is
 * formed and added in double.  Rows along the smallest stride, 16 B per lane, non-temporal; no floating-point atomic: runs of
 * equal shell are summed across lanes, the run heads update per-wave LDS tables, waves and workgroups are added in index
 * order (through `partials`, device memory of at least offt_hipk_spectrum_shells_partials bytes, which the call overwrites),
 * so that equal arguments give equal bits.  An empty box stores zeros.  -1, nothing launched: bad arguments, kmul[i] * N[i]/2
 * above 2^30, 2^30 rows or more, too few partials. */
#define OFFT_HIPK_SHELLS_MAX_BINS 4096
int offt_hipk_spectrum_shells(const void *a, const void *b, int precision, int r2c, const int n[3], const long long stride[3],
                              const int start[3], const int N[3], const int kmul[3], int nbins, double *sums, long long *counts,
                              void *partials, long long partials_bytes, void *stream);
/* bytes of `partials` a call with these arguments needs at most (whatever the strides and the arrays' alignment); 0 for an
 * empty box and for arguments the call refuses.  Host arithmetic only. */
long long offt_hipk_spectrum_shells_partials(int precision, const int n[3], const int N[3], const int kmul[3], int nbins);
/* ---- pseudo-spectral product (offt_hip_execute_product): two stored spectra to physical space, multiplied point by point, the
 * product back -- along ONE axis in one launch ----
 * `d` is the last pass of an inverse transform over strided lines (the z pass of the z-y-x schedule: !in_contig, complex, no
 * split, no half lines, no four-step twiddles), addressed through its in_* side for loads and stores alike.  Per line:
 * the unnormalised inverse (exp(+i...), whatever d->direction says) of the line of src0 and of the line of src1, their complex
 * product (src1 NULL or == src0: the square of the one, from one load and one inverse), the forward transform (exp(-i...)),
 * times d->scale, stored to `dst` at the load offsets.  `dst` may be either source: a workgroup owns whole lines and has loaded
 * them from both sources before its only stores; a source that is not `dst` is not written.  d->out_keep is ignored (no
 * cache-keeping twin).  Power-of-two lines of 64 ... 1024 points.  -1, nothing launched: no such kernel, a NULL src0 or dst. */
int offt_hipk_prod_pass(const offt_pass_desc *d, const void *src0, const void *src1, void *dst, void *stream);
/* 1 if offt_hipk_prod_pass has a kernel for d; the registry lookup needs no device */
int offt_hipk_prod_has_fused(const offt_pass_desc *d);
/* "fft_prod_panel_k", or "no fused kernel" */
const char *offt_hipk_prod_kernel_name(const offt_pass_desc *d);
/* ... of REAL fields held as half spectra, the z pass of a real-input (r2c) plan.  `d` is the real-output z pass of the
 * complex-to-real inverse as the schedule states it: real_input = 2, n the REAL length, a line the n/2+1 complex values of a
 * half spectrum at a pitch of in_axis_stride, !in_contig, no split, no half lines, no four-step twiddles; loads and stores
 * through the in_* side.  Per line: the Hermitian extension of the line of src0 and of src1 (X~[k] = X[k] for k <= n/2,
 * conj(X[n - k]) above; the imaginary parts of X[0] and X[n/2] have no effect), the two unnormalised real inverses -- from ONE
 * complex transform of A~ + i B~ --, their product (src1 NULL or == src0: the square), the forward transform, times
 * d->scale; the elements k <= n/2 stored to `dst` at the load offsets, nothing else of the line's pitch written.  `dst` may be
 * either source; a source that is not `dst` is not written.  Power-of-two real lengths of 64 ... 1024.  -1, nothing launched:
 * no such kernel, a NULL src0 or dst. */
int offt_hipk_prod_real_pass(const offt_pass_desc *d, const void *src0, const void *src1, void *dst, void *stream);
/* 1 if offt_hipk_prod_real_pass has a kernel for d; the registry lookup needs no device */
int offt_hipk_prod_real_has_fused(const offt_pass_desc *d);
/* "fft_prod_real_panel_k", or "no fused kernel" */
const char *offt_hipk_prod_real_kernel_name(const offt_pass_desc *d);
/* out[i0 s0 + i1 s1 + i2 s2] = x[same] * y[same] over the box n0 x n1 x n2: complex elements of `precision`, or, with
 * OFFT_HIPK_PROD_REAL or-ed into it, real scalars (the rows of an r2c plan; strides and extents then count scalars).  y NULL
 * or == x: the square, from one load.  `out` may be either operand: a lane loads both before its only store.  ONE sweep,
 * non-temporal, 16 B per lane along a unit stride where the rows allow. */
#define OFFT_HIPK_PROD_REAL 0x100
int offt_hipk_pointwise_prod(const void *x, const void *y, void *out, int precision, int n0, int n1, int n2, long long s0, long long s1,
                             long long s2, void *stream);
/* zero a strided 3-D block n0 x n1 x n2 OUTSIDE the kept sub-box [0,k0) x [0,k1) x [0,k2) (0 <= k <= n); the kept part is
 * not touched.  Elements are complex values of `precision`, or, with OFFT_HIPK_ZERO_REAL or-ed into it, real scalars (the
 * rows of an r2c plan; strides and extents then count scalars).  Vector stores, 16 B per lane along a unit stride s2. */
#define OFFT_HIPK_ZERO_REAL 0x100
int offt_hipk_zero_outside(void *buf, int precision, int n0, int n1, int n2, int k0, int k1, int k2, long long s0, long long s1,
                           long long s2, void *stream);
/* strided complex copy / permutation (used for layouts no FFT pass can fold)   */
int offt_hipk_copy3d(const void *in, void *out, int precision,
                     int n0, int n1, int n2,
                     long long is0, long long is1, long long is2,
                     long long os0, long long os1, long long os2, void *stream);
/* fill a local block with the seeded position hash / the harness ramp
 * (run-fft.c:46-61); kind 0 = ramp, 1 = hash.                                   */
int offt_hipk_fill(void *buf, int precision, int kind,
                   int n0, int n1, int n2, int s0, int s1, int s2,
                   long long st0, long long st1, long long st2, void *stream);
/* ---- flags of the direct-store exchange (offt_host.c, p2p mode) ----------------------------------------------------
 * A rank that has stored its blocks straight into its peers' receive volumes tells them so by writing a monotonically
 * growing value into one 64-bit word per peer (the role MPI_Wait plays behind MPI_Ialltoall, offt-compute.c:883-890);
 * the peers wait for the words of all their senders before the next pass reads.  Both are one-wave launches on the
 * stream: the signal is ordered behind the kernel that stored (whose end-of-kernel release has written its data back),
 * the wait holds the stream until every word has reached `value` or `timeout_s` seconds have passed -- then it writes 1
 * into *status (host-mapped or device memory) and gives up, so that a dead peer ends as an error, never as a hung GPU. */
#define OFFT_HIPK_MAX_FLAGS 16
int offt_hipk_flag_signal(int n, unsigned long long *const *addr, unsigned long long value, void *stream);
int offt_hipk_flag_wait(int n, unsigned long long *const *addr, unsigned long long value, unsigned long long *status,
                        double timeout_s, void *stream);
/* one wave that holds `stream` for `ms` milliseconds (used by test builds to make the device lag behind the host) */
int offt_hipk_delay(double ms, void *stream);
const char *offt_hipk_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
