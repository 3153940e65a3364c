// offt_panel.hpp -- hand-written CDNA4 (gfx950) kernels for the OFFT hot path.
//
// What the reference does per pencil with FFTW + element-wise memcpy
// (offt-compute.c:959-963 FFTz, 1484-1494 / 1708-1710 FFTy, 2493-2495 FFTx,
//  pack/unpack 1029-1109, 1307-1385, 1773-2058, 2447-2687, transpose 625-639)
// is done here by ONE kernel family: a panel Stockham FFT.
//
//  * a workgroup owns a panel [N x COLS] of one axis: N = FFT length, COLS =
//    independent lines;
//  * every thread keeps E complex points in registers and does radix-R0/R1/R2
//    butterflies entirely in registers (radix 2..32, built from radix-2 DIF
//    stages with compile-time twiddles);
//  * between register stages the panel is exchanged through LDS (Stockham
//    autosort indexing, padded against bank conflicts; optionally re / im in
//    two half-size sweeps so that two workgroups fit the 160 KiB LDS of a CU);
//  * inter-stage twiddles come from a quarter-wave table staged in LDS
//    (exact to 0.5 ulp, no sincos recurrences);
//  * loads and stores use independent stride descriptors, so the transposes
//    and the pack/unpack of the pencil decomposition ride on the FFT's own
//    HBM traffic.  Wave lanes run along whichever dimension is unit-stride
//    (IN_CONTIG / OUT_CONTIG), 16 B per lane.
//
// No MFMA: the path is HBM-bound (1.56 flop/B), see DESIGN.md.

//
// This header holds the device templates and the variant registry helpers; the
// instantiations live in offt_reg_*.hip (one translation unit per group so that
// the build runs in parallel), the C ABI in offt_kernels.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>
#include <vector>
#include <string>
#include <cstdio>
#include "offt_hipk.h"
#include "offt_w32_consts.h"
#include "offt_wr_consts.h"

namespace offtk {

template <typename T> struct vec2;
template <> struct vec2<double> { using type = double2; };
template <> struct vec2<float> { using type = float2; };

template <typename T> struct cx { T x, y; };

// COLUMN PAIRS (single precision).  T = f32x2 runs the same kernel with two adjacent columns per lane: every register
// value, butterfly operation and LDS word carries the pair (v_pk_* arithmetic, 8-B LDS words -- the double-precision
// kernel's instruction count for twice the elements), a strided side moves 16 B per lane (one 128-B segment = 8 lanes, as in
// double precision), twiddles and addresses are computed once per pair.  A contiguous side still moves 8 B per lane, one
// access per column.  Needs an even column count and, on a strided side, a unit column stride with even other strides
// (16-B alignment): pair_ok() in offt_kernels.hip; anything else runs on the one-column kernels.
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
template <> struct vec2<f32x2> { using type = float2; };  // memory and twiddle tables hold plain complex floats
template <typename T> struct lanes { using scalar = T; static constexpr int n = 1; };
template <> struct lanes<f32x2> { using scalar = float; static constexpr int n = 2; };

// global memory access helpers: 16-B (f64) / 8-B (f32) per lane.  Every element is
// touched exactly once per pass, so loads and stores are non-temporal (streaming): A/B on
// 1024^3 (profiles/r01_sweep.txt): -6 % transform time vs default cache policy.
template <typename V2>
__device__ __forceinline__ V2 gload(const V2 *p) {
  using E = decltype(p->x);
  typedef E vt __attribute__((ext_vector_type(2)));
  vt r = __builtin_nontemporal_load(reinterpret_cast<const vt *>(p));
  V2 o; o.x = r.x; o.y = r.y; return o;
}
template <typename V2>
__device__ __forceinline__ void gstore(V2 *p, V2 v) {
  using E = decltype(p->x);
  typedef E vt __attribute__((ext_vector_type(2)));
  vt r; r.x = v.x; r.y = v.y;
  __builtin_nontemporal_store(r, reinterpret_cast<vt *>(p));
}

// KEEP: the same vector store with the default cache policy.  The two forms differ in the store's cache hint and in nothing
// else the optimiser sees, so a KEEP instantiation rounds exactly like its plain twin (a struct store here once gave the
// single-precision 256- and 1024-point twins other packed-math and contraction choices: last-place differences)
template <bool KEEP, typename V2>
__device__ __forceinline__ void gstore_p(V2 *p, V2 v) {
  if constexpr (KEEP) {
    using E = decltype(p->x);
    typedef E vt __attribute__((ext_vector_type(2)));
    vt r; r.x = v.x; r.y = v.y;
    *reinterpret_cast<vt *>(p) = r;
  } else gstore(p, v);
}

// v with its sign bit XORed by m (m = 0 or 0x80000000, uniform): conjugation and half-wave twiddle signs cost one
// 32-bit XOR instead of a select + negate
__device__ __forceinline__ double xor_sign(double v, unsigned m) { return __hiloint2double(__double2hiint(v) ^ (int)m, __double2loint(v)); }
__device__ __forceinline__ float xor_sign(float v, unsigned m) { return __int_as_float(__float_as_int(v) ^ (int)m); }
__device__ __forceinline__ f32x2 xor_sign(f32x2 v, unsigned m) { f32x2 r; r.x = xor_sign((float)v.x, m); r.y = xor_sign((float)v.y, m); return r; }

// i / d for 0 <= i < 2^22 with inv = 1.0f / d: float estimate, one correction step each way
__device__ __forceinline__ int fdiv(int i, int d, float inv) {
  int q = (int)((float)i * inv);
  int r = i - q * d;
  if (r < 0) q--;
  else if (r >= d) q++;
  return q;
}

// Workgroups are dealt round-robin to the 8 XCDs (each with its own L2 and address translation cache), so in
// launch order neighbouring panels land on different XCDs.  Renumbering gives every XCD runs of G = 2^gshift
// panels that are neighbours in memory: block b (XCD b % 8, its r-th block) takes panel
// (r / G) * 8G + (b % 8) * G + r % G.  Blocks at or above lim (the tail that does not fill 8 G) keep their index.
// 1024^3 f64: 17.65 -> 17.0 ms per transform (profiles/r01_sweep.txt).
__device__ __forceinline__ unsigned panel_of_block(unsigned bid, unsigned lim, unsigned gshift) {
  if (bid >= lim) return bid;
  const unsigned x = bid & 7u, r = bid >> 3;
  return ((r >> gshift) << (gshift + 3u)) + (x << gshift) + (r & ((1u << gshift) - 1u));
}

// element offset of axis index n under a per-peer split (SPLIT = false: none): indices below lim = split * nfloor
// sit in blocks of `split`, the others in blocks of split + 1 -- the reference's uneven A2AV partition
// (offt-compute.c:132-144); an even split is the case lim >= N.
// `tab` (offt_pass_desc::in_block_tab / out_block_tab): per-block element offsets replacing blk * blk_stride, or nullptr.
template <bool SPLIT>
__device__ __forceinline__ long long split_offset(int n, int split, float inv, int nfloor, int lim, float inv1, long long blk_stride,
                                                  long long axis_stride, const long long *tab = nullptr) {
  if constexpr (!SPLIT) return (long long)n * axis_stride;
  else {
    int blk, rem;
    if (n < lim) { blk = fdiv(n, split, inv); rem = n - blk * split; }
    else { const int m = n - lim, b = fdiv(m, split + 1, inv1); blk = nfloor + b; rem = m - b * (split + 1); }
    return (tab ? tab[blk] : (long long)blk * blk_stride) + (long long)rem * axis_stride;
  }
}

template <int B, int E_, class F>
__device__ __forceinline__ void static_for(F &&f) {
  if constexpr (B < E_) {
    f(std::integral_constant<int, B>{});
    static_for<B + 1, E_>(f);
  }
}

constexpr int ilog2(int n) { return n <= 1 ? 0 : 1 + ilog2(n >> 1); }
constexpr int bitrev(int v, int bits) {
  int r = 0;
  for (int i = 0; i < bits; ++i) r |= ((v >> i) & 1) << (bits - 1 - i);
  return r;
}

constexpr double W32C[32] = OFFT_W32_COS;
constexpr double W32S[32] = OFFT_W32_SIN;
constexpr double WRC[33][32] = OFFT_WR_COS;
constexpr double WRS[33][32] = OFFT_WR_SIN;

// d * w32^K, w32 = exp(-2 pi i / 32)
template <typename T, int K>
__device__ __forceinline__ cx<T> mulw32(cx<T> d) {
  using S = typename lanes<T>::scalar;
  constexpr int k = K & 31;
  if constexpr (k == 0) return d;
  else if constexpr (k == 8) return cx<T>{d.y, -d.x};
  else if constexpr (k == 16) return cx<T>{-d.x, -d.y};
  else if constexpr (k == 24) return cx<T>{-d.y, d.x};
  else if constexpr (k == 4) {
    constexpr S s = (S)W32C[4];
    return cx<T>{(d.x + d.y) * s, (d.y - d.x) * s};
  } else if constexpr (k == 12) {
    constexpr S s = (S)W32C[4];
    return cx<T>{(d.y - d.x) * s, -(d.x + d.y) * s};
  } else {
    constexpr S c = (S)W32C[k], s = (S)W32S[k];
    return cx<T>{d.x * c + d.y * s, d.y * c - d.x * s};
  }
}

// In-register radix-R DFT (R = 2..32), radix-2 decimation in frequency with
// compile-time twiddles.  Result is left in bit-reversed order:
// X[k] = v[bitrev(k)].
// UZ: v[R/2 ...] are known zeros (the upper half of a zero-padded line, offt_pass_desc::half): they are not read, and
// the first butterfly is a copy and a twiddle.
template <typename T, int R, bool UZ = false>
__device__ __forceinline__ void dft_reg(cx<T> *v) {
  static_for<0, ilog2(R)>([&](auto st) {
    constexpr int h = R >> (decltype(st)::value + 1);
    static_for<0, R / 2>([&](auto bi) {
      constexpr int b = (decltype(bi)::value / h) * 2 * h;
      constexpr int i = decltype(bi)::value % h;
      if constexpr (UZ && decltype(st)::value == 0) {
        v[b + i + h] = mulw32<T, i * (16 / h)>(v[b + i]);
      } else {
        cx<T> p = v[b + i], q = v[b + i + h];
        v[b + i] = cx<T>{p.x + q.x, p.y + q.y};
        cx<T> d{p.x - q.x, p.y - q.y};
        v[b + i + h] = mulw32<T, i * (16 / h)>(d);
      }
    });
  });
}

struct PassArgs {
  long long in_axis, in_col, in_b1, in_b2, in_blk;
  long long out_axis, out_col, out_b1, out_b2, out_blk;
  int in_shift, out_shift;  // log2(split) or 31 for "no split"            (fft_panel_k)
  int in_split, out_split;  // split length, any value, 0 for "no split"   (fft_panelx_k)
  float in_inv, out_inv;    // 1 / split
  int in_nfloor, out_nfloor;  // uneven A2AV partition (offt-compute.c:132-144): the first nfloor blocks hold `split`
  int in_lim, out_lim;        //   indices (axis indices below lim = split * nfloor), the others split + 1;
  float in_inv1, out_inv1;    //   inv1 = 1 / (split + 1).  Even split: lim >= n.
  int ncols, ncp, nb1;      // ncp = column panels per batch entry
  int conj;                 // 1: inverse transform via conj-in / conj-out
  unsigned xcd_lim;         // XCD-aware panel order for blocks below this index (see panel_of_block), 0 = off
  unsigned xcd_gshift;      // log2 G, G = run of neighbouring panels one XCD takes
  double scale;
  const long long *in_tab, *out_tab;  // per-block element offsets (offt_pass_desc::in_block_tab / out_block_tab) or nullptr
  const void *tw4;          // TW4 kernels (first sub-pass of a four-step line): w^(k1 j2) of the LONG length as a table [k1][j2];
  int tw4_b1;               //   output index k1 of column j2 (tw4_b1 = 0) or of batch entry j2 = b1 (tw4_b1 = 1) times w^(k1 j2)
  int tw4_n2;               //   row length of that table
};

template <int N, int E, int R0, int R1, int R2, int COLS, bool SPLIT, typename T>
struct PanelCfg {
  static constexpr int TPL = N / E;
  static constexpr int NT = TPL * COLS;
  static constexpr int NSTAGE = (R2 > 1) ? 3 : ((R1 > 1) ? 2 : 1);
  // LDS image of one column: Stockham stage s writes index (q-k)*R + k + t*Ns with lanes
  // along q and reads index q' + t'*(N/R') with lanes along q'.  Stage 0 (Ns = 1) is a
  // stride-R0 write: all lanes of a ds_write group would hit one bank.
  //  * R0 >= 16: XOR swizzle  i -> i ^ ((i >> log2 R0) & 15).  The strided writes spread
  //    over 16 bank pairs, and the unit-stride accesses are only permuted inside aligned
  //    16-element runs, so they stay conflict-free (a padded image misaligns them: the
  //    PMC pass showed SQ_LDS_BANK_CONFLICT = 50 % of SQ_LDS_IDX_ACTIVE with padding).
  //  * R0 < 16 (small N): pad one element every R0.
  static constexpr bool SWZ = (R0 >= 16);
  static constexpr int PADSHIFT = ilog2(R0) < 3 ? 3 : ilog2(R0);
  static constexpr int SWZSHIFT = ilog2(R0);
  static constexpr int NPAD = SWZ ? N : N + (N >> PADSHIFT);
  // column pitch == 4 (mod 32) elements: the 8 columns x 4 rows of one 32-lane ds_read_b64
  // group of a strided-store flavour land in 32 distinct bank pairs
  static constexpr int LSTRIDE = SWZ ? ((NPAD + 31) / 32) * 32 + 4 : ((NPAD + 13) / 16) * 16 + 2;
  static constexpr size_t EX_BYTES =
      NSTAGE > 1 ? (size_t)COLS * LSTRIDE * sizeof(T) * (SPLIT ? 1 : 2) : 0;
  static constexpr size_t TW_OFF = (EX_BYTES + 15) / 16 * 16;
  // Inter-stage twiddles, staged in LDS from the exact full-wave table in global memory:
  //  * one table for all stages: the QUARTER wave (N/4+1 entries; the other three quadrants by swap / sign, ~10 integer
  //    instructions per twiddle) or the HALF wave (N/2 entries; w^(e + N/2) = -w^e is one XOR) -- the half wave whenever it
  //    does not cost a workgroup per CU;
  //  * a COMPACT table for stage 1, tw1[t-1][k] = w^(k t N/(R0 R1)), k < R0, t < R1: the 16 lanes of an LDS read group
  //    then read 16 consecutive entries instead of entries 16 t N/(R0 R1) bytes apart (the r02 PMC pass showed
  //    SQ_LDS_BANK_CONFLICT = 55-60 % of SQ_LDS_IDX_ACTIVE on the 2048-point kernels, from exactly these reads) -- again
  //    only when it does not cost a workgroup per CU.
  static constexpr int QTQ = (N >= 4) ? N / 4 + 1 : 1, QTH = N / 2, T1N = NSTAGE > 1 ? R0 * (R1 - 1) : 0;
  static constexpr size_t lds_with(int shared_entries, int t1_entries) {
    return NSTAGE > 1 ? TW_OFF + ((size_t)shared_entries + (size_t)t1_entries) * 2 * sizeof(typename lanes<T>::scalar) : 0;
  }
  static constexpr int wg_for(size_t lds) { return lds ? (int)(160 * 1024 / lds) : 8; }
  static constexpr bool USE_T1 = NSTAGE > 1 && wg_for(lds_with(QTQ, T1N)) == wg_for(lds_with(QTQ, 0));
  static constexpr bool USE_HALF = NSTAGE > 1 && N >= 16 && wg_for(lds_with(QTH, USE_T1 ? T1N : 0)) == wg_for(lds_with(QTQ, 0));
  static constexpr int QT = USE_HALF ? QTH : QTQ;
  static constexpr size_t T1_OFF = TW_OFF + (size_t)QT * 2 * sizeof(typename lanes<T>::scalar);
  static constexpr size_t LDS_BYTES = lds_with(QT, USE_T1 ? T1N : 0);
  // occupancy target handed to __launch_bounds__ (2nd argument = waves per
  // SIMD): as many workgroups per CU as the 160 KiB LDS admits, at most 4
  // waves per SIMD -- enough to overlap one group's butterflies with another
  // group's HBM traffic without starving the register allocator.
  static constexpr int WG_PER_CU_LDS = wg_for(LDS_BYTES);
  static constexpr int WPS_RAW = (WG_PER_CU_LDS * NT + 255) / 256;
  static constexpr int WPS = WPS_RAW < 1 ? 1 : (WPS_RAW > 4 ? 4 : WPS_RAW);
  // register budget: an E-point thread keeps E*sizeof(T)/2 data VGPRs; it needs
  // roughly twice that (butterfly temporaries, addresses, exchange staging)
  static constexpr int DATA_VGPR = E * (int)sizeof(T) / 2;
  // (a radix-32 butterfly alone keeps ~40 temporaries alive: never ask for more than 2 waves/SIMD)
  static constexpr int WPS_REG = (DATA_VGPR >= 128 || R0 >= 32 || R1 >= 32 || R2 >= 32) ? 2 : (DATA_VGPR >= 64 ? 3 : 4);
  static constexpr int WPS_MIN = (NT + 255) / 256;  // one workgroup must fit on a CU
  static constexpr int WPS_E = WPS < WPS_REG ? WPS : (WPS_REG < WPS_MIN ? WPS_MIN : WPS_REG);
};

template <bool SWZ, int SHIFT>
__device__ __forceinline__ int padidx(int i) {
  if constexpr (SWZ) return i ^ ((i >> SHIFT) & 15);
  else return i + (i >> SHIFT);
}

// The body of fft_panel_k and fft_c2r_panel_k (below).  The kernels are thin __global__ wrappers so that the complex and
// real-input instances keep their symbols (a template parameter added to fft_panel_k itself, defaulted or not, would be
// part of every instance's mangled name): profiles/ and the rocprof matching of tools/ rely on them.
//   R2C  real-input z pass (offt_pass_desc::real_input = 1)
//   KEEP stores with the default cache policy: the next launch re-reads the output (out_keep)
//   TW4  four-step lines (offt_kernels.hip): the twiddles w_n^(j2 k1) of the long length ride on the stores
//   C2R  real-output z pass (offt_pass_desc::real_input = 2): n/2+1 complex inputs, n real outputs
//   HALF zero-padded half lines (offt_pass_desc::half, fft_half_panel_k): bit 1 = axis indices >= N/2 of the input are
//        zero and not loaded, bit 2 = output indices >= N/2 are not stored.  An element's axis index is j + cn with
//        j < TPL and cn a compile-time multiple of TPL, and TPL divides N/2: which half an element is in is known at
//        compile time on either side -- no predicate, no address arithmetic for the skipped half.  The two real ends
//        of a half-box chain (fft_half_r2c_panel_k, fft_half_c2r_panel_k): R2C with bit 1 -- the reals n >= N/2 of a row
//        are zero and not loaded; C2R with bit 2 -- the reals n >= N/2 of a row are not stored
//   blk  the workgroup's index in the pass's grid: blockIdx.x, except in a launch that carries two passes (fft_pair_yx_k)
template <typename T, int N, int E, int R0, int R1, int R2, int COLS, bool INC, bool OUTC, bool SPLIT, bool R2C, bool KEEP, bool TW4,
          bool C2R, int HALF = 0>
__device__ __forceinline__ void panel_body(PassArgs a, const typename vec2<T>::type *in, typename vec2<T>::type *out,
                                           const typename vec2<T>::type *twq, const unsigned blk = blockIdx.x) {
  using V2 = typename vec2<T>::type;
  using S = typename lanes<T>::scalar;
  constexpr int NL = lanes<T>::n;   // memory columns per lane (2: column pairs)
  constexpr bool PAIR = NL == 2;
  using XV = std::conditional_t<PAIR, f32x4, V2>;  // packed exchange word: (re, im) of the lane's column(s)
  using Cfg = PanelCfg<N, E, R0, R1, R2, COLS, SPLIT, T>;
  constexpr int TPL = Cfg::TPL, NT = Cfg::NT, NSTAGE = Cfg::NSTAGE;
  constexpr int LSTRIDE = Cfg::LSTRIDE;
  constexpr bool SWZ = Cfg::SWZ;
  constexpr int PS = SWZ ? Cfg::SWZSHIFT : Cfg::PADSHIFT;
  static_assert(R0 * R1 * R2 == N, "radices must multiply to N");
  static_assert(E % R0 == 0 && E % R1 == 0 && E % R2 == 0 && N % E == 0, "bad E");
  static_assert(!(PAIR && R2C), "column pairs: complex input only");
  static_assert(!(PAIR && TW4), "four-step twiddles: one column per lane");
  static_assert(!(PAIR && C2R) && !(R2C && C2R) && !(TW4 && C2R) && (!C2R || OUTC), "real output: one column per lane, contiguous rows");
  static_assert(HALF == 0 || (!TW4 && NSTAGE > 1 && (N / 2) % TPL == 0), "half lines: no four-step twiddles");
  static_assert(HALF == 0 || ((!R2C || (HALF == 1 && INC && !OUTC)) && (!C2R || (HALF == 2 && !INC))),
                "half lines, real ends: bit 1 on the real-input pass, bit 2 on the real-output pass");

  extern __shared__ __align__(16) unsigned char smem[];
  T *exs = reinterpret_cast<T *>(smem);
  XV *exv = reinterpret_cast<XV *>(smem);
  V2 *tw = reinterpret_cast<V2 *>(smem + Cfg::TW_OFF);
  V2 *tw1 = reinterpret_cast<V2 *>(smem + Cfg::T1_OFF);

  const int tid = threadIdx.x;
  if constexpr (NSTAGE > 1) {
    // twq = the exact full-wave table w^m, m < N, in global memory (L2-resident: every workgroup reads it)
    for (int i = tid; i < Cfg::QT; i += NT) tw[i] = twq[i];
    if constexpr (Cfg::USE_T1) {
      constexpr int M1 = N / (R0 * R1);
      for (int i = tid; i < Cfg::T1N; i += NT) {
        const int t = i / R0 + 1, k = i - (t - 1) * R0;
        tw1[i] = twq[k * M1 * t];  // k t M1 <= (R0-1)(R1-1) M1 < N
      }
    }
  }

  // panel -> (column panel, b1, b2)
  const unsigned bid = panel_of_block(blk, a.xcd_lim, a.xcd_gshift);
  const int cp = bid % (unsigned)a.ncp;
  const unsigned rest = bid / (unsigned)a.ncp;
  const int b1 = rest % (unsigned)a.nb1;
  const int b2 = rest / (unsigned)a.nb1;
  const int c0 = cp * COLS * NL;
  const unsigned conj_mask = a.conj ? 0x80000000u : 0u;  // inverse transform = conj-in / conj-out: one XOR per element

  cx<T> v[E];

  // ---------------- stage 0: global load -------------------------------------
  // Element (u, t) of this thread is axis index n = j + cn with j < TPL and cn = u TPL + t N/R0, a compile-time multiple
  // of TPL.  A per-peer split has a power-of-two length F = 2^shift (any other split runs on fft_panelx_k): for F >= TPL
  // cn's offset bits plus j stay below F, for F < TPL cn has no offset bits at all -- either way block index and offset
  // of n are the SUMS of those of j and cn.  So the address is (a per-lane base for j) + (a wave-uniform offset for cn):
  // the offsets are scalar-unit work and an element costs a 64-bit add instead of two 64-bit multiply-adds (the ISA of the
  // r01 kernels had 130 v_mad_u64_u32 per thread).
  int c, j;
  if constexpr (INC) { j = tid % TPL; c = tid / TPL; }
  else               { c = tid % COLS; j = tid / COLS; }
  {
    const bool valid = (c0 + c * NL) < a.ncols;  // (pairs: the host sends even column counts only)
    // pairs: lanes past the last column re-read the panel's first pair instead of being predicated off (a predicated
    // load whose components are then regrouped into register pairs compiled to one branch and one full wait PER LOAD);
    // what they compute is never stored
    const int cl = (PAIR && !valid) ? 0 : c;
    const V2 *src = in + (long long)b1 * a.in_b1 + (long long)b2 * a.in_b2 + (long long)(c0 + cl * NL) * a.in_col;
    const int mask = (int)((1u << a.in_shift) - 1u);
    // TAB: the blocks of the split come from a table of element offsets (in_block_tab) instead of blk * in_blk; block
    // index and offset of n = j + cn are still the sums of those of j and cn, so the lookup index is (j >> shift) + (cn >> shift)
    // PLAIN (C2R only): no split on the input side
    auto load_all = [&](auto tabbed, auto plain) {
      constexpr bool TAB = decltype(tabbed)::value, PLAIN = decltype(plain)::value;
      const int jb = j >> a.in_shift;
      const V2 *p0 = src + (TAB ? 0LL : (long long)jb * a.in_blk) + (long long)(j & mask) * a.in_axis;
      const V2 *pm = src - (long long)j * a.in_axis;  // (C2R, PLAIN: mirrored index N - j - cn = -j + a uniform N - cn)
      static_for<0, E>([&](auto ii) {
        constexpr int u = decltype(ii)::value / R0, t = decltype(ii)::value % R0;
        constexpr int cn = u * TPL + t * (N / R0);
        const int n = j + cn;
        V2 val;
        val.x = 0; val.y = 0;
        if constexpr (C2R) {
          // the conjugate-symmetric extension of the n/2+1 stored values: element n is X[n] for n <= N/2 and conj(X[N - n])
          // above, then conj-in as for any inverse line.  The mirrored half re-reads values that this workgroup loads for
          // its own half as well (default cache policy, so that the second read is an L2 hit, not HBM traffic).  Without a
          // split the address is a per-lane base plus a uniform offset for either half; with one, block and offset of
          // N - n are not sums of per-lane and uniform parts, so they are computed per element.
          const bool lo = n <= N / 2;
          const int m = lo ? n : N - n;
          const V2 *p;
          if constexpr (PLAIN) p = lo ? p0 + (long long)cn * a.in_axis : pm + (long long)(N - cn) * a.in_axis;
          else {
            const int blk = m >> a.in_shift;
            p = src + (TAB ? a.in_tab[blk] : (long long)blk * a.in_blk) + (long long)(m & mask) * a.in_axis;
          }
          if (valid) val = *p;
          v[decltype(ii)::value] = cx<T>{val.x, xor_sign(val.y, lo ? conj_mask : conj_mask ^ 0x80000000u)};
        } else if constexpr (R2C && (HALF & 1) != 0 && cn >= N / 2) {
          v[decltype(ii)::value] = cx<T>{T{}, T{}};  // the padding of a real row: a literal zero, as on a complex line below
        } else if constexpr (R2C) {
          // n real values at the head of the row: element n is the n-th T of the row
          if constexpr (!PAIR) {
            if (valid) val.x = reinterpret_cast<const T *>(src)[n];
            v[decltype(ii)::value] = cx<T>{val.x, (T)0};
          }
        } else if constexpr ((HALF & 1) != 0 && cn >= N / 2) {
          v[decltype(ii)::value] = cx<T>{T{}, T{}};  // the padding: a literal zero (and the first butterfly knows it)
        } else {
          long long off = (long long)(cn & mask) * a.in_axis;  // uniform
          if constexpr (TAB) off += a.in_tab[jb + (cn >> a.in_shift)];
          else off += (long long)(cn >> a.in_shift) * a.in_blk;  // uniform
          if constexpr (PAIR) {
            T re, im;
            if constexpr (INC) {  // lanes along the line: one 8-B access per column
              const V2 w0 = gload(p0 + off), w1 = gload(p0 + off + a.in_col);
              re.x = w0.x; re.y = w1.x; im.x = w0.y; im.y = w1.y;
            } else {              // lanes across columns: the pair is 16 contiguous bytes
              const f32x4 q = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(p0 + off));
              re.x = q.x; im.x = q.y; re.y = q.z; im.y = q.w;
            }
            v[decltype(ii)::value] = cx<T>{re, xor_sign(im, conj_mask)};
          } else {
            if (valid) val = gload(p0 + off);
            v[decltype(ii)::value] = cx<T>{val.x, xor_sign(val.y, conj_mask)};
          }
        }
      });
    };
    if constexpr (C2R) {
      if (!a.in_split) load_all(std::false_type{}, std::true_type{});
      else if (a.in_tab) load_all(std::true_type{}, std::false_type{});
      else load_all(std::false_type{}, std::false_type{});
    } else {
      if (a.in_tab) load_all(std::true_type{}, std::false_type{});
      else load_all(std::false_type{}, std::false_type{});
    }
  }

  // ---------------- stages ---------------------------------------------------
  static_for<0, NSTAGE>([&](auto sidx) {
    constexpr int s = decltype(sidx)::value;
    constexpr int R = (s == 0) ? R0 : ((s == 1) ? R1 : R2);
    constexpr int Ns = (s == 0) ? 1 : ((s == 1) ? R0 : R0 * R1);
    constexpr int NB = E / R;           // butterflies per thread
    constexpr int LR = ilog2(R);

    if constexpr (s > 0) {
      // inter-stage twiddles w_N^(k * t * N/(Ns*R)), k = q mod Ns
      constexpr int M = N / (Ns * R);
      // the twiddle tables staged at kernel entry must be visible: exchange 0 had a workgroup barrier unless it was
      // wave-private
      if constexpr (s == 1 && (64 % TPL == 0) && (NT % 64 == 0) && INC && !(NSTAGE == 2 && !OUTC)) __syncthreads();
      static_for<0, NB>([&](auto uu) {
        constexpr int u = decltype(uu)::value;
        const int q = j + u * TPL;
        const int km = (q & (Ns - 1)) * M;
        static_for<1, R>([&](auto tt) {
          constexpr int t = decltype(tt)::value;
          S cr, ci;
          if constexpr (s == 1 && Cfg::USE_T1) {
            const V2 w = tw1[(t - 1) * R0 + (q & (R0 - 1))];  // consecutive lanes, consecutive entries
            cr = w.x; ci = w.y;
          } else if constexpr (Cfg::USE_HALF) {
            const int e = km * t;                              // < N
            const V2 w = tw[e & (N / 2 - 1)];
            const unsigned sm = ((unsigned)e << (32 - ilog2(N))) & 0x80000000u;  // bit log2(N)-1 of e: w^(e) = -w^(e - N/2)
            cr = xor_sign(w.x, sm); ci = xor_sign(w.y, sm);
          } else {
            const int e = km * t;
            const int qd = e / (N / 4);
            const int r = e & (N / 4 - 1);
            V2 w = tw[r];
            S wr = w.x, wi = w.y;
            // multiply by (-i)^qd
            cr = (qd & 1) ? wi : wr;
            ci = (qd & 1) ? -wr : wi;
            if (qd & 2) { cr = -cr; ci = -ci; }
          }
          cx<T> x = v[u * R + t];
          v[u * R + t] = cx<T>{x.x * cr - x.y * ci, x.x * ci + x.y * cr};
        });
      });
    }

    static_for<0, NB>([&](auto uu) { dft_reg<T, R, s == 0 && (HALF & 1) != 0>(&v[decltype(uu)::value * R]); });

    if constexpr (s < NSTAGE - 1) {
      // ---- exchange through LDS: write Stockham-ordered, read strided --------
      constexpr int Rn = (s == 0) ? R1 : R2;      // next radix
      constexpr bool next_last = (s + 1 == NSTAGE - 1);
      int cn, jn;                                  // reader mapping
      if constexpr (next_last && !OUTC) { cn = tid % COLS; jn = tid / COLS; }
      else                              { jn = tid % TPL; cn = tid / TPL; }

      auto wr_idx = [&](int u, int t) {
        const int q = j + u * TPL;
        const int k = q & (Ns - 1);
        return c * LSTRIDE + padidx<SWZ, PS>((q - k) * R + k + t * Ns);
      };
      auto rd_idx = [&](int u, int t) {
        return cn * LSTRIDE + padidx<SWZ, PS>(jn + u * TPL + t * (N / Rn));
      };

      // Synchronisation.  With lanes along the line (j = tid % TPL) and TPL a divisor of 64, a wave owns whole columns: it
      // writes and reads only its own columns' LDS image, DS operations of one wave execute in order, and no workgroup
      // barrier is needed -- waves drift apart and one wave's butterflies overlap another's LDS traffic.  Only an exchange
      // whose writer (stage 0 of a strided-in pass) or reader (last stage of a strided-out pass) runs lanes across
      // columns needs s_barrier.
      constexpr bool WAVE_COLS = (64 % TPL == 0) && (NT % 64 == 0);
      constexpr bool PRIV_W = WAVE_COLS && (s > 0 || INC);                 // writer mapping is wave-private
      constexpr bool PRIV = PRIV_W && !(next_last && !OUTC);              // ... and so is the reader's
      auto xsync = [&](auto priv) {
        if constexpr (decltype(priv)::value) {
          __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
          __builtin_amdgcn_wave_barrier();
        } else {
          __syncthreads();
        }
      };
      // previous exchange's reads done (its reader mapping is this exchange's writer mapping)
      if constexpr (s > 0) xsync(std::integral_constant<bool, PRIV_W>{});
      constexpr std::integral_constant<bool, PRIV> priv{};
      if constexpr (SPLIT) {
        static_for<0, E>([&](auto ii) {
          constexpr int u = decltype(ii)::value / R, t = decltype(ii)::value % R;
          exs[wr_idx(u, t)] = v[u * R + bitrev(t, LR)].x;
        });
        xsync(priv);
        T re[E];
        static_for<0, E>([&](auto ii) {
          constexpr int u = decltype(ii)::value / Rn, t = decltype(ii)::value % Rn;
          re[decltype(ii)::value] = exs[rd_idx(u, t)];
        });
        xsync(priv);
        static_for<0, E>([&](auto ii) {
          constexpr int u = decltype(ii)::value / R, t = decltype(ii)::value % R;
          exs[wr_idx(u, t)] = v[u * R + bitrev(t, LR)].y;
        });
        xsync(priv);
        static_for<0, E>([&](auto ii) {
          constexpr int u = decltype(ii)::value / Rn, t = decltype(ii)::value % Rn;
          v[decltype(ii)::value] = cx<T>{re[decltype(ii)::value], exs[rd_idx(u, t)]};
        });
      } else {
        static_for<0, E>([&](auto ii) {
          constexpr int u = decltype(ii)::value / R, t = decltype(ii)::value % R;
          cx<T> x = v[u * R + bitrev(t, LR)];
          XV w;
          if constexpr (PAIR) { w.x = x.x.x; w.y = x.x.y; w.z = x.y.x; w.w = x.y.y; }
          else { w.x = x.x; w.y = x.y; }
          exv[wr_idx(u, t)] = w;
        });
        xsync(priv);
        static_for<0, E>([&](auto ii) {
          constexpr int u = decltype(ii)::value / Rn, t = decltype(ii)::value % Rn;
          XV w = exv[rd_idx(u, t)];
          if constexpr (PAIR) { T re = {w.x, w.y}, im = {w.z, w.w}; v[decltype(ii)::value] = cx<T>{re, im}; }
          else v[decltype(ii)::value] = cx<T>{w.x, w.y};
        });
      }
      c = cn; j = jn;
    } else {
      // ---------------- last stage: global store ------------------------------
      const bool valid = (c0 + c * NL) < a.ncols;
      V2 *dst = out + (long long)b1 * a.out_b1 + (long long)b2 * a.out_b2 + (long long)(c0 + c * NL) * a.out_col;
      const int mask = (int)((1u << a.out_shift) - 1u);
      const S sc = (S)a.scale;
      const S scy = a.conj ? -sc : sc;  // conj-out rides on the scale
      auto store_all = [&](auto tabbed) {
        constexpr bool TAB = decltype(tabbed)::value;  // blocks from out_block_tab (see the load side)
        const int jb = j >> a.out_shift;
        V2 *p0 = dst + (TAB ? 0LL : (long long)jb * a.out_blk) + (long long)(j & mask) * a.out_axis;
        static_for<0, E>([&](auto ii) {
          constexpr int u = decltype(ii)::value / R, t = decltype(ii)::value % R;
          constexpr int cn = u * TPL + t * (N / R);
          if constexpr ((HALF & 2) != 0 && cn >= N / 2) return;  // the upper half of the output is not wanted
          const int n = j + cn;
          cx<T> x = v[u * R + bitrev(t, LR)];
          if constexpr (TW4) {
            // times w^(k1 j2) of the long line, before the conj-out / scale below (for the inverse conj(v w) = conj(v) conj(w))
            const long long jj = a.tw4_b1 ? b1 : (c0 + c);
            const V2 w = reinterpret_cast<const V2 *>(a.tw4)[(long long)n * a.tw4_n2 + jj];
            x = cx<T>{x.x * w.x - x.y * w.y, x.x * w.y + x.y * w.x};
          }
          long long off = (long long)(cn & mask) * a.out_axis;  // uniform
          if constexpr (TAB) off += a.out_tab[jb + (cn >> a.out_shift)];
          else off += (long long)(cn >> a.out_shift) * a.out_blk;  // uniform
          if constexpr (PAIR) {
            const T wx = x.x * sc, wy = x.y * scy;
            if constexpr (OUTC) {
              V2 w0, w1;
              w0.x = wx.x; w0.y = wy.x; w1.x = wx.y; w1.y = wy.y;
              if (valid) gstore_p<KEEP>(p0 + off, w0);
              if (valid) gstore_p<KEEP>(p0 + off + a.out_col, w1);
            } else {
              f32x4 q;
              q.x = wx.x; q.y = wy.x; q.z = wx.y; q.w = wy.y;
              if constexpr (KEEP) { if (valid) *reinterpret_cast<f32x4 *>(p0 + off) = q; }
              else { if (valid) __builtin_nontemporal_store(q, reinterpret_cast<f32x4 *>(p0 + off)); }
            }
          } else if constexpr (C2R) {
            // n reals at the head of the row (out_axis_stride = 1, no split): the real part of the line, scaled
            if (valid) __builtin_nontemporal_store(x.x * sc, reinterpret_cast<T *>(dst) + n);
            (void)off;
          } else {
            V2 w;
            w.x = x.x * sc;
            w.y = x.y * scy;
            if (valid && (!R2C || n <= N / 2)) gstore_p<KEEP>(p0 + off, w);
          }
        });
      };
      if (a.out_tab) store_all(std::true_type{});
      else store_all(std::false_type{});
    }
  });
}

template <typename T, int N, int E, int R0, int R1, int R2, int COLS, bool INC, bool OUTC, bool SPLIT, bool R2C = false,
          bool KEEP = false, bool TW4 = false>
__global__ void __launch_bounds__((N / E) * COLS, (PanelCfg<N, E, R0, R1, R2, COLS, SPLIT, T>::WPS_E))
fft_panel_k(PassArgs a, const typename vec2<T>::type *in, typename vec2<T>::type *out, const typename vec2<T>::type *twq) {
  panel_body<T, N, E, R0, R1, R2, COLS, INC, OUTC, SPLIT, R2C, KEEP, TW4, false>(a, in, out, twq);
}

// real-output z pass: contiguous rows on the store side, either flavour on the load side
template <typename T, int N, int E, int R0, int R1, int R2, int COLS, bool INC, bool SPLIT>
__global__ void __launch_bounds__((N / E) * COLS, (PanelCfg<N, E, R0, R1, R2, COLS, SPLIT, T>::WPS_E))
fft_c2r_panel_k(PassArgs a, const typename vec2<T>::type *in, typename vec2<T>::type *out, const typename vec2<T>::type *twq) {
  panel_body<T, N, E, R0, R1, R2, COLS, INC, true, SPLIT, false, false, false, true>(a, in, out, twq);
}

// zero-padded half lines (offt_pass_desc::half = HALF, 1 or 2): a kernel of its own name, so that no older symbol changes
template <typename T, int N, int E, int R0, int R1, int R2, int COLS, bool INC, bool OUTC, bool SPLIT, int HALF>
__global__ void __launch_bounds__((N / E) * COLS, (PanelCfg<N, E, R0, R1, R2, COLS, SPLIT, T>::WPS_E))
fft_half_panel_k(PassArgs a, const typename vec2<T>::type *in, typename vec2<T>::type *out, const typename vec2<T>::type *twq) {
  panel_body<T, N, E, R0, R1, R2, COLS, INC, OUTC, SPLIT, false, false, false, false, HALF>(a, in, out, twq);
}

// the real ends of a half-box chain on a real-input plan (offt_pass_desc::real_input with ::half), names of their own again:
// the real-input z pass that does not load the reals n >= N/2 (contiguous rows in, strided out) ...
template <typename T, int N, int E, int R0, int R1, int R2, int COLS, bool SPLIT>
__global__ void __launch_bounds__((N / E) * COLS, (PanelCfg<N, E, R0, R1, R2, COLS, SPLIT, T>::WPS_E))
fft_half_r2c_panel_k(PassArgs a, const typename vec2<T>::type *in, typename vec2<T>::type *out, const typename vec2<T>::type *twq) {
  panel_body<T, N, E, R0, R1, R2, COLS, true, false, SPLIT, true, false, false, false, 1>(a, in, out, twq);
}
// ... and its mirror image, the real-output z pass that does not store them (strided in, contiguous rows out)
template <typename T, int N, int E, int R0, int R1, int R2, int COLS, bool SPLIT>
__global__ void __launch_bounds__((N / E) * COLS, (PanelCfg<N, E, R0, R1, R2, COLS, SPLIT, T>::WPS_E))
fft_half_c2r_panel_k(PassArgs a, const typename vec2<T>::type *in, typename vec2<T>::type *out, const typename vec2<T>::type *twq) {
  panel_body<T, N, E, R0, R1, R2, COLS, false, true, SPLIT, false, false, false, true, 2>(a, in, out, twq);
}

// ---------------------------------------------------------------------------
// Spectral convolution of whole lines (offt_hipk_conv_pass): load a panel, forward stages, multiply every output by the
// filter, conjugate, one LDS round trip back into the load distribution, the stages again (an inverse by conj-in /
// conj-out), conjugate, scale, store where the lines came from.  The last pass of a forward 3-D transform and the first
// pass of the inverse work on the same lines: one launch instead of two, and no sweep for the multiply.
// Only the contiguous-line flavour (lanes along the line on both sides, no split, one column per lane): with it the
// thread mapping (column c = tid / TPL, line offset j = tid % TPL) is the same in every stage, so the exchanges are those
// of panel_body's contiguous / contiguous kernels.  In place: a workgroup owns whole lines and has loaded all of them
// before its first exchange, i.e. before any of its stores.
struct ConvArgs {
  long long axis, col, b1, b2;  // filter strides in complex elements (the forward pass's store side)
  int cplx;                     // 1: one complex value per element, 0: one real scalar per complex slot (same element index)
};

// HALF (fft_conv_half_panel_k, offt_pass_desc::half = 3): the lines are zero above N/2 going in and only their lower half
// is wanted coming out -- the upper half is neither loaded nor stored (compile-time, as in panel_body); the filter and
// everything between the two is the full line
// The lines are loaded from `data` and stored at the same offsets from `dst`: the in-place kernels pass one pointer twice,
// the out-of-place ones (fft_conv_oop_panel_k, offt_hipk_conv_pass_oop) a second volume, and never write the first.
template <typename T, int N, int E, int R0, int R1, int R2, int COLS, bool SPLIT, bool KEEP, bool HALF = false>
__device__ __forceinline__ void conv_body(PassArgs a, ConvArgs f, const typename vec2<T>::type *data, typename vec2<T>::type *dst,
                                          const void *filter, const typename vec2<T>::type *twq) {
  using V2 = typename vec2<T>::type;
  using Cfg = PanelCfg<N, E, R0, R1, R2, COLS, SPLIT, T>;
  constexpr int TPL = Cfg::TPL, NT = Cfg::NT, NSTAGE = Cfg::NSTAGE;
  constexpr int LSTRIDE = Cfg::LSTRIDE;
  constexpr bool SWZ = Cfg::SWZ;
  constexpr int PS = SWZ ? Cfg::SWZSHIFT : Cfg::PADSHIFT;
  static_assert(R0 * R1 * R2 == N, "radices must multiply to N");
  static_assert(E % R0 == 0 && E % R1 == 0 && E % R2 == 0 && N % E == 0, "bad E");
  static_assert(NSTAGE > 1, "the round trip goes through the exchange image");
  constexpr int RL = NSTAGE == 3 ? R2 : R1;  // radix of the last stage
  constexpr int LRL = ilog2(RL);

  extern __shared__ __align__(16) unsigned char smem[];
  T *exs = reinterpret_cast<T *>(smem);
  V2 *exv = reinterpret_cast<V2 *>(smem);
  V2 *tw = reinterpret_cast<V2 *>(smem + Cfg::TW_OFF);
  V2 *tw1 = reinterpret_cast<V2 *>(smem + Cfg::T1_OFF);

  const int tid = threadIdx.x;
  for (int i = tid; i < Cfg::QT; i += NT) tw[i] = twq[i];
  if constexpr (Cfg::USE_T1) {
    constexpr int M1 = N / (R0 * R1);
    for (int i = tid; i < Cfg::T1N; i += NT) {
      const int t = i / R0 + 1, k = i - (t - 1) * R0;
      tw1[i] = twq[k * M1 * t];
    }
  }

  const unsigned bid = panel_of_block(blockIdx.x, a.xcd_lim, a.xcd_gshift);
  const int cp = bid % (unsigned)a.ncp;
  const unsigned rest = bid / (unsigned)a.ncp;
  const int b1 = rest % (unsigned)a.nb1;
  const int b2 = rest / (unsigned)a.nb1;
  const int c0 = cp * COLS;
  const int j = tid % TPL, c = tid / TPL;
  const bool valid = (c0 + c) < a.ncols;
  const long long lo = (long long)b1 * a.in_b1 + (long long)b2 * a.in_b2 + (long long)(c0 + c) * a.in_col + (long long)j * a.in_axis;
  const V2 *line = data + lo;
  V2 *sline = dst + lo;
  const long long fb = (long long)b1 * f.b1 + (long long)b2 * f.b2 + (long long)(c0 + c) * f.col + (long long)j * f.axis;

  // a wave owns whole columns when TPL divides 64: its exchanges need no workgroup barrier (see panel_body)
  constexpr bool WAVE_COLS = (64 % TPL == 0) && (NT % 64 == 0);
  auto xsync = [&]() {
    if constexpr (WAVE_COLS) {
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
    } else {
      __syncthreads();
    }
  };
  auto at = [&](int i) { return c * LSTRIDE + padidx<SWZ, PS>(i); };

  cx<T> v[E];
  static_for<0, E>([&](auto ii) {
    constexpr int u = decltype(ii)::value / R0, t = decltype(ii)::value % R0;
    constexpr int cn = u * TPL + t * (N / R0);
    V2 val;
    val.x = 0; val.y = 0;
    if constexpr (!(HALF && cn >= N / 2)) {
      if (valid) val = gload(line + (long long)cn * a.in_axis);
    }
    v[decltype(ii)::value] = cx<T>{val.x, val.y};
  });

  // the forward stages of panel_body (contiguous / contiguous), ending in the last stage's register order:
  // v[u RL + bitrev(t)] holds line index j + u TPL + t N/RL
  auto stages = [&](auto upper_zero) {
    static_for<0, NSTAGE>([&](auto sidx) {
      constexpr int s = decltype(sidx)::value;
      constexpr int R = (s == 0) ? R0 : ((s == 1) ? R1 : R2);
      constexpr int Ns = (s == 0) ? 1 : ((s == 1) ? R0 : R0 * R1);
      constexpr int NB = E / R;
      constexpr int LR = ilog2(R);
      if constexpr (s > 0) {
        constexpr int M = N / (Ns * R);
        if constexpr (s == 1 && WAVE_COLS) __syncthreads();  // the twiddle tables staged at entry are visible
        static_for<0, NB>([&](auto uu) {
          constexpr int u = decltype(uu)::value;
          const int q = j + u * TPL;
          const int km = (q & (Ns - 1)) * M;
          static_for<1, R>([&](auto tt) {
            constexpr int t = decltype(tt)::value;
            T cr, ci;
            if constexpr (s == 1 && Cfg::USE_T1) {
              const V2 w = tw1[(t - 1) * R0 + (q & (R0 - 1))];
              cr = w.x; ci = w.y;
            } else if constexpr (Cfg::USE_HALF) {
              const int e = km * t;
              const V2 w = tw[e & (N / 2 - 1)];
              const unsigned sm = ((unsigned)e << (32 - ilog2(N))) & 0x80000000u;
              cr = xor_sign(w.x, sm); ci = xor_sign(w.y, sm);
            } else {
              const int e = km * t;
              const int qd = e / (N / 4);
              const V2 w = tw[e & (N / 4 - 1)];
              cr = (qd & 1) ? w.y : w.x;
              ci = (qd & 1) ? -w.x : w.y;
              if (qd & 2) { cr = -cr; ci = -ci; }
            }
            const cx<T> x = v[u * R + t];
            v[u * R + t] = cx<T>{x.x * cr - x.y * ci, x.x * ci + x.y * cr};
          });
        });
      }
      static_for<0, NB>([&](auto uu) { dft_reg<T, R, s == 0 && decltype(upper_zero)::value>(&v[decltype(uu)::value * R]); });
      if constexpr (s < NSTAGE - 1) {
        constexpr int Rn = (s == 0) ? R1 : R2;
        auto wr_idx = [&](int u, int t) {
          const int q = j + u * TPL;
          const int k = q & (Ns - 1);
          return at((q - k) * R + k + t * Ns);
        };
        auto rd_idx = [&](int u, int t) { return at(j + u * TPL + t * (N / Rn)); };
        if constexpr (s > 0) xsync();  // previous exchange's reads done
        if constexpr (SPLIT) {
          static_for<0, E>([&](auto ii) {
            constexpr int u = decltype(ii)::value / R, t = decltype(ii)::value % R;
            exs[wr_idx(u, t)] = v[u * R + bitrev(t, LR)].x;
          });
          xsync();
          T re[E];
          static_for<0, E>([&](auto ii) {
            constexpr int u = decltype(ii)::value / Rn, t = decltype(ii)::value % Rn;
            re[decltype(ii)::value] = exs[rd_idx(u, t)];
          });
          xsync();
          static_for<0, E>([&](auto ii) {
            constexpr int u = decltype(ii)::value / R, t = decltype(ii)::value % R;
            exs[wr_idx(u, t)] = v[u * R + bitrev(t, LR)].y;
          });
          xsync();
          static_for<0, E>([&](auto ii) {
            constexpr int u = decltype(ii)::value / Rn, t = decltype(ii)::value % Rn;
            v[decltype(ii)::value] = cx<T>{re[decltype(ii)::value], exs[rd_idx(u, t)]};
          });
        } else {
          static_for<0, E>([&](auto ii) {
            constexpr int u = decltype(ii)::value / R, t = decltype(ii)::value % R;
            const cx<T> x = v[u * R + bitrev(t, LR)];
            V2 w; w.x = x.x; w.y = x.y;
            exv[wr_idx(u, t)] = w;
          });
          xsync();
          static_for<0, E>([&](auto ii) {
            constexpr int u = decltype(ii)::value / Rn, t = decltype(ii)::value % Rn;
            const V2 w = exv[rd_idx(u, t)];
            v[decltype(ii)::value] = cx<T>{w.x, w.y};
          });
        }
      }
    });
  };

  stages(std::integral_constant<bool, HALF>{});

  // times H[n], then conjugated (the inverse as conj(F(conj(.)))); filter values are read once: non-temporal
  auto filt = [&](auto complex_filter) {
    static_for<0, E>([&](auto ii) {
      constexpr int u = decltype(ii)::value / RL, t = decltype(ii)::value % RL;
      constexpr int cn = u * TPL + t * (N / RL);
      const int r = u * RL + bitrev(t, LRL);
      const long long off = fb + (long long)cn * f.axis;
      const cx<T> x = v[r];
      if constexpr (decltype(complex_filter)::value) {
        V2 h;
        h.x = 0; h.y = 0;
        if (valid) h = gload(reinterpret_cast<const V2 *>(filter) + off);
        v[r] = cx<T>{x.x * h.x - x.y * h.y, -(x.x * h.y + x.y * h.x)};
      } else {
        T h = 0;
        if (valid) h = __builtin_nontemporal_load(reinterpret_cast<const T *>(filter) + off);
        v[r] = cx<T>{x.x * h, -(x.y * h)};
      }
    });
  };
  if (f.cplx) filt(std::true_type{});
  else filt(std::false_type{});

  // round trip through the exchange image: from the last stage's order back into the load distribution
  xsync();  // the last exchange's reads done
  if constexpr (SPLIT) {
    T re[E];
    static_for<0, E>([&](auto ii) {
      constexpr int u = decltype(ii)::value / RL, t = decltype(ii)::value % RL;
      exs[at(j + u * TPL + t * (N / RL))] = v[u * RL + bitrev(t, LRL)].x;
    });
    xsync();
    static_for<0, E>([&](auto ii) {
      constexpr int u = decltype(ii)::value / R0, t = decltype(ii)::value % R0;
      re[decltype(ii)::value] = exs[at(j + u * TPL + t * (N / R0))];
    });
    xsync();
    static_for<0, E>([&](auto ii) {
      constexpr int u = decltype(ii)::value / RL, t = decltype(ii)::value % RL;
      exs[at(j + u * TPL + t * (N / RL))] = v[u * RL + bitrev(t, LRL)].y;
    });
    xsync();
    static_for<0, E>([&](auto ii) {
      constexpr int u = decltype(ii)::value / R0, t = decltype(ii)::value % R0;
      v[decltype(ii)::value] = cx<T>{re[decltype(ii)::value], exs[at(j + u * TPL + t * (N / R0))]};
    });
  } else {
    static_for<0, E>([&](auto ii) {
      constexpr int u = decltype(ii)::value / RL, t = decltype(ii)::value % RL;
      const cx<T> x = v[u * RL + bitrev(t, LRL)];
      V2 w; w.x = x.x; w.y = x.y;
      exv[at(j + u * TPL + t * (N / RL))] = w;
    });
    xsync();
    static_for<0, E>([&](auto ii) {
      constexpr int u = decltype(ii)::value / R0, t = decltype(ii)::value % R0;
      const V2 w = exv[at(j + u * TPL + t * (N / R0))];
      v[decltype(ii)::value] = cx<T>{w.x, w.y};
    });
  }
  xsync();  // the round trip's reads done before the first exchange of the second half writes

  stages(std::false_type{});

  const T sc = (T)a.scale;
  static_for<0, E>([&](auto ii) {
    constexpr int u = decltype(ii)::value / RL, t = decltype(ii)::value % RL;
    constexpr int cn = u * TPL + t * (N / RL);
    if constexpr (HALF && cn >= N / 2) return;
    const cx<T> x = v[u * RL + bitrev(t, LRL)];
    V2 w;
    w.x = x.x * sc;
    w.y = -x.y * sc;
    if (valid) gstore_p<KEEP>(sline + (long long)cn * a.in_axis, w);
  });
}

// (the filter values and the second half's live ranges cost registers the plain pass does not need: at most 2 waves per
//  SIMD, 256 VGPRs, so that no instance spills)
template <typename T, int N, int E, int R0, int R1, int R2, int COLS, bool SPLIT>
constexpr int conv_wps() { return PanelCfg<N, E, R0, R1, R2, COLS, SPLIT, T>::WPS_E < 2 ? PanelCfg<N, E, R0, R1, R2, COLS, SPLIT, T>::WPS_E : 2; }

template <typename T, int N, int E, int R0, int R1, int R2, int COLS, bool SPLIT, bool KEEP = false>
__global__ void __launch_bounds__((N / E) * COLS, (conv_wps<T, N, E, R0, R1, R2, COLS, SPLIT>()))
fft_conv_panel_k(PassArgs a, ConvArgs f, typename vec2<T>::type *data, const void *filter, const typename vec2<T>::type *twq) {
  conv_body<T, N, E, R0, R1, R2, COLS, SPLIT, KEEP>(a, f, data, data, filter, twq);
}

template <typename T, int N, int E, int R0, int R1, int R2, int COLS, bool SPLIT, bool KEEP = false>
__global__ void __launch_bounds__((N / E) * COLS, (conv_wps<T, N, E, R0, R1, R2, COLS, SPLIT>()))
fft_conv_half_panel_k(PassArgs a, ConvArgs f, typename vec2<T>::type *data, const void *filter, const typename vec2<T>::type *twq) {
  conv_body<T, N, E, R0, R1, R2, COLS, SPLIT, KEEP, true>(a, f, data, data, filter, twq);
}

// out of place (offt_hipk_conv_pass_oop): the lines of `src` convolved into `dst` at the same offsets, `src` left as it
// was -- the multi-output convolution applies several filters to one spectrum.  Kernels of their own names: the in-place
// symbols above stay what they were.
template <typename T, int N, int E, int R0, int R1, int R2, int COLS, bool SPLIT, bool KEEP = false>
__global__ void __launch_bounds__((N / E) * COLS, (conv_wps<T, N, E, R0, R1, R2, COLS, SPLIT>()))
fft_conv_oop_panel_k(PassArgs a, ConvArgs f, const typename vec2<T>::type *src, typename vec2<T>::type *dst, const void *filter,
                     const typename vec2<T>::type *twq) {
  conv_body<T, N, E, R0, R1, R2, COLS, SPLIT, KEEP>(a, f, src, dst, filter, twq);
}

template <typename T, int N, int E, int R0, int R1, int R2, int COLS, bool SPLIT, bool KEEP = false>
__global__ void __launch_bounds__((N / E) * COLS, (conv_wps<T, N, E, R0, R1, R2, COLS, SPLIT>()))
fft_conv_oop_half_panel_k(PassArgs a, ConvArgs f, const typename vec2<T>::type *src, typename vec2<T>::type *dst, const void *filter,
                          const typename vec2<T>::type *twq) {
  conv_body<T, N, E, R0, R1, R2, COLS, SPLIT, KEEP, true>(a, f, src, dst, filter, twq);
}

// ---------------------------------------------------------------------------
// Filtered forward and filtered inverse of whole lines (offt_hipk_filt_pass_fwd, offt_hipk_filt_pass_inv): the two halves of
// conv_body as kernels of their own, for a caller whose state lives in spectral space.  Contiguous lines, no split, one
// column per lane, conv_body's thread mapping (column c = tid / TPL, line offset j = tid % TPL in every stage).
//   INV = false (fft_filt_fwd_panel_k): load, forward stages, H[n] times the register that holds output index n, scale,
//     store where the line came from -- the x pass of a forward transform with the multiply on its stores.  In place.
//   INV = true (fft_filt_inv_panel_k): load from `src`, H[n] loaded with the element's own index and multiplied in the load
//     distribution, conjugate, the stages, conjugate, scale, store to `dst` at the same offsets -- the x pass of an inverse
//     transform with the multiply on its loads.  `src` is not written unless dst == src (a workgroup owns whole lines and has
//     loaded all of them before its first exchange, i.e. before any of its stores).
// No round trip through the exchange image: each half multiplies in the distribution it already has.  Filter values are
// read once: non-temporal.
template <typename T, int N, int E, int R0, int R1, int R2, int COLS, bool SPLIT, bool KEEP, bool INV>
__device__ __forceinline__ void filt_body(PassArgs a, ConvArgs f, const typename vec2<T>::type *src, typename vec2<T>::type *dst,
                                          const void *filter, const typename vec2<T>::type *twq) {
  using V2 = typename vec2<T>::type;
  using Cfg = PanelCfg<N, E, R0, R1, R2, COLS, SPLIT, T>;
  constexpr int TPL = Cfg::TPL, NT = Cfg::NT, NSTAGE = Cfg::NSTAGE;
  constexpr int LSTRIDE = Cfg::LSTRIDE;
  constexpr bool SWZ = Cfg::SWZ;
  constexpr int PS = SWZ ? Cfg::SWZSHIFT : Cfg::PADSHIFT;
  static_assert(R0 * R1 * R2 == N, "radices must multiply to N");
  static_assert(E % R0 == 0 && E % R1 == 0 && E % R2 == 0 && N % E == 0, "bad E");
  static_assert(NSTAGE > 1, "the twiddle tables are staged for the exchanges");
  constexpr int RL = NSTAGE == 3 ? R2 : R1;  // radix of the last stage
  constexpr int LRL = ilog2(RL);

  extern __shared__ __align__(16) unsigned char smem[];
  T *exs = reinterpret_cast<T *>(smem);
  V2 *exv = reinterpret_cast<V2 *>(smem);
  V2 *tw = reinterpret_cast<V2 *>(smem + Cfg::TW_OFF);
  V2 *tw1 = reinterpret_cast<V2 *>(smem + Cfg::T1_OFF);

  const int tid = threadIdx.x;
  for (int i = tid; i < Cfg::QT; i += NT) tw[i] = twq[i];
  if constexpr (Cfg::USE_T1) {
    constexpr int M1 = N / (R0 * R1);
    for (int i = tid; i < Cfg::T1N; i += NT) {
      const int t = i / R0 + 1, k = i - (t - 1) * R0;
      tw1[i] = twq[k * M1 * t];
    }
  }

  const unsigned bid = panel_of_block(blockIdx.x, a.xcd_lim, a.xcd_gshift);
  const int cp = bid % (unsigned)a.ncp;
  const unsigned rest = bid / (unsigned)a.ncp;
  const int b1 = rest % (unsigned)a.nb1;
  const int b2 = rest / (unsigned)a.nb1;
  const int c0 = cp * COLS;
  const int j = tid % TPL, c = tid / TPL;
  const bool valid = (c0 + c) < a.ncols;
  const long long lo = (long long)b1 * a.in_b1 + (long long)b2 * a.in_b2 + (long long)(c0 + c) * a.in_col + (long long)j * a.in_axis;
  const V2 *line = src + lo;
  V2 *sline = dst + lo;
  const long long fb = (long long)b1 * f.b1 + (long long)b2 * f.b2 + (long long)(c0 + c) * f.col + (long long)j * f.axis;

  // a wave owns whole columns when TPL divides 64: its exchanges need no workgroup barrier (see panel_body)
  constexpr bool WAVE_COLS = (64 % TPL == 0) && (NT % 64 == 0);
  auto xsync = [&]() {
    if constexpr (WAVE_COLS) {
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
    } else {
      __syncthreads();
    }
  };
  auto at = [&](int i) { return c * LSTRIDE + padidx<SWZ, PS>(i); };

  // register r holds line index j + cn: times H at that index (a lane past the last column multiplies by zero and stores nothing)
  auto times_h = [&](cx<T> x, int cn, auto complex_filter) {
    const long long off = fb + (long long)cn * f.axis;
    if constexpr (decltype(complex_filter)::value) {
      V2 h;
      h.x = 0; h.y = 0;
      if (valid) h = gload(reinterpret_cast<const V2 *>(filter) + off);
      return cx<T>{x.x * h.x - x.y * h.y, x.x * h.y + x.y * h.x};
    } else {
      T h = 0;
      if (valid) h = __builtin_nontemporal_load(reinterpret_cast<const T *>(filter) + off);
      return cx<T>{x.x * h, x.y * h};
    }
  };

  cx<T> v[E];
  static_for<0, E>([&](auto ii) {
    constexpr int u = decltype(ii)::value / R0, t = decltype(ii)::value % R0;
    constexpr int cn = u * TPL + t * (N / R0);
    V2 val;
    val.x = 0; val.y = 0;
    if (valid) val = gload(line + (long long)cn * a.in_axis);
    v[decltype(ii)::value] = cx<T>{val.x, val.y};
  });
  if constexpr (INV) {
    // H in the load distribution, then conjugated (the inverse as conj(F(conj(.))))
    auto filt = [&](auto complex_filter) {
      static_for<0, E>([&](auto ii) {
        constexpr int u = decltype(ii)::value / R0, t = decltype(ii)::value % R0;
        constexpr int cn = u * TPL + t * (N / R0);
        const cx<T> x = times_h(v[decltype(ii)::value], cn, complex_filter);
        v[decltype(ii)::value] = cx<T>{x.x, -x.y};
      });
    };
    if (f.cplx) filt(std::true_type{});
    else filt(std::false_type{});
  }

  // the forward stages of panel_body (contiguous / contiguous), ending in the last stage's register order:
  // v[u RL + bitrev(t)] holds line index j + u TPL + t N/RL
  static_for<0, NSTAGE>([&](auto sidx) {
    constexpr int s = decltype(sidx)::value;
    constexpr int R = (s == 0) ? R0 : ((s == 1) ? R1 : R2);
    constexpr int Ns = (s == 0) ? 1 : ((s == 1) ? R0 : R0 * R1);
    constexpr int NB = E / R;
    constexpr int LR = ilog2(R);
    if constexpr (s > 0) {
      constexpr int M = N / (Ns * R);
      if constexpr (s == 1 && WAVE_COLS) __syncthreads();  // the twiddle tables staged at entry are visible
      static_for<0, NB>([&](auto uu) {
        constexpr int u = decltype(uu)::value;
        const int q = j + u * TPL;
        const int km = (q & (Ns - 1)) * M;
        static_for<1, R>([&](auto tt) {
          constexpr int t = decltype(tt)::value;
          T cr, ci;
          if constexpr (s == 1 && Cfg::USE_T1) {
            const V2 w = tw1[(t - 1) * R0 + (q & (R0 - 1))];
            cr = w.x; ci = w.y;
          } else if constexpr (Cfg::USE_HALF) {
            const int e = km * t;
            const V2 w = tw[e & (N / 2 - 1)];
            const unsigned sm = ((unsigned)e << (32 - ilog2(N))) & 0x80000000u;
            cr = xor_sign(w.x, sm); ci = xor_sign(w.y, sm);
          } else {
            const int e = km * t;
            const int qd = e / (N / 4);
            const V2 w = tw[e & (N / 4 - 1)];
            cr = (qd & 1) ? w.y : w.x;
            ci = (qd & 1) ? -w.x : w.y;
            if (qd & 2) { cr = -cr; ci = -ci; }
          }
          const cx<T> x = v[u * R + t];
          v[u * R + t] = cx<T>{x.x * cr - x.y * ci, x.x * ci + x.y * cr};
        });
      });
    }
    static_for<0, NB>([&](auto uu) { dft_reg<T, R>(&v[decltype(uu)::value * R]); });
    if constexpr (s < NSTAGE - 1) {
      constexpr int Rn = (s == 0) ? R1 : R2;
      auto wr_idx = [&](int u, int t) {
        const int q = j + u * TPL;
        const int k = q & (Ns - 1);
        return at((q - k) * R + k + t * Ns);
      };
      auto rd_idx = [&](int u, int t) { return at(j + u * TPL + t * (N / Rn)); };
      if constexpr (s > 0) xsync();  // previous exchange's reads done
      if constexpr (SPLIT) {
        static_for<0, E>([&](auto ii) {
          constexpr int u = decltype(ii)::value / R, t = decltype(ii)::value % R;
          exs[wr_idx(u, t)] = v[u * R + bitrev(t, LR)].x;
        });
        xsync();
        T re[E];
        static_for<0, E>([&](auto ii) {
          constexpr int u = decltype(ii)::value / Rn, t = decltype(ii)::value % Rn;
          re[decltype(ii)::value] = exs[rd_idx(u, t)];
        });
        xsync();
        static_for<0, E>([&](auto ii) {
          constexpr int u = decltype(ii)::value / R, t = decltype(ii)::value % R;
          exs[wr_idx(u, t)] = v[u * R + bitrev(t, LR)].y;
        });
        xsync();
        static_for<0, E>([&](auto ii) {
          constexpr int u = decltype(ii)::value / Rn, t = decltype(ii)::value % Rn;
          v[decltype(ii)::value] = cx<T>{re[decltype(ii)::value], exs[rd_idx(u, t)]};
        });
      } else {
        static_for<0, E>([&](auto ii) {
          constexpr int u = decltype(ii)::value / R, t = decltype(ii)::value % R;
          const cx<T> x = v[u * R + bitrev(t, LR)];
          V2 w; w.x = x.x; w.y = x.y;
          exv[wr_idx(u, t)] = w;
        });
        xsync();
        static_for<0, E>([&](auto ii) {
          constexpr int u = decltype(ii)::value / Rn, t = decltype(ii)::value % Rn;
          const V2 w = exv[rd_idx(u, t)];
          v[decltype(ii)::value] = cx<T>{w.x, w.y};
        });
      }
    }
  });

  // the last stage's order: forward times H[n] at the output index; inverse conjugated back; scale; store
  const T sc = (T)a.scale;
  auto store_all = [&](auto complex_filter) {
    static_for<0, E>([&](auto ii) {
      constexpr int u = decltype(ii)::value / RL, t = decltype(ii)::value % RL;
      constexpr int cn = u * TPL + t * (N / RL);
      cx<T> x = v[u * RL + bitrev(t, LRL)];
      V2 w;
      if constexpr (INV) {
        w.x = x.x * sc;
        w.y = -x.y * sc;
      } else {
        x = times_h(x, cn, complex_filter);
        w.x = x.x * sc;
        w.y = x.y * sc;
      }
      if (valid) gstore_p<KEEP>(sline + (long long)cn * a.in_axis, w);
    });
  };
  if (!INV && f.cplx) store_all(std::true_type{});
  else store_all(std::false_type{});
}

// (one transform plus the filter values: the plain pass's waves per SIMD, no instance spills -- the VGPR table is in DESIGN.md 4.5)
template <typename T, int N, int E, int R0, int R1, int R2, int COLS, bool SPLIT, bool KEEP = false>
__global__ void __launch_bounds__((N / E) * COLS, (PanelCfg<N, E, R0, R1, R2, COLS, SPLIT, T>::WPS_E))
fft_filt_fwd_panel_k(PassArgs a, ConvArgs f, typename vec2<T>::type *data, const void *filter, const typename vec2<T>::type *twq) {
  filt_body<T, N, E, R0, R1, R2, COLS, SPLIT, KEEP, false>(a, f, data, data, filter, twq);
}

template <typename T, int N, int E, int R0, int R1, int R2, int COLS, bool SPLIT, bool KEEP = false>
__global__ void __launch_bounds__((N / E) * COLS, (PanelCfg<N, E, R0, R1, R2, COLS, SPLIT, T>::WPS_E))
fft_filt_inv_panel_k(PassArgs a, ConvArgs f, const typename vec2<T>::type *src, typename vec2<T>::type *dst, const void *filter,
                     const typename vec2<T>::type *twq) {
  filt_body<T, N, E, R0, R1, R2, COLS, SPLIT, KEEP, true>(a, f, src, dst, filter, twq);
}

// ---------------------------------------------------------------------------
// Multi-input spectral convolution (offt_hipk_conv_pass_sum): out = ifft( sum_k H_k . fft(x_k) ) on whole lines.  The
// transpose of the out-of-place kernels above: several sources, one destination.  By linearity the K inverse transforms are
// one, and the sum lives in registers between the forward stages and the inverse stages -- conv_body with its first half
// in a loop over the inputs.  Per workgroup, for k = 0 ... nin-1: load the panel from src[k] (conv_body's loads), forward
// stages, times H_k in the last stage's register order, added into acc[E] in that order (k ascending: the same bits on
// every run); then conjugate, the one LDS round trip, the stages again, conjugate, scale, store to dst at the load offsets.
// In place on any ONE source: a workgroup owns whole lines and has loaded them from every source before its only stores.
// The pointers travel by value.  k is workgroup-uniform, and the two tables are read through a chain of compares on
// compile-time indices (sum_pick), so that they stay in scalar registers: indexed by k they would be copied to scratch.
#define OFFT_CONV_SUM_MAX 8
struct SumArgs {
  const void *src[OFFT_CONV_SUM_MAX];
  const void *filter[OFFT_CONV_SUM_MAX];
  int nin;
};
__device__ __forceinline__ const void *sum_pick(const void *const (&p)[OFFT_CONV_SUM_MAX], int k) {
  const void *r = p[0];
  static_for<1, OFFT_CONV_SUM_MAX>([&](auto ii) {
    if (k == decltype(ii)::value) r = p[decltype(ii)::value];
  });
  return r;
}

template <typename T, int N, int E, int R0, int R1, int R2, int COLS, bool SPLIT, bool KEEP, bool HALF = false>
__device__ __forceinline__ void conv_sum_body(PassArgs a, ConvArgs f, SumArgs sa, typename vec2<T>::type *dst,
                                              const typename vec2<T>::type *twq) {
  using V2 = typename vec2<T>::type;
  using Cfg = PanelCfg<N, E, R0, R1, R2, COLS, SPLIT, T>;
  constexpr int TPL = Cfg::TPL, NT = Cfg::NT, NSTAGE = Cfg::NSTAGE;
  constexpr int LSTRIDE = Cfg::LSTRIDE;
  constexpr bool SWZ = Cfg::SWZ;
  constexpr int PS = SWZ ? Cfg::SWZSHIFT : Cfg::PADSHIFT;
  static_assert(R0 * R1 * R2 == N, "radices must multiply to N");
  static_assert(E % R0 == 0 && E % R1 == 0 && E % R2 == 0 && N % E == 0, "bad E");
  static_assert(NSTAGE > 1, "the round trip goes through the exchange image");
  constexpr int RL = NSTAGE == 3 ? R2 : R1;  // radix of the last stage
  constexpr int LRL = ilog2(RL);

  extern __shared__ __align__(16) unsigned char smem[];
  T *exs = reinterpret_cast<T *>(smem);
  V2 *exv = reinterpret_cast<V2 *>(smem);
  V2 *tw = reinterpret_cast<V2 *>(smem + Cfg::TW_OFF);
  V2 *tw1 = reinterpret_cast<V2 *>(smem + Cfg::T1_OFF);

  const int tid = threadIdx.x;
  for (int i = tid; i < Cfg::QT; i += NT) tw[i] = twq[i];
  if constexpr (Cfg::USE_T1) {
    constexpr int M1 = N / (R0 * R1);
    for (int i = tid; i < Cfg::T1N; i += NT) {
      const int t = i / R0 + 1, k = i - (t - 1) * R0;
      tw1[i] = twq[k * M1 * t];
    }
  }
  __syncthreads();  // the twiddle tables are visible (once, ahead of the loop over the inputs)

  const unsigned bid = panel_of_block(blockIdx.x, a.xcd_lim, a.xcd_gshift);
  const int cp = bid % (unsigned)a.ncp;
  const unsigned rest = bid / (unsigned)a.ncp;
  const int b1 = rest % (unsigned)a.nb1;
  const int b2 = rest / (unsigned)a.nb1;
  const int c0 = cp * COLS;
  const int j = tid % TPL, c = tid / TPL;
  const bool valid = (c0 + c) < a.ncols;
  const long long lo = (long long)b1 * a.in_b1 + (long long)b2 * a.in_b2 + (long long)(c0 + c) * a.in_col + (long long)j * a.in_axis;
  const long long fb = (long long)b1 * f.b1 + (long long)b2 * f.b2 + (long long)(c0 + c) * f.col + (long long)j * f.axis;

  // a wave owns whole columns when TPL divides 64: its exchanges need no workgroup barrier (see panel_body)
  constexpr bool WAVE_COLS = (64 % TPL == 0) && (NT % 64 == 0);
  auto xsync = [&]() {
    if constexpr (WAVE_COLS) {
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
    } else {
      __syncthreads();
    }
  };
  auto at = [&](int i) { return c * LSTRIDE + padidx<SWZ, PS>(i); };

  cx<T> v[E];

  // conv_body's stages (contiguous / contiguous), ending in the last stage's register order:
  // v[u RL + bitrev(t)] holds line index j + u TPL + t N/RL
  auto stages = [&](auto upper_zero) {
    static_for<0, NSTAGE>([&](auto sidx) {
      constexpr int s = decltype(sidx)::value;
      constexpr int R = (s == 0) ? R0 : ((s == 1) ? R1 : R2);
      constexpr int Ns = (s == 0) ? 1 : ((s == 1) ? R0 : R0 * R1);
      constexpr int NB = E / R;
      constexpr int LR = ilog2(R);
      if constexpr (s > 0) {
        constexpr int M = N / (Ns * R);
        static_for<0, NB>([&](auto uu) {
          constexpr int u = decltype(uu)::value;
          const int q = j + u * TPL;
          const int km = (q & (Ns - 1)) * M;
          static_for<1, R>([&](auto tt) {
            constexpr int t = decltype(tt)::value;
            T cr, ci;
            if constexpr (s == 1 && Cfg::USE_T1) {
              const V2 w = tw1[(t - 1) * R0 + (q & (R0 - 1))];
              cr = w.x; ci = w.y;
            } else if constexpr (Cfg::USE_HALF) {
              const int e = km * t;
              const V2 w = tw[e & (N / 2 - 1)];
              const unsigned sm = ((unsigned)e << (32 - ilog2(N))) & 0x80000000u;
              cr = xor_sign(w.x, sm); ci = xor_sign(w.y, sm);
            } else {
              const int e = km * t;
              const int qd = e / (N / 4);
              const V2 w = tw[e & (N / 4 - 1)];
              cr = (qd & 1) ? w.y : w.x;
              ci = (qd & 1) ? -w.x : w.y;
              if (qd & 2) { cr = -cr; ci = -ci; }
            }
            const cx<T> x = v[u * R + t];
            v[u * R + t] = cx<T>{x.x * cr - x.y * ci, x.x * ci + x.y * cr};
          });
        });
      }
      static_for<0, NB>([&](auto uu) { dft_reg<T, R, s == 0 && decltype(upper_zero)::value>(&v[decltype(uu)::value * R]); });
      if constexpr (s < NSTAGE - 1) {
        constexpr int Rn = (s == 0) ? R1 : R2;
        auto wr_idx = [&](int u, int t) {
          const int q = j + u * TPL;
          const int k = q & (Ns - 1);
          return at((q - k) * R + k + t * Ns);
        };
        auto rd_idx = [&](int u, int t) { return at(j + u * TPL + t * (N / Rn)); };
        if constexpr (s > 0) xsync();  // previous exchange's reads done
        if constexpr (SPLIT) {
          static_for<0, E>([&](auto ii) {
            constexpr int u = decltype(ii)::value / R, t = decltype(ii)::value % R;
            exs[wr_idx(u, t)] = v[u * R + bitrev(t, LR)].x;
          });
          xsync();
          T re[E];
          static_for<0, E>([&](auto ii) {
            constexpr int u = decltype(ii)::value / Rn, t = decltype(ii)::value % Rn;
            re[decltype(ii)::value] = exs[rd_idx(u, t)];
          });
          xsync();
          static_for<0, E>([&](auto ii) {
            constexpr int u = decltype(ii)::value / R, t = decltype(ii)::value % R;
            exs[wr_idx(u, t)] = v[u * R + bitrev(t, LR)].y;
          });
          xsync();
          static_for<0, E>([&](auto ii) {
            constexpr int u = decltype(ii)::value / Rn, t = decltype(ii)::value % Rn;
            v[decltype(ii)::value] = cx<T>{re[decltype(ii)::value], exs[rd_idx(u, t)]};
          });
        } else {
          static_for<0, E>([&](auto ii) {
            constexpr int u = decltype(ii)::value / R, t = decltype(ii)::value % R;
            const cx<T> x = v[u * R + bitrev(t, LR)];
            V2 w; w.x = x.x; w.y = x.y;
            exv[wr_idx(u, t)] = w;
          });
          xsync();
          static_for<0, E>([&](auto ii) {
            constexpr int u = decltype(ii)::value / Rn, t = decltype(ii)::value % Rn;
            const V2 w = exv[rd_idx(u, t)];
            v[decltype(ii)::value] = cx<T>{w.x, w.y};
          });
        }
      }
    });
  };

  // acc[r] += v[r] * H_k[n], r the last stage's register order; filter values are read once: non-temporal
  cx<T> acc[E];
  static_for<0, E>([&](auto ii) { acc[decltype(ii)::value] = cx<T>{0, 0}; });
  auto filt = [&](const void *filter, auto complex_filter) {
    static_for<0, E>([&](auto ii) {
      constexpr int u = decltype(ii)::value / RL, t = decltype(ii)::value % RL;
      constexpr int cn = u * TPL + t * (N / RL);
      constexpr int r = u * RL + bitrev(t, LRL);
      const long long off = fb + (long long)cn * f.axis;
      const cx<T> x = v[r];
      if constexpr (decltype(complex_filter)::value) {
        V2 h;
        h.x = 0; h.y = 0;
        if (valid) h = gload(reinterpret_cast<const V2 *>(filter) + off);
        const T pr = x.x * h.x - x.y * h.y, pi = x.x * h.y + x.y * h.x;
        acc[r] = cx<T>{acc[r].x + pr, acc[r].y + pi};
      } else {
        T h = 0;
        if (valid) h = __builtin_nontemporal_load(reinterpret_cast<const T *>(filter) + off);
        acc[r] = cx<T>{acc[r].x + x.x * h, acc[r].y + x.y * h};
      }
    });
  };

#pragma nounroll
  for (int k = 0; k < sa.nin; k++) {
    const V2 *line = reinterpret_cast<const V2 *>(sum_pick(sa.src, k)) + lo;
    static_for<0, E>([&](auto ii) {
      constexpr int u = decltype(ii)::value / R0, t = decltype(ii)::value % R0;
      constexpr int cn = u * TPL + t * (N / R0);
      V2 val;
      val.x = 0; val.y = 0;
      if constexpr (!(HALF && cn >= N / 2)) {
        if (valid) val = gload(line + (long long)cn * a.in_axis);
      }
      v[decltype(ii)::value] = cx<T>{val.x, val.y};
    });
    stages(std::integral_constant<bool, HALF>{});
    const void *filter = sum_pick(sa.filter, k);
    if (f.cplx) filt(filter, std::true_type{});
    else filt(filter, std::false_type{});
    xsync();  // this input's last exchange reads done: before the next input's first exchange write, or the round trip's
  }

  // the sum, conjugated (the inverse as conj(F(conj(.)))), through the exchange image: from the last stage's order back
  // into the load distribution
  if constexpr (SPLIT) {
    T re[E];
    static_for<0, E>([&](auto ii) {
      constexpr int u = decltype(ii)::value / RL, t = decltype(ii)::value % RL;
      exs[at(j + u * TPL + t * (N / RL))] = acc[u * RL + bitrev(t, LRL)].x;
    });
    xsync();
    static_for<0, E>([&](auto ii) {
      constexpr int u = decltype(ii)::value / R0, t = decltype(ii)::value % R0;
      re[decltype(ii)::value] = exs[at(j + u * TPL + t * (N / R0))];
    });
    xsync();
    static_for<0, E>([&](auto ii) {
      constexpr int u = decltype(ii)::value / RL, t = decltype(ii)::value % RL;
      exs[at(j + u * TPL + t * (N / RL))] = -acc[u * RL + bitrev(t, LRL)].y;
    });
    xsync();
    static_for<0, E>([&](auto ii) {
      constexpr int u = decltype(ii)::value / R0, t = decltype(ii)::value % R0;
      v[decltype(ii)::value] = cx<T>{re[decltype(ii)::value], exs[at(j + u * TPL + t * (N / R0))]};
    });
  } else {
    static_for<0, E>([&](auto ii) {
      constexpr int u = decltype(ii)::value / RL, t = decltype(ii)::value % RL;
      const cx<T> x = acc[u * RL + bitrev(t, LRL)];
      V2 w; w.x = x.x; w.y = -x.y;
      exv[at(j + u * TPL + t * (N / RL))] = w;
    });
    xsync();
    static_for<0, E>([&](auto ii) {
      constexpr int u = decltype(ii)::value / R0, t = decltype(ii)::value % R0;
      const V2 w = exv[at(j + u * TPL + t * (N / R0))];
      v[decltype(ii)::value] = cx<T>{w.x, w.y};
    });
  }
  xsync();  // the round trip's reads done before the first exchange of the second half writes

  stages(std::false_type{});

  V2 *sline = dst + lo;
  const T sc = (T)a.scale;
  static_for<0, E>([&](auto ii) {
    constexpr int u = decltype(ii)::value / RL, t = decltype(ii)::value % RL;
    constexpr int cn = u * TPL + t * (N / RL);
    if constexpr (HALF && cn >= N / 2) return;
    const cx<T> x = v[u * RL + bitrev(t, LRL)];
    V2 w;
    w.x = x.x * sc;
    w.y = -x.y * sc;
    if (valid) gstore_p<KEEP>(sline + (long long)cn * a.in_axis, w);
  });
}

// (v[E] and acc[E] live together, under the butterfly temporaries: with 64 data VGPRs -- 16 points in double, 32 in single
//  precision -- an instance compiled for 2 waves per SIMD spills (8 ... 570 B per lane), so those are compiled for the fewest
//  waves their workgroup admits, 1 per SIMD at up to 256 threads, and take the accumulator from the 512 registers a lone wave
//  has; the smaller ones are bounded like the fused convolution)
template <typename T, int N, int E, int R0, int R1, int R2, int COLS, bool SPLIT>
constexpr int conv_sum_wps() {
  using Cfg = PanelCfg<N, E, R0, R1, R2, COLS, SPLIT, T>;
  return Cfg::DATA_VGPR >= 64 ? Cfg::WPS_MIN : conv_wps<T, N, E, R0, R1, R2, COLS, SPLIT>();
}

template <typename T, int N, int E, int R0, int R1, int R2, int COLS, bool SPLIT, bool KEEP = false>
__global__ void __launch_bounds__((N / E) * COLS, (conv_sum_wps<T, N, E, R0, R1, R2, COLS, SPLIT>()))
fft_conv_sum_panel_k(PassArgs a, ConvArgs f, SumArgs sa, typename vec2<T>::type *dst, const typename vec2<T>::type *twq) {
  conv_sum_body<T, N, E, R0, R1, R2, COLS, SPLIT, KEEP>(a, f, sa, dst, twq);
}

template <typename T, int N, int E, int R0, int R1, int R2, int COLS, bool SPLIT, bool KEEP = false>
__global__ void __launch_bounds__((N / E) * COLS, (conv_sum_wps<T, N, E, R0, R1, R2, COLS, SPLIT>()))
fft_conv_sum_half_panel_k(PassArgs a, ConvArgs f, SumArgs sa, typename vec2<T>::type *dst, const typename vec2<T>::type *twq) {
  conv_sum_body<T, N, E, R0, R1, R2, COLS, SPLIT, KEEP, true>(a, f, sa, dst, twq);
}

// ---------------------------------------------------------------------------
// Mixed-radix panel kernel: the same three-stage register/LDS Stockham scheme for
// lengths N = R0 * R1 * R2 whose radices are products of small primes (2, 3, 5 with hand-written
// butterflies, 7, 11, 13 as direct DFTs): 768 = 12 x 8 x 8, 1000 = 10 x 10 x 10, 896 = 8 x 8 x 14, ...  Differences from fft_panel_k:
//  * the register butterfly is a mixed-radix decimation in frequency (prime steps with
//    compile-time twiddles w_R^k); its output order is the digit-reversal perm_mixed;
//  * TPL threads share a line and a thread owns ceil((N/R)/TPL) butterflies of a stage, the
//    last one predicated when TPL does not divide N/R, so the register count may differ from
//    stage to stage (the exchange goes through LDS anyway);
//  * index arithmetic uses division by compile-time constants instead of masks; per-peer
//    splits of any length (N/p is rarely a power of two here) use a float-reciprocal divide;
//  * LDS image: the XOR swizzle when R0 is a multiple of 16, else one pad element every R0 when
//    R0 is even (stage-0 write stride becomes odd), none when R0 is odd.
// ---------------------------------------------------------------------------
constexpr int first_factor(int r) {
  return r % 2 == 0 ? 2 : (r % 3 == 0 ? 3 : (r % 5 == 0 ? 5 : (r % 7 == 0 ? 7 : (r % 11 == 0 ? 11 : (r % 13 == 0 ? 13 : r)))));
}
// register radices (<= 32): products of the primes 2 .. 13, or one of the primes 17 .. 31 (a radix <= 32 with such a
// factor is that prime itself; first_factor returns it)
constexpr bool smooth235(int r) { return r <= 1 ? true : (first_factor(r) <= 31 && smooth235(r / first_factor(r))); }
// X[k] of dft_mixed<R> is left in v[perm_mixed(R, k)]
constexpr int perm_mixed(int r, int k) {
  if (r <= 1) return 0;
  const int p = first_factor(r), m = r / p;
  return m * (k % p) + perm_mixed(m, k / p);
}

// d * w_R^K, w_R = exp(-2 pi i / R)
template <typename T, int R, int K>
__device__ __forceinline__ cx<T> mulwr(cx<T> d) {
  constexpr int k = ((K % R) + R) % R;
  if constexpr (k == 0) return d;
  else if constexpr (4 * k == R) return cx<T>{d.y, -d.x};
  else if constexpr (2 * k == R) return cx<T>{-d.x, -d.y};
  else if constexpr (4 * k == 3 * R) return cx<T>{-d.y, d.x};
  else if constexpr (8 * k == R) {
    constexpr T s = (T)W32C[4];
    return cx<T>{(d.x + d.y) * s, (d.y - d.x) * s};
  } else if constexpr (8 * k == 3 * R) {
    constexpr T s = (T)W32C[4];
    return cx<T>{(d.y - d.x) * s, -(d.x + d.y) * s};
  } else {
    constexpr T c = (T)WRC[R][k], s = (T)WRS[R][k];
    return cx<T>{d.x * c + d.y * s, d.y * c - d.x * s};
  }
}

// In-register DFT of R = 2^a 3^b 5^c points, decimation in frequency by the smallest prime p
// (R = p m):  y_d[b] = w_R^(b d) * sum_a x[m a + b] w_p^(a d)  stored at v[m d + b], then a
// DFT of length m on every block d.  X[d + p c] ends in v[m d + perm_mixed(m, c)].
// UZ (R even, so p = 2): v[R/2 ...] are known zeros (the upper half of a zero-padded line, offt_pass_desc::half): they are
// not read, and the first butterfly is a copy and a twiddle (see dft_reg).
template <typename T, int R, bool UZ = false>
__device__ __forceinline__ void dft_mixed(cx<T> *v) {
  if constexpr (R > 1) {
    constexpr int p = first_factor(R), m = R / p;
    static_assert(!UZ || p == 2, "known-zero upper half: even radix");
    static_assert(p == 2 || p == 3 || p == 5 || p == 7 || p == 11 || p == 13 || p == 17 || p == 19 || p == 23 || p == 29 || p == 31,
                  "register radix must be a product of primes <= 13 or a prime <= 31");
    static_for<0, m>([&](auto bb) {
      constexpr int b = decltype(bb)::value;
      if constexpr (UZ) {
        v[m + b] = mulwr<T, R, b>(v[b]);
      } else if constexpr (p == 2) {
        const cx<T> x0 = v[b], x1 = v[m + b];
        v[b] = cx<T>{x0.x + x1.x, x0.y + x1.y};
        v[m + b] = mulwr<T, R, b>(cx<T>{x0.x - x1.x, x0.y - x1.y});
      } else if constexpr (p == 3) {
        constexpr T S3 = (T)WRS[3][1];
        const cx<T> x0 = v[b], x1 = v[m + b], x2 = v[2 * m + b];
        const cx<T> sm{x1.x + x2.x, x1.y + x2.y}, df{x1.x - x2.x, x1.y - x2.y};
        const cx<T> t{x0.x - (T)0.5 * sm.x, x0.y - (T)0.5 * sm.y};
        const cx<T> e{S3 * df.y, -S3 * df.x};  // -i sin(2 pi/3) (x1 - x2)
        v[b] = cx<T>{x0.x + sm.x, x0.y + sm.y};
        v[m + b] = mulwr<T, R, b>(cx<T>{t.x + e.x, t.y + e.y});
        v[2 * m + b] = mulwr<T, R, 2 * b>(cx<T>{t.x - e.x, t.y - e.y});
      } else if constexpr (p == 5) {
        constexpr T C1 = (T)WRC[5][1], C2 = (T)WRC[5][2], S1 = (T)WRS[5][1], S2 = (T)WRS[5][2];
        const cx<T> x0 = v[b], x1 = v[m + b], x2 = v[2 * m + b], x3 = v[3 * m + b], x4 = v[4 * m + b];
        const cx<T> s1{x1.x + x4.x, x1.y + x4.y}, s2{x2.x + x3.x, x2.y + x3.y};
        const cx<T> d1{x1.x - x4.x, x1.y - x4.y}, d2{x2.x - x3.x, x2.y - x3.y};
        const cx<T> p1{x0.x + C1 * s1.x + C2 * s2.x, x0.y + C1 * s1.y + C2 * s2.y};
        const cx<T> p2{x0.x + C2 * s1.x + C1 * s2.x, x0.y + C2 * s1.y + C1 * s2.y};
        const cx<T> q1{S1 * d1.x + S2 * d2.x, S1 * d1.y + S2 * d2.y};
        const cx<T> q2{S2 * d1.x - S1 * d2.x, S2 * d1.y - S1 * d2.y};
        v[b] = cx<T>{x0.x + s1.x + s2.x, x0.y + s1.y + s2.y};
        v[m + b] = mulwr<T, R, b>(cx<T>{p1.x + q1.y, p1.y - q1.x});          // p1 - i q1
        v[2 * m + b] = mulwr<T, R, 2 * b>(cx<T>{p2.x + q2.y, p2.y - q2.x});  // p2 - i q2
        v[3 * m + b] = mulwr<T, R, 3 * b>(cx<T>{p2.x - q2.y, p2.y + q2.x});  // p2 + i q2
        v[4 * m + b] = mulwr<T, R, 4 * b>(cx<T>{p1.x - q1.y, p1.y + q1.x});  // p1 + i q1
      } else {
        // any odd prime p (7, 11, 13; 17 .. 31 in plan-time instances): X_k = x0 + sum_j cos(2 pi j k/p) s_j - i sum_j sin(2 pi j k/p) d_j with
        // s_j = x_j + x_(p-j), d_j = x_j - x_(p-j), j = 1..(p-1)/2; X_(p-k) is the same with + i.  The path is
        // HBM-bound, so the h^2 multiply-adds are not worth a Winograd factorisation.
        constexpr int h = (p - 1) / 2;
        const cx<T> x0 = v[b];
        cx<T> sj[h], dj[h];
        static_for<0, h>([&](auto jj) {
          constexpr int j = decltype(jj)::value + 1;
          const cx<T> xa = v[j * m + b], xb = v[(p - j) * m + b];
          sj[j - 1] = cx<T>{xa.x + xb.x, xa.y + xb.y};
          dj[j - 1] = cx<T>{xa.x - xb.x, xa.y - xb.y};
        });
        cx<T> sum = x0;
        static_for<0, h>([&](auto jj) { sum.x += sj[decltype(jj)::value].x; sum.y += sj[decltype(jj)::value].y; });
        v[b] = sum;
        static_for<0, h>([&](auto kk) {
          constexpr int k = decltype(kk)::value + 1;
          cx<T> pc = x0, qs{(T)0, (T)0};
          static_for<0, h>([&](auto jj) {
            constexpr int j = decltype(jj)::value + 1;
            constexpr T c = (T)WRC[p][(j * k) % p], sn = (T)WRS[p][(j * k) % p];
            pc.x += c * sj[j - 1].x; pc.y += c * sj[j - 1].y;
            qs.x += sn * dj[j - 1].x; qs.y += sn * dj[j - 1].y;
          });
          v[k * m + b] = mulwr<T, R, k * b>(cx<T>{pc.x + qs.y, pc.y - qs.x});              // pc - i qs
          v[(p - k) * m + b] = mulwr<T, R, (p - k) * b>(cx<T>{pc.x - qs.y, pc.y + qs.x});  // pc + i qs
        });
      }
    });
    static_for<0, p>([&](auto dd) { dft_mixed<T, m>(v + decltype(dd)::value * m); });
  }
}

constexpr int cdiv(int a, int b) { return (a + b - 1) / b; }
constexpr int cmax(int a, int b) { return a > b ? a : b; }

template <int N, int TPL, int R0, int R1, int R2, int COLS, bool SPLIT, typename T>
struct PanelXCfg {
  static constexpr int NT = TPL * COLS;
  static constexpr int NSTAGE = (R2 > 1) ? 3 : ((R1 > 1) ? 2 : 1);
  static constexpr int NB0 = cdiv(N / R0, TPL), NB1 = cdiv(N / R1, TPL), NB2 = cdiv(N / R2, TPL);
  static constexpr int EMAX = cmax(NB0 * R0, cmax(R1 > 1 ? NB1 * R1 : 0, R2 > 1 ? NB2 * R2 : 0));
  // LDS image of one column (see PanelCfg): R0 a multiple of 16 -> the XOR swizzle of fft_panel_k (it only
  // permutes inside aligned 16-element runs, so any N that is a multiple of 16 works); otherwise one pad
  // element every R0 when R0 is even (stage-0 write stride becomes odd), nothing when R0 is odd.
  static constexpr bool SWZ = (R0 % 16 == 0) && (N % 16 == 0);
  static constexpr int PADDIV = (!SWZ && R0 % 2 == 0) ? R0 : 0;
  static constexpr int NPAD = PADDIV ? N + N / PADDIV : N;
  static constexpr int LSTRIDE = ((NPAD + 31) / 32) * 32 + 4;
  static constexpr bool QUARTER = (N % 4 == 0);
  static constexpr int QT = QUARTER ? N / 4 + 1 : N;  // twiddle table entries staged in LDS
  static constexpr size_t EX_BYTES = NSTAGE > 1 ? (size_t)COLS * LSTRIDE * sizeof(T) * (SPLIT ? 1 : 2) : 0;
  static constexpr size_t TW_OFF = (EX_BYTES + 15) / 16 * 16;
  static constexpr size_t LDS_BYTES = NSTAGE > 1 ? TW_OFF + (size_t)QT * 2 * sizeof(T) : 0;
  static constexpr int WG_PER_CU_LDS = LDS_BYTES ? (int)(160 * 1024 / LDS_BYTES) : 8;
  static constexpr int WAVES = (NT + 63) / 64;
  static constexpr int WPS_RAW = (WG_PER_CU_LDS * WAVES + 3) / 4;
  static constexpr int WPS = WPS_RAW < 1 ? 1 : (WPS_RAW > 4 ? 4 : WPS_RAW);
  static constexpr int DATA_VGPR = EMAX * (int)sizeof(T) / 2;
  static constexpr int WPS_REG = DATA_VGPR >= 128 ? 2 : (DATA_VGPR >= 64 ? 3 : 4);
  static constexpr int WPS_MIN = (WAVES + 3) / 4;  // one workgroup must fit on a CU
  static constexpr int WPS_E = WPS < WPS_REG ? (WPS < WPS_MIN ? WPS_MIN : WPS) : (WPS_REG < WPS_MIN ? WPS_MIN : WPS_REG);
};

// the body of fft_panelx_k, fft_c2r_panelx_k and fft_half_panelx_k (thin wrappers below, see panel_body)
//   HALF zero-padded half lines (offt_pass_desc::half), with the meaning it has in panel_body.  A load index is
//        n = q + t N/R0 with q < N/R0 and t a compile-time constant: with R0 even, n >= N/2 exactly when t >= R0/2, whatever
//        TPL is and whether or not the butterfly is a predicated one.  The same holds for a store index n = q + t N/R of the
//        last stage's radix R.  So the skipped half costs no load, no predicate and no address on either side; the first
//        and the last radix of a half instance are even.
//        With the two real forms, as in panel_body (fft_half_r2c_panelx_k, fft_half_c2r_panelx_k): R2C with bit 1 -- the reals
//        n >= N/2 of a row are literal zeros; of the N/2+1 outputs, the stores with 2t > R are not compiled and the one
//        with 2t == R is live for q == 0 only.  C2R with bit 2 -- the reals n >= N/2 of a row are not stored.
template <typename T, int N, int TPL, int R0, int R1, int R2, int COLS, bool INC, bool OUTC, bool SPLIT, bool R2C, bool C2R, int HALF = 0>
__device__ __forceinline__ void panelx_body(PassArgs a, const typename vec2<T>::type *in, typename vec2<T>::type *out,
                                            const typename vec2<T>::type *twt) {
  using V2 = typename vec2<T>::type;
  using Cfg = PanelXCfg<N, TPL, R0, R1, R2, COLS, SPLIT, T>;
  constexpr int NT = Cfg::NT, NSTAGE = Cfg::NSTAGE, LSTRIDE = Cfg::LSTRIDE, EMAX = Cfg::EMAX;
  constexpr int PADDIV = Cfg::PADDIV;
  static_assert(R0 * R1 * R2 == N, "radices must multiply to N");
  static_assert(smooth235(R0) && smooth235(R1) && smooth235(R2), "radices must be products of primes <= 13, or primes <= 31");
  static_assert(R0 <= 32 && R1 <= 32 && R2 <= 32, "register radix <= 32");
  static_assert(!(R2C && C2R) && (!C2R || OUTC), "real output: contiguous rows");
  constexpr int RLAST = NSTAGE == 3 ? R2 : (NSTAGE == 2 ? R1 : R0);
  static_assert(HALF == 0 || (R0 % 2 == 0 && RLAST % 2 == 0), "half lines: first and last radix even");
  static_assert(HALF == 0 || ((!R2C || (HALF == 1 && INC && !OUTC)) && (!C2R || (HALF == 2 && !INC))),
                "half lines, real ends: bit 1 on the real-input pass, bit 2 on the real-output pass");

  extern __shared__ __align__(16) unsigned char smem[];
  T *exs = reinterpret_cast<T *>(smem);
  V2 *exv = reinterpret_cast<V2 *>(smem);
  V2 *tw = reinterpret_cast<V2 *>(smem + Cfg::TW_OFF);

  const int tid = threadIdx.x;
  if constexpr (NSTAGE > 1) {
    for (int i = tid; i < Cfg::QT; i += NT) tw[i] = twt[i];
  }
  auto pad = [](int i) {
    if constexpr (Cfg::SWZ) return i ^ ((i / R0) & 15);
    else if constexpr (PADDIV > 0) return i + i / PADDIV;
    else return i;
  };

  const unsigned bid = panel_of_block(blockIdx.x, a.xcd_lim, a.xcd_gshift);
  const int cp = bid % (unsigned)a.ncp;
  const unsigned rest = bid / (unsigned)a.ncp;
  const int b1 = rest % (unsigned)a.nb1;
  const int b2 = rest / (unsigned)a.nb1;
  const int c0 = cp * COLS;

  cx<T> v[EMAX];

  // ---------------- stage 0: global load -------------------------------------
  int c, j;
  if constexpr (INC) { j = tid % TPL; c = tid / TPL; }
  else               { c = tid % COLS; j = tid / COLS; }
  {
    const bool valid = (c0 + c) < a.ncols;
    const V2 *src = in + (long long)b1 * a.in_b1 + (long long)b2 * a.in_b2 + (long long)(c0 + c) * a.in_col;
    constexpr int NBF = N / R0;
    // (the split test is hoisted out of the unrolled loop: the loads of one thread stay back to back)
    auto load_all = [&](auto has_split) {
      static_for<0, Cfg::NB0 * R0>([&](auto ii) {
        constexpr int u = decltype(ii)::value / R0, t = decltype(ii)::value % R0;
        if constexpr ((HALF & 1) != 0 && 2 * t >= R0) {
          v[decltype(ii)::value] = cx<T>{T{}, T{}};  // the padding: a literal zero (and the first butterfly knows it)
          return;
        }
        const int q = j + u * TPL;
        const int n = q + t * NBF;
        const bool live = valid && ((u + 1) * TPL <= NBF || q < NBF);
        V2 val;
        val.x = 0; val.y = 0;
        if constexpr (C2R) {
          // conjugate-symmetric extension of the n/2+1 stored values, then conj-in (see fft_panel_k)
          const bool lo = n <= N / 2;
          if (live)
            val = src[split_offset<decltype(has_split)::value>(lo ? n : N - n, a.in_split, a.in_inv, a.in_nfloor, a.in_lim, a.in_inv1, a.in_blk, a.in_axis, a.in_tab)];
          v[decltype(ii)::value] = cx<T>{val.x, ((a.conj != 0) == lo) ? -val.y : val.y};
        } else if constexpr (R2C) {
          if (live) val.x = reinterpret_cast<const T *>(src)[n];
          v[decltype(ii)::value] = cx<T>{val.x, (T)0};
        } else {
          if (live)
            val = gload(&src[split_offset<decltype(has_split)::value>(n, a.in_split, a.in_inv, a.in_nfloor, a.in_lim, a.in_inv1, a.in_blk, a.in_axis, a.in_tab)]);
          v[decltype(ii)::value] = cx<T>{val.x, a.conj ? -val.y : val.y};
        }
      });
    };
    if (a.in_split || a.in_nfloor) load_all(std::true_type{});
    else load_all(std::false_type{});
  }

  // ---------------- stages ---------------------------------------------------
  static_for<0, NSTAGE>([&](auto sidx) {
    constexpr int s = decltype(sidx)::value;
    constexpr int R = (s == 0) ? R0 : ((s == 1) ? R1 : R2);
    constexpr int Ns = (s == 0) ? 1 : ((s == 1) ? R0 : R0 * R1);
    constexpr int NBF = N / R;             // butterflies per line
    constexpr int NB = cdiv(NBF, TPL);     // butterflies per thread (the last one predicated)

    if constexpr (s > 0) {
      // inter-stage twiddles w_N^(k t M), k = q mod Ns, M = N / (Ns R)
      constexpr int M = N / (Ns * R);
      static_for<0, NB>([&](auto uu) {
        constexpr int u = decltype(uu)::value;
        const int q = j + u * TPL;
        const int km = (q % Ns) * M;
        static_for<1, R>([&](auto tt) {
          constexpr int t = decltype(tt)::value;
          const int e = km * t;            // <= (Ns-1)(R-1)M < N, also for a predicated-off butterfly
          T cr, ci;
          if constexpr (Cfg::QUARTER) {
            const int qd = e / (N / 4);
            const V2 w = tw[e - qd * (N / 4)];
            cr = (qd & 1) ? w.y : w.x;     // times (-i)^qd
            ci = (qd & 1) ? -w.x : w.y;
            if (qd & 2) { cr = -cr; ci = -ci; }
          } else {
            const V2 w = tw[e];
            cr = w.x; ci = w.y;
          }
          const cx<T> x = v[u * R + t];
          v[u * R + t] = cx<T>{x.x * cr - x.y * ci, x.x * ci + x.y * cr};
        });
      });
    }

    static_for<0, NB>([&](auto uu) { dft_mixed<T, R, s == 0 && (HALF & 1) != 0>(&v[decltype(uu)::value * R]); });

    if constexpr (s < NSTAGE - 1) {
      // ---- exchange through LDS: write Stockham-ordered, read strided --------
      constexpr int Rn = (s == 0) ? R1 : R2;
      constexpr int NBFn = N / Rn, NBn = cdiv(NBFn, TPL);
      constexpr bool next_last = (s + 1 == NSTAGE - 1);
      int cn, jn;
      if constexpr (next_last && !OUTC) { cn = tid % COLS; jn = tid / COLS; }
      else                              { jn = tid % TPL; cn = tid / TPL; }

      auto wr_idx = [&](int u, int t) {
        const int q = j + u * TPL;
        const int k = q % Ns;
        return c * LSTRIDE + pad((q - k) * R + k + t * Ns);
      };
      auto wr_live = [&](int u) { return (u + 1) * TPL <= NBF || j + u * TPL < NBF; };
      auto rd_idx = [&](int u, int t) { return cn * LSTRIDE + pad(jn + u * TPL + t * NBFn); };
      auto rd_live = [&](int u) { return (u + 1) * TPL <= NBFn || jn + u * TPL < NBFn; };

      if constexpr (s > 0) __syncthreads();  // previous exchange's reads done
      if constexpr (SPLIT) {
        static_for<0, NB * R>([&](auto ii) {
          constexpr int u = decltype(ii)::value / R, t = decltype(ii)::value % R;
          constexpr int src = u * R + perm_mixed(R, t);
          if (wr_live(u)) exs[wr_idx(u, t)] = v[src].x;
        });
        __syncthreads();
        T re[NBn * Rn];
        static_for<0, NBn * Rn>([&](auto ii) {
          constexpr int u = decltype(ii)::value / Rn, t = decltype(ii)::value % Rn;
          re[decltype(ii)::value] = rd_live(u) ? exs[rd_idx(u, t)] : (T)0;
        });
        __syncthreads();
        static_for<0, NB * R>([&](auto ii) {
          constexpr int u = decltype(ii)::value / R, t = decltype(ii)::value % R;
          constexpr int src = u * R + perm_mixed(R, t);
          if (wr_live(u)) exs[wr_idx(u, t)] = v[src].y;
        });
        __syncthreads();
        static_for<0, NBn * Rn>([&](auto ii) {
          constexpr int u = decltype(ii)::value / Rn, t = decltype(ii)::value % Rn;
          v[decltype(ii)::value] = cx<T>{re[decltype(ii)::value], rd_live(u) ? exs[rd_idx(u, t)] : (T)0};
        });
      } else {
        static_for<0, NB * R>([&](auto ii) {
          constexpr int u = decltype(ii)::value / R, t = decltype(ii)::value % R;
          constexpr int src = u * R + perm_mixed(R, t);
          const cx<T> x = v[src];
          V2 w; w.x = x.x; w.y = x.y;
          if (wr_live(u)) exv[wr_idx(u, t)] = w;
        });
        __syncthreads();
        static_for<0, NBn * Rn>([&](auto ii) {
          constexpr int u = decltype(ii)::value / Rn, t = decltype(ii)::value % Rn;
          V2 w; w.x = 0; w.y = 0;
          if (rd_live(u)) w = exv[rd_idx(u, t)];
          v[decltype(ii)::value] = cx<T>{w.x, w.y};
        });
      }
      c = cn; j = jn;
    } else {
      // ---------------- last stage: global store ------------------------------
      const bool valid = (c0 + c) < a.ncols;
      V2 *dst = out + (long long)b1 * a.out_b1 + (long long)b2 * a.out_b2 + (long long)(c0 + c) * a.out_col;
      const T sc = (T)a.scale;
      auto store_all = [&](auto has_split) {
        static_for<0, NB * R>([&](auto ii) {
          constexpr int u = decltype(ii)::value / R, t = decltype(ii)::value % R;
          if constexpr ((HALF & 2) != 0 && 2 * t >= R) return;  // the upper half of the output is not wanted
          // (real input on half lines: n = q + t N/R is <= N/2 only with 2t < R, or 2t == R and q == 0 -- the rest is not compiled)
          if constexpr (HALF != 0 && R2C && 2 * t > R) return;
          const int q = j + u * TPL;
          const int n = q + t * NBF;
          constexpr int src = u * R + perm_mixed(R, t);
          const cx<T> x = v[src];
          V2 w;
          w.x = x.x * sc;
          w.y = (a.conj ? -x.y : x.y) * sc;
          const bool live = valid && ((u + 1) * TPL <= NBF || q < NBF);
          if constexpr (C2R) {
            if (live) __builtin_nontemporal_store(w.x, reinterpret_cast<T *>(dst) + n);
          } else if (live && (!R2C || n <= N / 2))
            gstore(&dst[split_offset<decltype(has_split)::value>(n, a.out_split, a.out_inv, a.out_nfloor, a.out_lim, a.out_inv1, a.out_blk, a.out_axis, a.out_tab)], w);
        });
      };
      if (a.out_split || a.out_nfloor) store_all(std::true_type{});
      else store_all(std::false_type{});
    }
  });
}

template <typename T, int N, int TPL, int R0, int R1, int R2, int COLS, bool INC, bool OUTC, bool SPLIT, bool R2C = false>
__global__ void __launch_bounds__(TPL * COLS, (PanelXCfg<N, TPL, R0, R1, R2, COLS, SPLIT, T>::WPS_E))
fft_panelx_k(PassArgs a, const typename vec2<T>::type *in, typename vec2<T>::type *out, const typename vec2<T>::type *twt) {
  panelx_body<T, N, TPL, R0, R1, R2, COLS, INC, OUTC, SPLIT, R2C, false>(a, in, out, twt);
}

template <typename T, int N, int TPL, int R0, int R1, int R2, int COLS, bool INC, bool SPLIT>
__global__ void __launch_bounds__(TPL * COLS, (PanelXCfg<N, TPL, R0, R1, R2, COLS, SPLIT, T>::WPS_E))
fft_c2r_panelx_k(PassArgs a, const typename vec2<T>::type *in, typename vec2<T>::type *out, const typename vec2<T>::type *twt) {
  panelx_body<T, N, TPL, R0, R1, R2, COLS, INC, true, SPLIT, false, true>(a, in, out, twt);
}

// zero-padded half lines of a mixed-radix length (offt_pass_desc::half = HALF, 1 or 2): a kernel of its own name, as
// fft_half_panel_k is for the power-of-two body -- fft_panelx_k and fft_c2r_panelx_k keep their symbols
template <typename T, int N, int TPL, int R0, int R1, int R2, int COLS, bool INC, bool OUTC, bool SPLIT, int HALF>
__global__ void __launch_bounds__(TPL * COLS, (PanelXCfg<N, TPL, R0, R1, R2, COLS, SPLIT, T>::WPS_E))
fft_half_panelx_k(PassArgs a, const typename vec2<T>::type *in, typename vec2<T>::type *out, const typename vec2<T>::type *twt) {
  panelx_body<T, N, TPL, R0, R1, R2, COLS, INC, OUTC, SPLIT, false, false, HALF>(a, in, out, twt);
}

// the real ends of a half-box chain at a mixed-radix length (offt_pass_desc::real_input with ::half and its bit 4), names of
// their own like fft_half_r2c_panel_k and fft_half_c2r_panel_k: the real-input z pass that does not load the reals
// n >= N/2 (contiguous rows in, strided out) ...
template <typename T, int N, int TPL, int R0, int R1, int R2, int COLS, bool SPLIT>
__global__ void __launch_bounds__(TPL * COLS, (PanelXCfg<N, TPL, R0, R1, R2, COLS, SPLIT, T>::WPS_E))
fft_half_r2c_panelx_k(PassArgs a, const typename vec2<T>::type *in, typename vec2<T>::type *out, const typename vec2<T>::type *twt) {
  panelx_body<T, N, TPL, R0, R1, R2, COLS, true, false, SPLIT, true, false, 1>(a, in, out, twt);
}
// ... and the real-output z pass that does not store them (strided in, contiguous rows out)
template <typename T, int N, int TPL, int R0, int R1, int R2, int COLS, bool SPLIT>
__global__ void __launch_bounds__(TPL * COLS, (PanelXCfg<N, TPL, R0, R1, R2, COLS, SPLIT, T>::WPS_E))
fft_half_c2r_panelx_k(PassArgs a, const typename vec2<T>::type *in, typename vec2<T>::type *out, const typename vec2<T>::type *twt) {
  panelx_body<T, N, TPL, R0, R1, R2, COLS, false, true, SPLIT, false, true, 2>(a, in, out, twt);
}

// Spectral convolution of whole lines of a mixed-radix length (offt_hipk_conv_pass with offt_filter_desc::mixed): to
// panelx_body what conv_body is to panel_body.  Contiguous lines only -- line offset j = tid % TPL and column c = tid / TPL in
// every stage, no split, complex data, in place through the load side.  A thread owns ceil((N/R)/TPL) butterflies of a
// stage, the last one predicated when TPL does not divide N/R: the filter loads, the round trip and the stores carry the
// live predicates of the exchanges, and a butterfly that is off holds zeros throughout.
//   HALF (fft_conv_half_panelx_k, offt_pass_desc::half = 3): the lines are zero above N/2 going in and only their lower
//        half is wanted coming out; a load index q + t N/R0 is in the upper half exactly when 2t >= R0 and a store index
//        q + t N/RL exactly when 2t >= RL (see panelx_body), so neither is compiled.  The filter and everything between the
//        two is the full line.
// The lines are loaded from `data` and stored at the same offsets from `dst` (as in conv_body): the in-place kernels pass
// one pointer twice, the out-of-place ones (fft_conv_oop_panelx_k, offt_hipk_conv_pass_oop) a second volume, and never
// write the first.
template <typename T, int N, int TPL, int R0, int R1, int R2, int COLS, bool SPLIT, bool HALF = false>
__device__ __forceinline__ void convx_body(PassArgs a, ConvArgs f, const typename vec2<T>::type *data, typename vec2<T>::type *dst,
                                           const void *filter, const typename vec2<T>::type *twt) {
  using V2 = typename vec2<T>::type;
  using Cfg = PanelXCfg<N, TPL, R0, R1, R2, COLS, SPLIT, T>;
  constexpr int NT = Cfg::NT, NSTAGE = Cfg::NSTAGE, LSTRIDE = Cfg::LSTRIDE, EMAX = Cfg::EMAX;
  constexpr int PADDIV = Cfg::PADDIV;
  static_assert(R0 * R1 * R2 == N, "radices must multiply to N");
  static_assert(smooth235(R0) && smooth235(R1) && smooth235(R2), "radices must be products of primes <= 13, or primes <= 31");
  static_assert(R0 <= 32 && R1 <= 32 && R2 <= 32, "register radix <= 32");
  static_assert(NSTAGE > 1, "the round trip goes through the exchange image");
  static_assert(Cfg::QUARTER, "quarter-wave twiddle table: N is a multiple of 4");
  constexpr int RL = NSTAGE == 3 ? R2 : R1;  // radix of the last stage
  static_assert(!HALF || (R0 % 2 == 0 && RL % 2 == 0), "half lines: first and last radix even");
  constexpr int NBF0 = N / R0, NB0 = cdiv(NBF0, TPL);  // butterflies per line / per thread, first stage
  constexpr int NBFL = N / RL, NBL = cdiv(NBFL, TPL);  // ... last stage

  extern __shared__ __align__(16) unsigned char smem[];
  T *exs = reinterpret_cast<T *>(smem);
  V2 *exv = reinterpret_cast<V2 *>(smem);
  V2 *tw = reinterpret_cast<V2 *>(smem + Cfg::TW_OFF);

  const int tid = threadIdx.x;
  for (int i = tid; i < Cfg::QT; i += NT) tw[i] = twt[i];  // (visible after the first exchange's barrier)
  auto pad = [](int i) {
    if constexpr (Cfg::SWZ) return i ^ ((i / R0) & 15);
    else if constexpr (PADDIV > 0) return i + i / PADDIV;
    else return i;
  };

  const unsigned bid = panel_of_block(blockIdx.x, a.xcd_lim, a.xcd_gshift);
  const int cp = bid % (unsigned)a.ncp;
  const unsigned rest = bid / (unsigned)a.ncp;
  const int b1 = rest % (unsigned)a.nb1;
  const int b2 = rest / (unsigned)a.nb1;
  const int c0 = cp * COLS;
  const int j = tid % TPL, c = tid / TPL;
  const bool valid = (c0 + c) < a.ncols;
  const long long lo = (long long)b1 * a.in_b1 + (long long)b2 * a.in_b2 + (long long)(c0 + c) * a.in_col;
  const V2 *line = data + lo;
  V2 *sline = dst + lo;
  const long long fb = (long long)b1 * f.b1 + (long long)b2 * f.b2 + (long long)(c0 + c) * f.col;
  // butterfly u of a stage with NBF butterflies per line is live for this thread (compile-time true but for the last one)
  auto live0 = [&](int u) { return (u + 1) * TPL <= NBF0 || j + u * TPL < NBF0; };
  auto liveL = [&](int u) { return (u + 1) * TPL <= NBFL || j + u * TPL < NBFL; };
  auto at = [&](int i) { return c * LSTRIDE + pad(i); };

  cx<T> v[EMAX];

  static_for<0, NB0 * R0>([&](auto ii) {
    constexpr int u = decltype(ii)::value / R0, t = decltype(ii)::value % R0;
    if constexpr (HALF && 2 * t >= R0) {
      v[decltype(ii)::value] = cx<T>{T{}, T{}};  // the padding: a literal zero (and the first butterfly knows it)
      return;
    }
    const int n = j + u * TPL + t * NBF0;
    V2 val;
    val.x = 0; val.y = 0;
    if (valid && live0(u)) val = gload(line + (long long)n * a.in_axis);
    v[decltype(ii)::value] = cx<T>{val.x, val.y};
  });

  // the forward stages of panelx_body (contiguous / contiguous), ending in the last stage's register order:
  // v[u RL + perm_mixed(RL, t)] holds line index j + u TPL + t N/RL
  auto stages = [&](auto upper_zero) {
    static_for<0, NSTAGE>([&](auto sidx) {
      constexpr int s = decltype(sidx)::value;
      constexpr int R = (s == 0) ? R0 : ((s == 1) ? R1 : R2);
      constexpr int Ns = (s == 0) ? 1 : ((s == 1) ? R0 : R0 * R1);
      constexpr int NBF = N / R;
      constexpr int NB = cdiv(NBF, TPL);
      if constexpr (s > 0) {
        constexpr int M = N / (Ns * R);
        static_for<0, NB>([&](auto uu) {
          constexpr int u = decltype(uu)::value;
          const int q = j + u * TPL;
          const int km = (q % Ns) * M;
          static_for<1, R>([&](auto tt) {
            constexpr int t = decltype(tt)::value;
            const int e = km * t;            // <= (Ns-1)(R-1)M < N, also for a predicated-off butterfly
            const int qd = e / (N / 4);
            const V2 w = tw[e - qd * (N / 4)];
            T cr = (qd & 1) ? w.y : w.x;     // times (-i)^qd
            T ci = (qd & 1) ? -w.x : w.y;
            if (qd & 2) { cr = -cr; ci = -ci; }
            const cx<T> x = v[u * R + t];
            v[u * R + t] = cx<T>{x.x * cr - x.y * ci, x.x * ci + x.y * cr};
          });
        });
      }
      static_for<0, NB>([&](auto uu) { dft_mixed<T, R, s == 0 && decltype(upper_zero)::value>(&v[decltype(uu)::value * R]); });
      if constexpr (s < NSTAGE - 1) {
        constexpr int Rn = (s == 0) ? R1 : R2;
        constexpr int NBFn = N / Rn, NBn = cdiv(NBFn, TPL);
        auto wr_idx = [&](int u, int t) {
          const int q = j + u * TPL;
          const int k = q % Ns;
          return at((q - k) * R + k + t * Ns);
        };
        auto wr_live = [&](int u) { return (u + 1) * TPL <= NBF || j + u * TPL < NBF; };
        auto rd_idx = [&](int u, int t) { return at(j + u * TPL + t * NBFn); };
        auto rd_live = [&](int u) { return (u + 1) * TPL <= NBFn || j + u * TPL < NBFn; };
        if constexpr (s > 0) __syncthreads();  // previous exchange's reads done
        if constexpr (SPLIT) {
          static_for<0, NB * R>([&](auto ii) {
            constexpr int u = decltype(ii)::value / R, t = decltype(ii)::value % R;
            constexpr int src = u * R + perm_mixed(R, t);
            if (wr_live(u)) exs[wr_idx(u, t)] = v[src].x;
          });
          __syncthreads();
          T re[NBn * Rn];
          static_for<0, NBn * Rn>([&](auto ii) {
            constexpr int u = decltype(ii)::value / Rn, t = decltype(ii)::value % Rn;
            re[decltype(ii)::value] = rd_live(u) ? exs[rd_idx(u, t)] : (T)0;
          });
          __syncthreads();
          static_for<0, NB * R>([&](auto ii) {
            constexpr int u = decltype(ii)::value / R, t = decltype(ii)::value % R;
            constexpr int src = u * R + perm_mixed(R, t);
            if (wr_live(u)) exs[wr_idx(u, t)] = v[src].y;
          });
          __syncthreads();
          static_for<0, NBn * Rn>([&](auto ii) {
            constexpr int u = decltype(ii)::value / Rn, t = decltype(ii)::value % Rn;
            v[decltype(ii)::value] = cx<T>{re[decltype(ii)::value], rd_live(u) ? exs[rd_idx(u, t)] : (T)0};
          });
        } else {
          static_for<0, NB * R>([&](auto ii) {
            constexpr int u = decltype(ii)::value / R, t = decltype(ii)::value % R;
            constexpr int src = u * R + perm_mixed(R, t);
            const cx<T> x = v[src];
            V2 w; w.x = x.x; w.y = x.y;
            if (wr_live(u)) exv[wr_idx(u, t)] = w;
          });
          __syncthreads();
          static_for<0, NBn * Rn>([&](auto ii) {
            constexpr int u = decltype(ii)::value / Rn, t = decltype(ii)::value % Rn;
            V2 w; w.x = 0; w.y = 0;
            if (rd_live(u)) w = exv[rd_idx(u, t)];
            v[decltype(ii)::value] = cx<T>{w.x, w.y};
          });
        }
      }
    });
  };

  stages(std::integral_constant<bool, HALF>{});

  // times H[n], then conjugated (the inverse as conj(F(conj(.)))); filter values are read once: non-temporal
  auto filt = [&](auto complex_filter) {
    static_for<0, NBL * RL>([&](auto ii) {
      constexpr int u = decltype(ii)::value / RL, t = decltype(ii)::value % RL;
      constexpr int r = u * RL + perm_mixed(RL, t);
      const int n = j + u * TPL + t * NBFL;
      const long long off = fb + (long long)n * f.axis;
      const bool on = valid && liveL(u);
      const cx<T> x = v[r];
      if constexpr (decltype(complex_filter)::value) {
        V2 h;
        h.x = 0; h.y = 0;
        if (on) h = gload(reinterpret_cast<const V2 *>(filter) + off);
        v[r] = cx<T>{x.x * h.x - x.y * h.y, -(x.x * h.y + x.y * h.x)};
      } else {
        T h = 0;
        if (on) h = __builtin_nontemporal_load(reinterpret_cast<const T *>(filter) + off);
        v[r] = cx<T>{x.x * h, -(x.y * h)};
      }
    });
  };
  if (f.cplx) filt(std::true_type{});
  else filt(std::false_type{});

  // round trip through the exchange image: from the last stage's order back into the load distribution
  __syncthreads();  // the last exchange's reads done
  if constexpr (SPLIT) {
    T re[NB0 * R0];
    static_for<0, NBL * RL>([&](auto ii) {
      constexpr int u = decltype(ii)::value / RL, t = decltype(ii)::value % RL;
      constexpr int src = u * RL + perm_mixed(RL, t);
      if (liveL(u)) exs[at(j + u * TPL + t * NBFL)] = v[src].x;
    });
    __syncthreads();
    static_for<0, NB0 * R0>([&](auto ii) {
      constexpr int u = decltype(ii)::value / R0, t = decltype(ii)::value % R0;
      re[decltype(ii)::value] = live0(u) ? exs[at(j + u * TPL + t * NBF0)] : (T)0;
    });
    __syncthreads();
    static_for<0, NBL * RL>([&](auto ii) {
      constexpr int u = decltype(ii)::value / RL, t = decltype(ii)::value % RL;
      constexpr int src = u * RL + perm_mixed(RL, t);
      if (liveL(u)) exs[at(j + u * TPL + t * NBFL)] = v[src].y;
    });
    __syncthreads();
    static_for<0, NB0 * R0>([&](auto ii) {
      constexpr int u = decltype(ii)::value / R0, t = decltype(ii)::value % R0;
      v[decltype(ii)::value] = cx<T>{re[decltype(ii)::value], live0(u) ? exs[at(j + u * TPL + t * NBF0)] : (T)0};
    });
  } else {
    static_for<0, NBL * RL>([&](auto ii) {
      constexpr int u = decltype(ii)::value / RL, t = decltype(ii)::value % RL;
      constexpr int src = u * RL + perm_mixed(RL, t);
      const cx<T> x = v[src];
      V2 w; w.x = x.x; w.y = x.y;
      if (liveL(u)) exv[at(j + u * TPL + t * NBFL)] = w;
    });
    __syncthreads();
    static_for<0, NB0 * R0>([&](auto ii) {
      constexpr int u = decltype(ii)::value / R0, t = decltype(ii)::value % R0;
      V2 w; w.x = 0; w.y = 0;
      if (live0(u)) w = exv[at(j + u * TPL + t * NBF0)];
      v[decltype(ii)::value] = cx<T>{w.x, w.y};
    });
  }
  __syncthreads();  // the round trip's reads done before the first exchange of the second half writes

  stages(std::false_type{});

  const T sc = (T)a.scale;
  static_for<0, NBL * RL>([&](auto ii) {
    constexpr int u = decltype(ii)::value / RL, t = decltype(ii)::value % RL;
    if constexpr (HALF && 2 * t >= RL) return;  // the upper half of the output is not wanted
    const int n = j + u * TPL + t * NBFL;
    constexpr int src = u * RL + perm_mixed(RL, t);
    const cx<T> x = v[src];
    V2 w;
    w.x = x.x * sc;
    w.y = -x.y * sc;
    if (valid && liveL(u)) gstore(sline + (long long)n * a.in_axis, w);
  });
}

// (at most 2 waves per SIMD, the rule of conv_wps: the filter values and the second half's live ranges cost registers)
template <typename T, int N, int TPL, int R0, int R1, int R2, int COLS, bool SPLIT>
constexpr int convx_wps() { return PanelXCfg<N, TPL, R0, R1, R2, COLS, SPLIT, T>::WPS_E < 2 ? PanelXCfg<N, TPL, R0, R1, R2, COLS, SPLIT, T>::WPS_E : 2; }

template <typename T, int N, int TPL, int R0, int R1, int R2, int COLS, bool SPLIT>
__global__ void __launch_bounds__(TPL * COLS, (convx_wps<T, N, TPL, R0, R1, R2, COLS, SPLIT>()))
fft_conv_panelx_k(PassArgs a, ConvArgs f, typename vec2<T>::type *data, const void *filter, const typename vec2<T>::type *twt) {
  convx_body<T, N, TPL, R0, R1, R2, COLS, SPLIT>(a, f, data, data, filter, twt);
}

template <typename T, int N, int TPL, int R0, int R1, int R2, int COLS, bool SPLIT>
__global__ void __launch_bounds__(TPL * COLS, (convx_wps<T, N, TPL, R0, R1, R2, COLS, SPLIT>()))
fft_conv_half_panelx_k(PassArgs a, ConvArgs f, typename vec2<T>::type *data, const void *filter, const typename vec2<T>::type *twt) {
  convx_body<T, N, TPL, R0, R1, R2, COLS, SPLIT, true>(a, f, data, data, filter, twt);
}

// out of place (offt_hipk_conv_pass_oop with both bits of offt_filter_desc::mixed): the lines of `src` convolved into `dst`
// at the same offsets, `src` left as it was.  Kernels of their own names: the in-place symbols above stay what they were.
template <typename T, int N, int TPL, int R0, int R1, int R2, int COLS, bool SPLIT>
__global__ void __launch_bounds__(TPL * COLS, (convx_wps<T, N, TPL, R0, R1, R2, COLS, SPLIT>()))
fft_conv_oop_panelx_k(PassArgs a, ConvArgs f, const typename vec2<T>::type *src, typename vec2<T>::type *dst, const void *filter,
                      const typename vec2<T>::type *twt) {
  convx_body<T, N, TPL, R0, R1, R2, COLS, SPLIT>(a, f, src, dst, filter, twt);
}

template <typename T, int N, int TPL, int R0, int R1, int R2, int COLS, bool SPLIT>
__global__ void __launch_bounds__(TPL * COLS, (convx_wps<T, N, TPL, R0, R1, R2, COLS, SPLIT>()))
fft_conv_oop_half_panelx_k(PassArgs a, ConvArgs f, const typename vec2<T>::type *src, typename vec2<T>::type *dst, const void *filter,
                           const typename vec2<T>::type *twt) {
  convx_body<T, N, TPL, R0, R1, R2, COLS, SPLIT, true>(a, f, src, dst, filter, twt);
}

// Filtered forward and filtered inverse of whole lines of a mixed-radix length (offt_hipk_filt_pass_fwd and
// offt_hipk_filt_pass_inv with bit 4 of offt_filter_desc::mixed): convx_body cut in two, the way filt_body is conv_body cut in
// two.  Contiguous complex lines, no split, no half lines, addressing through the load side, convx_body's thread mapping and
// predicates: a butterfly that is off neither loads the filter nor stores.
//   INV = false (fft_filt_fwd_panelx_k): load, forward stages, H[n] times the register that holds output index n in the last
//     stage's order, scale, store where the line came from.  In place.
//   INV = true (fft_filt_inv_panelx_k): load from `src`, H[n] loaded with the element's own index and multiplied in the load
//     distribution, conjugate, the stages, conjugate, scale, store to `dst` at the same offsets.  `src` is not written unless
//     dst == src (a workgroup owns whole lines and has loaded all of them before its first exchange, i.e. before any store).
// No round trip through the exchange image: there is only one half.  Filter values are read once: non-temporal.
template <typename T, int N, int TPL, int R0, int R1, int R2, int COLS, bool SPLIT, bool INV>
__device__ __forceinline__ void filtx_body(PassArgs a, ConvArgs f, const typename vec2<T>::type *src, typename vec2<T>::type *dst,
                                           const void *filter, const typename vec2<T>::type *twt) {
  using V2 = typename vec2<T>::type;
  using Cfg = PanelXCfg<N, TPL, R0, R1, R2, COLS, SPLIT, T>;
  constexpr int NT = Cfg::NT, NSTAGE = Cfg::NSTAGE, LSTRIDE = Cfg::LSTRIDE, EMAX = Cfg::EMAX;
  constexpr int PADDIV = Cfg::PADDIV;
  static_assert(R0 * R1 * R2 == N, "radices must multiply to N");
  static_assert(smooth235(R0) && smooth235(R1) && smooth235(R2), "radices must be products of primes <= 13, or primes <= 31");
  static_assert(R0 <= 32 && R1 <= 32 && R2 <= 32, "register radix <= 32");
  static_assert(NSTAGE > 1, "the twiddle table is staged for the exchanges");
  static_assert(Cfg::QUARTER, "quarter-wave twiddle table: N is a multiple of 4");
  constexpr int RL = NSTAGE == 3 ? R2 : R1;  // radix of the last stage
  constexpr int NBF0 = N / R0, NB0 = cdiv(NBF0, TPL);  // butterflies per line / per thread, first stage
  constexpr int NBFL = N / RL, NBL = cdiv(NBFL, TPL);  // ... last stage

  extern __shared__ __align__(16) unsigned char smem[];
  T *exs = reinterpret_cast<T *>(smem);
  V2 *exv = reinterpret_cast<V2 *>(smem);
  V2 *tw = reinterpret_cast<V2 *>(smem + Cfg::TW_OFF);

  const int tid = threadIdx.x;
  for (int i = tid; i < Cfg::QT; i += NT) tw[i] = twt[i];  // (visible after the first exchange's barrier)
  auto pad = [](int i) {
    if constexpr (Cfg::SWZ) return i ^ ((i / R0) & 15);
    else if constexpr (PADDIV > 0) return i + i / PADDIV;
    else return i;
  };

  const unsigned bid = panel_of_block(blockIdx.x, a.xcd_lim, a.xcd_gshift);
  const int cp = bid % (unsigned)a.ncp;
  const unsigned rest = bid / (unsigned)a.ncp;
  const int b1 = rest % (unsigned)a.nb1;
  const int b2 = rest / (unsigned)a.nb1;
  const int c0 = cp * COLS;
  const int j = tid % TPL, c = tid / TPL;
  const bool valid = (c0 + c) < a.ncols;
  const long long lo = (long long)b1 * a.in_b1 + (long long)b2 * a.in_b2 + (long long)(c0 + c) * a.in_col;
  const V2 *line = src + lo;
  V2 *sline = dst + lo;
  const long long fb = (long long)b1 * f.b1 + (long long)b2 * f.b2 + (long long)(c0 + c) * f.col;
  // butterfly u of a stage with NBF butterflies per line is live for this thread (compile-time true but for the last one)
  auto live0 = [&](int u) { return (u + 1) * TPL <= NBF0 || j + u * TPL < NBF0; };
  auto liveL = [&](int u) { return (u + 1) * TPL <= NBFL || j + u * TPL < NBFL; };
  auto at = [&](int i) { return c * LSTRIDE + pad(i); };

  // x times H at line index n (a lane that is off multiplies by zero and stores nothing)
  auto times_h = [&](cx<T> x, int n, bool on, auto complex_filter) {
    const long long off = fb + (long long)n * f.axis;
    if constexpr (decltype(complex_filter)::value) {
      V2 h;
      h.x = 0; h.y = 0;
      if (on) h = gload(reinterpret_cast<const V2 *>(filter) + off);
      return cx<T>{x.x * h.x - x.y * h.y, x.x * h.y + x.y * h.x};
    } else {
      T h = 0;
      if (on) h = __builtin_nontemporal_load(reinterpret_cast<const T *>(filter) + off);
      return cx<T>{x.x * h, x.y * h};
    }
  };

  cx<T> v[EMAX];

  static_for<0, NB0 * R0>([&](auto ii) {
    constexpr int u = decltype(ii)::value / R0, t = decltype(ii)::value % R0;
    const int n = j + u * TPL + t * NBF0;
    V2 val;
    val.x = 0; val.y = 0;
    if (valid && live0(u)) val = gload(line + (long long)n * a.in_axis);
    v[decltype(ii)::value] = cx<T>{val.x, val.y};
  });
  if constexpr (INV) {
    // H in the load distribution, then conjugated (the inverse as conj(F(conj(.))))
    auto filt = [&](auto complex_filter) {
      static_for<0, NB0 * R0>([&](auto ii) {
        constexpr int u = decltype(ii)::value / R0, t = decltype(ii)::value % R0;
        const int n = j + u * TPL + t * NBF0;
        const cx<T> x = times_h(v[decltype(ii)::value], n, valid && live0(u), complex_filter);
        v[decltype(ii)::value] = cx<T>{x.x, -x.y};
      });
    };
    if (f.cplx) filt(std::true_type{});
    else filt(std::false_type{});
  }

  // the forward stages of panelx_body (contiguous / contiguous), ending in the last stage's register order:
  // v[u RL + perm_mixed(RL, t)] holds line index j + u TPL + t N/RL
  static_for<0, NSTAGE>([&](auto sidx) {
    constexpr int s = decltype(sidx)::value;
    constexpr int R = (s == 0) ? R0 : ((s == 1) ? R1 : R2);
    constexpr int Ns = (s == 0) ? 1 : ((s == 1) ? R0 : R0 * R1);
    constexpr int NBF = N / R;
    constexpr int NB = cdiv(NBF, TPL);
    if constexpr (s > 0) {
      constexpr int M = N / (Ns * R);
      static_for<0, NB>([&](auto uu) {
        constexpr int u = decltype(uu)::value;
        const int q = j + u * TPL;
        const int km = (q % Ns) * M;
        static_for<1, R>([&](auto tt) {
          constexpr int t = decltype(tt)::value;
          const int e = km * t;            // <= (Ns-1)(R-1)M < N, also for a predicated-off butterfly
          const int qd = e / (N / 4);
          const V2 w = tw[e - qd * (N / 4)];
          T cr = (qd & 1) ? w.y : w.x;     // times (-i)^qd
          T ci = (qd & 1) ? -w.x : w.y;
          if (qd & 2) { cr = -cr; ci = -ci; }
          const cx<T> x = v[u * R + t];
          v[u * R + t] = cx<T>{x.x * cr - x.y * ci, x.x * ci + x.y * cr};
        });
      });
    }
    static_for<0, NB>([&](auto uu) { dft_mixed<T, R, false>(&v[decltype(uu)::value * R]); });
    if constexpr (s < NSTAGE - 1) {
      constexpr int Rn = (s == 0) ? R1 : R2;
      constexpr int NBFn = N / Rn, NBn = cdiv(NBFn, TPL);
      auto wr_idx = [&](int u, int t) {
        const int q = j + u * TPL;
        const int k = q % Ns;
        return at((q - k) * R + k + t * Ns);
      };
      auto wr_live = [&](int u) { return (u + 1) * TPL <= NBF || j + u * TPL < NBF; };
      auto rd_idx = [&](int u, int t) { return at(j + u * TPL + t * NBFn); };
      auto rd_live = [&](int u) { return (u + 1) * TPL <= NBFn || j + u * TPL < NBFn; };
      if constexpr (s > 0) __syncthreads();  // previous exchange's reads done
      if constexpr (SPLIT) {
        static_for<0, NB * R>([&](auto ii) {
          constexpr int u = decltype(ii)::value / R, t = decltype(ii)::value % R;
          constexpr int from = u * R + perm_mixed(R, t);
          if (wr_live(u)) exs[wr_idx(u, t)] = v[from].x;
        });
        __syncthreads();
        T re[NBn * Rn];
        static_for<0, NBn * Rn>([&](auto ii) {
          constexpr int u = decltype(ii)::value / Rn, t = decltype(ii)::value % Rn;
          re[decltype(ii)::value] = rd_live(u) ? exs[rd_idx(u, t)] : (T)0;
        });
        __syncthreads();
        static_for<0, NB * R>([&](auto ii) {
          constexpr int u = decltype(ii)::value / R, t = decltype(ii)::value % R;
          constexpr int from = u * R + perm_mixed(R, t);
          if (wr_live(u)) exs[wr_idx(u, t)] = v[from].y;
        });
        __syncthreads();
        static_for<0, NBn * Rn>([&](auto ii) {
          constexpr int u = decltype(ii)::value / Rn, t = decltype(ii)::value % Rn;
          v[decltype(ii)::value] = cx<T>{re[decltype(ii)::value], rd_live(u) ? exs[rd_idx(u, t)] : (T)0};
        });
      } else {
        static_for<0, NB * R>([&](auto ii) {
          constexpr int u = decltype(ii)::value / R, t = decltype(ii)::value % R;
          constexpr int from = u * R + perm_mixed(R, t);
          const cx<T> x = v[from];
          V2 w; w.x = x.x; w.y = x.y;
          if (wr_live(u)) exv[wr_idx(u, t)] = w;
        });
        __syncthreads();
        static_for<0, NBn * Rn>([&](auto ii) {
          constexpr int u = decltype(ii)::value / Rn, t = decltype(ii)::value % Rn;
          V2 w; w.x = 0; w.y = 0;
          if (rd_live(u)) w = exv[rd_idx(u, t)];
          v[decltype(ii)::value] = cx<T>{w.x, w.y};
        });
      }
    }
  });

  // the last stage's order: forward times H[n] at the output index; inverse conjugated back; scale; store
  const T sc = (T)a.scale;
  auto store_all = [&](auto complex_filter) {
    static_for<0, NBL * RL>([&](auto ii) {
      constexpr int u = decltype(ii)::value / RL, t = decltype(ii)::value % RL;
      constexpr int from = u * RL + perm_mixed(RL, t);
      const int n = j + u * TPL + t * NBFL;
      const bool on = valid && liveL(u);
      cx<T> x = v[from];
      V2 w;
      if constexpr (INV) {
        w.x = x.x * sc;
        w.y = -x.y * sc;
      } else {
        x = times_h(x, n, on, complex_filter);
        w.x = x.x * sc;
        w.y = x.y * sc;
      }
      if (on) gstore(sline + (long long)n * a.in_axis, w);
    });
  };
  if (!INV && f.cplx) store_all(std::true_type{});
  else store_all(std::false_type{});
}

// (bounded like fft_conv_panelx_k: one transform plus the filter values needs no more registers than the fused convolve --
// the VGPR table is in DESIGN.md 4.5)
template <typename T, int N, int TPL, int R0, int R1, int R2, int COLS, bool SPLIT>
__global__ void __launch_bounds__(TPL * COLS, (convx_wps<T, N, TPL, R0, R1, R2, COLS, SPLIT>()))
fft_filt_fwd_panelx_k(PassArgs a, ConvArgs f, typename vec2<T>::type *data, const void *filter, const typename vec2<T>::type *twt) {
  filtx_body<T, N, TPL, R0, R1, R2, COLS, SPLIT, false>(a, f, data, data, filter, twt);
}

template <typename T, int N, int TPL, int R0, int R1, int R2, int COLS, bool SPLIT>
__global__ void __launch_bounds__(TPL * COLS, (convx_wps<T, N, TPL, R0, R1, R2, COLS, SPLIT>()))
fft_filt_inv_panelx_k(PassArgs a, ConvArgs f, const typename vec2<T>::type *src, typename vec2<T>::type *dst, const void *filter,
                      const typename vec2<T>::type *twt) {
  filtx_body<T, N, TPL, R0, R1, R2, COLS, SPLIT, true>(a, f, src, dst, filter, twt);
}

// Multi-input spectral convolution of whole lines of a mixed-radix length (offt_hipk_conv_pass_sum with bits 1 and 3 of
// offt_filter_desc::mixed): to convx_body what conv_sum_body is to conv_body -- its first half in a loop over the inputs.
// Per workgroup, for k = 0 ... nin-1: load the panel from src[k] (convx_body's loads), forward stages, times H_k in the last
// stage's register order, added into acc[EMAX] in that order (k ascending: the same bits on every run); then conjugate, the
// one round trip through the exchange image, the stages again, conjugate, scale, store to dst at the load offsets.  The
// sources and filters travel by value and are read through sum_pick (see conv_sum_body).  A butterfly that is predicated
// off holds zeros in v and adds zeros.  In place on any ONE source: a workgroup owns whole lines and has loaded them from
// every source before its only stores.  HALF and the limits (contiguous lines, no split, complex data) as in convx_body.
// A __syncthreads() closes every pass of the loop: the first exchange of `stages` has no barrier in front of it, and input
// k's last exchange reads must be done before input k+1's first exchange (or the round trip) writes the image.
template <typename T, int N, int TPL, int R0, int R1, int R2, int COLS, bool SPLIT, bool HALF = false>
__device__ __forceinline__ void convx_sum_body(PassArgs a, ConvArgs f, SumArgs sa, typename vec2<T>::type *dst,
                                               const typename vec2<T>::type *twt) {
  using V2 = typename vec2<T>::type;
  using Cfg = PanelXCfg<N, TPL, R0, R1, R2, COLS, SPLIT, T>;
  constexpr int NT = Cfg::NT, NSTAGE = Cfg::NSTAGE, LSTRIDE = Cfg::LSTRIDE, EMAX = Cfg::EMAX;
  constexpr int PADDIV = Cfg::PADDIV;
  static_assert(R0 * R1 * R2 == N, "radices must multiply to N");
  static_assert(smooth235(R0) && smooth235(R1) && smooth235(R2), "radices must be products of primes <= 13, or primes <= 31");
  static_assert(R0 <= 32 && R1 <= 32 && R2 <= 32, "register radix <= 32");
  static_assert(NSTAGE > 1, "the round trip goes through the exchange image");
  static_assert(Cfg::QUARTER, "quarter-wave twiddle table: N is a multiple of 4");
  constexpr int RL = NSTAGE == 3 ? R2 : R1;  // radix of the last stage
  static_assert(!HALF || (R0 % 2 == 0 && RL % 2 == 0), "half lines: first and last radix even");
  constexpr int NBF0 = N / R0, NB0 = cdiv(NBF0, TPL);  // butterflies per line / per thread, first stage
  constexpr int NBFL = N / RL, NBL = cdiv(NBFL, TPL);  // ... last stage

  extern __shared__ __align__(16) unsigned char smem[];
  T *exs = reinterpret_cast<T *>(smem);
  V2 *exv = reinterpret_cast<V2 *>(smem);
  V2 *tw = reinterpret_cast<V2 *>(smem + Cfg::TW_OFF);

  const int tid = threadIdx.x;
  for (int i = tid; i < Cfg::QT; i += NT) tw[i] = twt[i];  // (visible after the first exchange's barrier)
  auto pad = [](int i) {
    if constexpr (Cfg::SWZ) return i ^ ((i / R0) & 15);
    else if constexpr (PADDIV > 0) return i + i / PADDIV;
    else return i;
  };

  const unsigned bid = panel_of_block(blockIdx.x, a.xcd_lim, a.xcd_gshift);
  const int cp = bid % (unsigned)a.ncp;
  const unsigned rest = bid / (unsigned)a.ncp;
  const int b1 = rest % (unsigned)a.nb1;
  const int b2 = rest / (unsigned)a.nb1;
  const int c0 = cp * COLS;
  const int j = tid % TPL, c = tid / TPL;
  const bool valid = (c0 + c) < a.ncols;
  const long long lo = (long long)b1 * a.in_b1 + (long long)b2 * a.in_b2 + (long long)(c0 + c) * a.in_col;
  const long long fb = (long long)b1 * f.b1 + (long long)b2 * f.b2 + (long long)(c0 + c) * f.col;
  // butterfly u of a stage with NBF butterflies per line is live for this thread (compile-time true but for the last one)
  auto live0 = [&](int u) { return (u + 1) * TPL <= NBF0 || j + u * TPL < NBF0; };
  auto liveL = [&](int u) { return (u + 1) * TPL <= NBFL || j + u * TPL < NBFL; };
  auto at = [&](int i) { return c * LSTRIDE + pad(i); };

  cx<T> v[EMAX];

  // convx_body's stages (contiguous / contiguous), ending in the last stage's register order:
  // v[u RL + perm_mixed(RL, t)] holds line index j + u TPL + t N/RL
  auto stages = [&](auto upper_zero) {
    static_for<0, NSTAGE>([&](auto sidx) {
      constexpr int s = decltype(sidx)::value;
      constexpr int R = (s == 0) ? R0 : ((s == 1) ? R1 : R2);
      constexpr int Ns = (s == 0) ? 1 : ((s == 1) ? R0 : R0 * R1);
      constexpr int NBF = N / R;
      constexpr int NB = cdiv(NBF, TPL);
      if constexpr (s > 0) {
        constexpr int M = N / (Ns * R);
        static_for<0, NB>([&](auto uu) {
          constexpr int u = decltype(uu)::value;
          const int q = j + u * TPL;
          const int km = (q % Ns) * M;
          static_for<1, R>([&](auto tt) {
            constexpr int t = decltype(tt)::value;
            const int e = km * t;            // <= (Ns-1)(R-1)M < N, also for a predicated-off butterfly
            const int qd = e / (N / 4);
            const V2 w = tw[e - qd * (N / 4)];
            T cr = (qd & 1) ? w.y : w.x;     // times (-i)^qd
            T ci = (qd & 1) ? -w.x : w.y;
            if (qd & 2) { cr = -cr; ci = -ci; }
            const cx<T> x = v[u * R + t];
            v[u * R + t] = cx<T>{x.x * cr - x.y * ci, x.x * ci + x.y * cr};
          });
        });
      }
      static_for<0, NB>([&](auto uu) { dft_mixed<T, R, s == 0 && decltype(upper_zero)::value>(&v[decltype(uu)::value * R]); });
      if constexpr (s < NSTAGE - 1) {
        constexpr int Rn = (s == 0) ? R1 : R2;
        constexpr int NBFn = N / Rn, NBn = cdiv(NBFn, TPL);
        auto wr_idx = [&](int u, int t) {
          const int q = j + u * TPL;
          const int k = q % Ns;
          return at((q - k) * R + k + t * Ns);
        };
        auto wr_live = [&](int u) { return (u + 1) * TPL <= NBF || j + u * TPL < NBF; };
        auto rd_idx = [&](int u, int t) { return at(j + u * TPL + t * NBFn); };
        auto rd_live = [&](int u) { return (u + 1) * TPL <= NBFn || j + u * TPL < NBFn; };
        if constexpr (s > 0) __syncthreads();  // previous exchange's reads done
        if constexpr (SPLIT) {
          static_for<0, NB * R>([&](auto ii) {
            constexpr int u = decltype(ii)::value / R, t = decltype(ii)::value % R;
            constexpr int src = u * R + perm_mixed(R, t);
            if (wr_live(u)) exs[wr_idx(u, t)] = v[src].x;
          });
          __syncthreads();
          T re[NBn * Rn];
          static_for<0, NBn * Rn>([&](auto ii) {
            constexpr int u = decltype(ii)::value / Rn, t = decltype(ii)::value % Rn;
            re[decltype(ii)::value] = rd_live(u) ? exs[rd_idx(u, t)] : (T)0;
          });
          __syncthreads();
          static_for<0, NB * R>([&](auto ii) {
            constexpr int u = decltype(ii)::value / R, t = decltype(ii)::value % R;
            constexpr int src = u * R + perm_mixed(R, t);
            if (wr_live(u)) exs[wr_idx(u, t)] = v[src].y;
          });
          __syncthreads();
          static_for<0, NBn * Rn>([&](auto ii) {
            constexpr int u = decltype(ii)::value / Rn, t = decltype(ii)::value % Rn;
            v[decltype(ii)::value] = cx<T>{re[decltype(ii)::value], rd_live(u) ? exs[rd_idx(u, t)] : (T)0};
          });
        } else {
          static_for<0, NB * R>([&](auto ii) {
            constexpr int u = decltype(ii)::value / R, t = decltype(ii)::value % R;
            constexpr int src = u * R + perm_mixed(R, t);
            const cx<T> x = v[src];
            V2 w; w.x = x.x; w.y = x.y;
            if (wr_live(u)) exv[wr_idx(u, t)] = w;
          });
          __syncthreads();
          static_for<0, NBn * Rn>([&](auto ii) {
            constexpr int u = decltype(ii)::value / Rn, t = decltype(ii)::value % Rn;
            V2 w; w.x = 0; w.y = 0;
            if (rd_live(u)) w = exv[rd_idx(u, t)];
            v[decltype(ii)::value] = cx<T>{w.x, w.y};
          });
        }
      }
    });
  };

  // acc[r] += v[r] * H_k[n], r the last stage's register order; filter values are read once: non-temporal.  (A butterfly
  // that is off holds zeros in v, and its filter value is a zero too: it adds zeros.)
  cx<T> acc[EMAX];
  static_for<0, EMAX>([&](auto ii) { acc[decltype(ii)::value] = cx<T>{0, 0}; });
  auto filt = [&](const void *filter, auto complex_filter) {
    static_for<0, NBL * RL>([&](auto ii) {
      constexpr int u = decltype(ii)::value / RL, t = decltype(ii)::value % RL;
      constexpr int r = u * RL + perm_mixed(RL, t);
      const int n = j + u * TPL + t * NBFL;
      const long long off = fb + (long long)n * f.axis;
      const bool on = valid && liveL(u);
      const cx<T> x = v[r];
      if constexpr (decltype(complex_filter)::value) {
        V2 h;
        h.x = 0; h.y = 0;
        if (on) h = gload(reinterpret_cast<const V2 *>(filter) + off);
        const T pr = x.x * h.x - x.y * h.y, pi = x.x * h.y + x.y * h.x;
        acc[r] = cx<T>{acc[r].x + pr, acc[r].y + pi};
      } else {
        T h = 0;
        if (on) h = __builtin_nontemporal_load(reinterpret_cast<const T *>(filter) + off);
        acc[r] = cx<T>{acc[r].x + x.x * h, acc[r].y + x.y * h};
      }
    });
  };

#pragma nounroll
  for (int k = 0; k < sa.nin; k++) {
    const V2 *line = reinterpret_cast<const V2 *>(sum_pick(sa.src, k)) + lo;
    static_for<0, NB0 * R0>([&](auto ii) {
      constexpr int u = decltype(ii)::value / R0, t = decltype(ii)::value % R0;
      if constexpr (HALF && 2 * t >= R0) {
        v[decltype(ii)::value] = cx<T>{T{}, T{}};  // the padding: a literal zero (and the first butterfly knows it)
        return;
      }
      const int n = j + u * TPL + t * NBF0;
      V2 val;
      val.x = 0; val.y = 0;
      if (valid && live0(u)) val = gload(line + (long long)n * a.in_axis);
      v[decltype(ii)::value] = cx<T>{val.x, val.y};
    });
    stages(std::integral_constant<bool, HALF>{});
    const void *filter = sum_pick(sa.filter, k);
    if (f.cplx) filt(filter, std::true_type{});
    else filt(filter, std::false_type{});
    __syncthreads();  // this input's last exchange reads done: before the next input's first exchange write, or the round trip's
  }

  // the sum, conjugated (the inverse as conj(F(conj(.)))), through the exchange image: from the last stage's order back
  // into the load distribution
  if constexpr (SPLIT) {
    T re[NB0 * R0];
    static_for<0, NBL * RL>([&](auto ii) {
      constexpr int u = decltype(ii)::value / RL, t = decltype(ii)::value % RL;
      constexpr int src = u * RL + perm_mixed(RL, t);
      if (liveL(u)) exs[at(j + u * TPL + t * NBFL)] = acc[src].x;
    });
    __syncthreads();
    static_for<0, NB0 * R0>([&](auto ii) {
      constexpr int u = decltype(ii)::value / R0, t = decltype(ii)::value % R0;
      re[decltype(ii)::value] = live0(u) ? exs[at(j + u * TPL + t * NBF0)] : (T)0;
    });
    __syncthreads();
    static_for<0, NBL * RL>([&](auto ii) {
      constexpr int u = decltype(ii)::value / RL, t = decltype(ii)::value % RL;
      constexpr int src = u * RL + perm_mixed(RL, t);
      if (liveL(u)) exs[at(j + u * TPL + t * NBFL)] = -acc[src].y;
    });
    __syncthreads();
    static_for<0, NB0 * R0>([&](auto ii) {
      constexpr int u = decltype(ii)::value / R0, t = decltype(ii)::value % R0;
      v[decltype(ii)::value] = cx<T>{re[decltype(ii)::value], live0(u) ? exs[at(j + u * TPL + t * NBF0)] : (T)0};
    });
  } else {
    static_for<0, NBL * RL>([&](auto ii) {
      constexpr int u = decltype(ii)::value / RL, t = decltype(ii)::value % RL;
      constexpr int src = u * RL + perm_mixed(RL, t);
      const cx<T> x = acc[src];
      V2 w; w.x = x.x; w.y = -x.y;
      if (liveL(u)) exv[at(j + u * TPL + t * NBFL)] = w;
    });
    __syncthreads();
    static_for<0, NB0 * R0>([&](auto ii) {
      constexpr int u = decltype(ii)::value / R0, t = decltype(ii)::value % R0;
      V2 w; w.x = 0; w.y = 0;
      if (live0(u)) w = exv[at(j + u * TPL + t * NBF0)];
      v[decltype(ii)::value] = cx<T>{w.x, w.y};
    });
  }
  __syncthreads();  // the round trip's reads done before the first exchange of the second half writes

  stages(std::false_type{});

  V2 *sline = dst + lo;
  const T sc = (T)a.scale;
  static_for<0, NBL * RL>([&](auto ii) {
    constexpr int u = decltype(ii)::value / RL, t = decltype(ii)::value % RL;
    if constexpr (HALF && 2 * t >= RL) return;  // the upper half of the output is not wanted
    const int n = j + u * TPL + t * NBFL;
    constexpr int src = u * RL + perm_mixed(RL, t);
    const cx<T> x = v[src];
    V2 w;
    w.x = x.x * sc;
    w.y = -x.y * sc;
    if (valid && liveL(u)) gstore(sline + (long long)n * a.in_axis, w);
  });
}

// (v[EMAX] and acc[EMAX] live together under the butterfly temporaries: the instances are compiled for the fewest waves per
//  SIMD their workgroup admits -- 1 at up to 256 threads, 512 registers a lane -- as the power-of-two gather kernels with 64
//  data VGPRs are (conv_sum_wps); their shapes, offt_reg_conv_sum_mixed_*.hip, are chosen so that nothing spills there)
template <typename T, int N, int TPL, int R0, int R1, int R2, int COLS, bool SPLIT>
constexpr int convx_sum_wps() { return PanelXCfg<N, TPL, R0, R1, R2, COLS, SPLIT, T>::WPS_MIN; }

template <typename T, int N, int TPL, int R0, int R1, int R2, int COLS, bool SPLIT>
__global__ void __launch_bounds__(TPL * COLS, (convx_sum_wps<T, N, TPL, R0, R1, R2, COLS, SPLIT>()))
fft_conv_sum_panelx_k(PassArgs a, ConvArgs f, SumArgs sa, typename vec2<T>::type *dst, const typename vec2<T>::type *twt) {
  convx_sum_body<T, N, TPL, R0, R1, R2, COLS, SPLIT>(a, f, sa, dst, twt);
}

template <typename T, int N, int TPL, int R0, int R1, int R2, int COLS, bool SPLIT>
__global__ void __launch_bounds__(TPL * COLS, (convx_sum_wps<T, N, TPL, R0, R1, R2, COLS, SPLIT>()))
fft_conv_sum_half_panelx_k(PassArgs a, ConvArgs f, SumArgs sa, typename vec2<T>::type *dst, const typename vec2<T>::type *twt) {
  convx_sum_body<T, N, TPL, R0, R1, R2, COLS, SPLIT, true>(a, f, sa, dst, twt);
}

// ---------------------------------------------------------------------------
// Pseudo-spectral product of whole lines (offt_hipk_prod_pass): out = fft( ifft(a) . ifft(b) ), the last pass of two inverse
// transforms, the pointwise product and the first pass of the forward transform in one launch -- the dual of
// conv_sum_body.  In the z-y-x layout all three are the z pass over the lines of the scratch volume W[x][z][y], so the lines
// are STRIDED: a panel is COLS consecutive columns (128-B segments at a pitch of one W line), panel_body's strided / strided
// addressing and thread mappings:
//   A  lanes across columns (c = tid % COLS, j = tid / COLS): the loads, the first and the last stage, the stores
//   B  lanes along the line  (j = tid % TPL,  c = tid / TPL): the middle stage of a three-stage shape
// Per workgroup, for source 0 and, if there is one, source 1: load the panel conjugated (the inverse as conj(F(conj(.)))), the
// stages; acc[E] = the first result, then acc[i] *= v[i] -- both in the last stage's register order, and the product is
// pointwise, so nothing is reordered.  One source: acc[i] *= acc[i], a uniform branch (the two-source form's registers).
// Then back to the load order.  The last stage leaves a thread the line indices j + m TPL, m < E, of its column, which are
// the indices it loaded: going back is a renaming of registers at compile time (conj(acc) read in another order), no trip
// through LDS.  The stages again (forward), scale, store at the load offsets of `dst`.
// `dst` may be either source: a workgroup owns whole lines and has loaded them from both before its only stores.
//
// REAL (offt_hipk_prod_real_pass, fft_prod_real_panel_k): the lines are HALF SPECTRA of real fields -- N is the real length, a
// line in memory the N/2+1 complex values at a pitch of in_axis.  Both inverses ride on ONE complex FFT: with A~, B~ the
// Hermitian extensions (X~[n] = X[n] for n <= N/2, conj(X[N - n]) above), Z = A~ + i B~ has the unnormalised inverse a + i b,
// a and b the two real fields.  The stages get conj(Z) and leave v = a - i b, so the product is p = -v.x v.y: no accumulator
// array and no barrier between sources.  One source: Z = A~, v = (a, 0), p = v.x^2.  The imaginary parts of X[0] and X[N/2]
// are DROPPED before packing: the separate real-output passes discard them with their imaginary output, here Im A[0] would
// end up in field b and Im B[0] in field a.  The mirrored half re-reads what the workgroup loads for its own half anyway
// (panel_body's C2R load: a per-lane base plus a uniform offset for either half, default cache policy so that the second
// read is an L2 hit).  (p, 0) goes back to the load order by the same renaming, the stages run again, and only the indices
// n <= N/2 are stored.
template <typename T, int N, int E, int R0, int R1, int R2, int COLS, bool SPLIT, bool REAL = false>
__device__ __forceinline__ void prod_body(PassArgs a, const typename vec2<T>::type *src0, const typename vec2<T>::type *src1,
                                          typename vec2<T>::type *dst, const typename vec2<T>::type *twq) {
  using V2 = typename vec2<T>::type;
  using Cfg = PanelCfg<N, E, R0, R1, R2, COLS, SPLIT, T>;
  constexpr int TPL = Cfg::TPL, NT = Cfg::NT, NSTAGE = Cfg::NSTAGE;
  constexpr int LSTRIDE = Cfg::LSTRIDE;
  constexpr bool SWZ = Cfg::SWZ;
  constexpr int PS = SWZ ? Cfg::SWZSHIFT : Cfg::PADSHIFT;
  static_assert(lanes<T>::n == 1, "one column per lane");
  static_assert(R0 * R1 * R2 == N, "radices must multiply to N");
  static_assert(E % R0 == 0 && E % R1 == 0 && E % R2 == 0 && N % E == 0, "bad E");
  static_assert(NSTAGE > 1, "at least one exchange");
  constexpr int RL = NSTAGE == 3 ? R2 : R1;  // radix of the last stage
  constexpr int LRL = ilog2(RL);

  extern __shared__ __align__(16) unsigned char smem[];
  T *exs = reinterpret_cast<T *>(smem);
  V2 *exv = reinterpret_cast<V2 *>(smem);
  V2 *tw = reinterpret_cast<V2 *>(smem + Cfg::TW_OFF);
  V2 *tw1 = reinterpret_cast<V2 *>(smem + Cfg::T1_OFF);

  const int tid = threadIdx.x;
  for (int i = tid; i < Cfg::QT; i += NT) tw[i] = twq[i];
  if constexpr (Cfg::USE_T1) {
    constexpr int M1 = N / (R0 * R1);
    for (int i = tid; i < Cfg::T1N; i += NT) {
      const int t = i / R0 + 1, k = i - (t - 1) * R0;
      tw1[i] = twq[k * M1 * t];
    }
  }
  __syncthreads();  // the twiddle tables are visible (once, ahead of the three runs of the stages)

  const unsigned bid = panel_of_block(blockIdx.x, a.xcd_lim, a.xcd_gshift);
  const int cp = bid % (unsigned)a.ncp;
  const unsigned rest = bid / (unsigned)a.ncp;
  const int b1 = rest % (unsigned)a.nb1;
  const int b2 = rest / (unsigned)a.nb1;
  const int c0 = cp * COLS;
  const int cA = tid % COLS, jA = tid / COLS, jB = tid % TPL, cB = tid / TPL;
  const bool valid = (c0 + cA) < a.ncols;  // a ragged last column group: lanes past the last column load and store nothing
  const long long lo = (long long)b1 * a.in_b1 + (long long)b2 * a.in_b2 + (long long)(c0 + cA) * a.in_col + (long long)jA * a.in_axis;

  // a wave owns whole columns in mapping B when TPL divides 64 (see panel_body)
  constexpr bool WAVE_COLS = (64 % TPL == 0) && (NT % 64 == 0);

  cx<T> v[E];

  // panel_body's stages, strided / strided: from the load distribution in mapping A to the last stage's register order in
  // mapping A -- v[u RL + bitrev(t)] holds line index jA + u TPL + t N/RL of column cA.  Every exchange has mapping A on one
  // side at least, so its writes and reads are a workgroup barrier apart.
  auto stages = [&]() {
    int c = cA, j = jA;
    static_for<0, NSTAGE>([&](auto sidx) {
      constexpr int s = decltype(sidx)::value;
      constexpr int R = (s == 0) ? R0 : ((s == 1) ? R1 : R2);
      constexpr int Ns = (s == 0) ? 1 : ((s == 1) ? R0 : R0 * R1);
      constexpr int NB = E / R;
      constexpr int LR = ilog2(R);
      if constexpr (s > 0) {
        constexpr int M = N / (Ns * R);
        static_for<0, NB>([&](auto uu) {
          constexpr int u = decltype(uu)::value;
          const int q = j + u * TPL;
          const int km = (q & (Ns - 1)) * M;
          static_for<1, R>([&](auto tt) {
            constexpr int t = decltype(tt)::value;
            T cr, ci;
            if constexpr (s == 1 && Cfg::USE_T1) {
              const V2 w = tw1[(t - 1) * R0 + (q & (R0 - 1))];
              cr = w.x; ci = w.y;
            } else if constexpr (Cfg::USE_HALF) {
              const int e = km * t;
              const V2 w = tw[e & (N / 2 - 1)];
              const unsigned sm = ((unsigned)e << (32 - ilog2(N))) & 0x80000000u;
              cr = xor_sign(w.x, sm); ci = xor_sign(w.y, sm);
            } else {
              const int e = km * t;
              const int qd = e / (N / 4);
              const V2 w = tw[e & (N / 4 - 1)];
              cr = (qd & 1) ? w.y : w.x;
              ci = (qd & 1) ? -w.x : w.y;
              if (qd & 2) { cr = -cr; ci = -ci; }
            }
            const cx<T> x = v[u * R + t];
            v[u * R + t] = cx<T>{x.x * cr - x.y * ci, x.x * ci + x.y * cr};
          });
        });
      }
      static_for<0, NB>([&](auto uu) { dft_reg<T, R>(&v[decltype(uu)::value * R]); });
      if constexpr (s < NSTAGE - 1) {
        constexpr int Rn = (s == 0) ? R1 : R2;
        constexpr bool next_last = (s + 1 == NSTAGE - 1);
        const int cn = next_last ? cA : cB, jn = next_last ? jA : jB;  // the reader's mapping
        auto wr_idx = [&](int u, int t) {
          const int q = j + u * TPL;
          const int k = q & (Ns - 1);
          return c * LSTRIDE + padidx<SWZ, PS>((q - k) * R + k + t * Ns);
        };
        auto rd_idx = [&](int u, int t) { return cn * LSTRIDE + padidx<SWZ, PS>(jn + u * TPL + t * (N / Rn)); };
        if constexpr (s > 0) {
          // the previous exchange's reads are done: they ran in mapping B, as these writes do
          if constexpr (WAVE_COLS) {
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
          } else {
            __syncthreads();
          }
        }
        if constexpr (SPLIT) {
          static_for<0, E>([&](auto ii) {
            constexpr int u = decltype(ii)::value / R, t = decltype(ii)::value % R;
            exs[wr_idx(u, t)] = v[u * R + bitrev(t, LR)].x;
          });
          __syncthreads();
          T re[E];
          static_for<0, E>([&](auto ii) {
            constexpr int u = decltype(ii)::value / Rn, t = decltype(ii)::value % Rn;
            re[decltype(ii)::value] = exs[rd_idx(u, t)];
          });
          __syncthreads();
          static_for<0, E>([&](auto ii) {
            constexpr int u = decltype(ii)::value / R, t = decltype(ii)::value % R;
            exs[wr_idx(u, t)] = v[u * R + bitrev(t, LR)].y;
          });
          __syncthreads();
          static_for<0, E>([&](auto ii) {
            constexpr int u = decltype(ii)::value / Rn, t = decltype(ii)::value % Rn;
            v[decltype(ii)::value] = cx<T>{re[decltype(ii)::value], exs[rd_idx(u, t)]};
          });
        } else {
          static_for<0, E>([&](auto ii) {
            constexpr int u = decltype(ii)::value / R, t = decltype(ii)::value % R;
            const cx<T> x = v[u * R + bitrev(t, LR)];
            V2 w; w.x = x.x; w.y = x.y;
            exv[wr_idx(u, t)] = w;
          });
          __syncthreads();
          static_for<0, E>([&](auto ii) {
            constexpr int u = decltype(ii)::value / Rn, t = decltype(ii)::value % Rn;
            const V2 w = exv[rd_idx(u, t)];
            v[decltype(ii)::value] = cx<T>{w.x, w.y};
          });
        }
        c = cn; j = jn;
      }
    });
  };

  if constexpr (REAL) {
    static_assert(TPL <= N / 2 && (N / 2) % TPL == 0, "the line's halves are whole rows of registers");
    // element (u, t) is line index n = jA + cn: the stored value at n for n <= N/2, the conjugate of the one at N - n above
    // -- N - n = -jA + a uniform N - cn, so the mirrored half has a per-lane base of its own
    const long long lm = lo - 2LL * jA * a.in_axis;
    auto load_packed = [&](auto two_) {
      constexpr bool TWO = decltype(two_)::value;
      static_for<0, E>([&](auto ii) {
        constexpr int u = decltype(ii)::value / R0, t = decltype(ii)::value % R0;
        constexpr int cn = u * TPL + t * (N / R0);
        const bool low = (jA + cn) <= N / 2;
        const bool end = (cn == 0 || cn == N / 2) && jA == 0;  // n = 0 or N/2: real by symmetry, the stored imaginary part dropped
        const long long off = low ? lo + (long long)cn * a.in_axis : lm + (long long)(N - cn) * a.in_axis;
        V2 x, y;
        x.x = 0; x.y = 0; y.x = 0; y.y = 0;
        if (valid) {
          x = src0[off];
          if constexpr (TWO) y = src1[off];
        }
        const T ai = end ? (T)0 : (low ? x.y : -x.y);
        if constexpr (TWO) {
          const T bi = end ? (T)0 : (low ? y.y : -y.y);
          v[decltype(ii)::value] = cx<T>{x.x - bi, -(ai + y.x)};  // conj(A~ + i B~)
        } else {
          v[decltype(ii)::value] = cx<T>{x.x, -ai};
        }
      });
    };
    const bool two = src1 != nullptr;
    if (two) load_packed(std::true_type{});
    else load_packed(std::false_type{});

    stages();

    // v = a - i b (one source: (a, 0)); the product (p, 0) back in the load order, by prod_body's renaming of registers
    T p[E];
    if (two) static_for<0, E>([&](auto ii) { p[decltype(ii)::value] = -(v[decltype(ii)::value].x * v[decltype(ii)::value].y); });
    else static_for<0, E>([&](auto ii) { p[decltype(ii)::value] = v[decltype(ii)::value].x * v[decltype(ii)::value].x; });
    static_for<0, E>([&](auto ii) {
      constexpr int u = decltype(ii)::value / R0, t = decltype(ii)::value % R0;
      constexpr int m = u + t * (E / R0);
      constexpr int ul = m % (E / RL), tl = m / (E / RL);
      v[decltype(ii)::value] = cx<T>{p[ul * RL + bitrev(tl, LRL)], (T)0};
    });
    __syncthreads();  // the inverse's last exchange reads done: before the forward's first exchange writes

    stages();

    // the half spectrum of the product: indices n <= N/2 only (n = N/2 is row cn = N/2 of the lanes with jA = 0)
    V2 *sline = dst + lo;
    const T sc = (T)a.scale;
    static_for<0, E>([&](auto ii) {
      constexpr int u = decltype(ii)::value / RL, t = decltype(ii)::value % RL;
      constexpr int cn = u * TPL + t * (N / RL);
      if constexpr (cn > N / 2) return;
      const cx<T> x = v[u * RL + bitrev(t, LRL)];
      V2 w;
      w.x = x.x * sc;
      w.y = x.y * sc;
      if (valid && (cn < N / 2 || jA == 0)) gstore(sline + (long long)cn * a.in_axis, w);
    });
    return;
  }

  // acc = conj(ifft(src0)) . conj(ifft(src1)) = conj of the product, in the last stage's register order
  cx<T> acc[E];
  const int nsrc = src1 ? 2 : 1;
#pragma nounroll
  for (int k = 0; k < nsrc; k++) {
    const V2 *line = (k ? src1 : src0) + lo;
    static_for<0, E>([&](auto ii) {
      constexpr int u = decltype(ii)::value / R0, t = decltype(ii)::value % R0;
      constexpr int cn = u * TPL + t * (N / R0);
      V2 val;
      val.x = 0; val.y = 0;
      if (valid) val = gload(line + (long long)cn * a.in_axis);
      v[decltype(ii)::value] = cx<T>{val.x, -val.y};
    });
    stages();
    if (k == 0) {
      static_for<0, E>([&](auto ii) { acc[decltype(ii)::value] = v[decltype(ii)::value]; });
    } else {
      static_for<0, E>([&](auto ii) {
        const cx<T> p = acc[decltype(ii)::value], q = v[decltype(ii)::value];
        acc[decltype(ii)::value] = cx<T>{p.x * q.x - p.y * q.y, p.x * q.y + p.y * q.x};
      });
    }
    __syncthreads();  // this source's last exchange reads done: before the next run of the stages writes its first exchange
  }
  if (nsrc == 1) {
    static_for<0, E>([&](auto ii) {
      const cx<T> p = acc[decltype(ii)::value];
      acc[decltype(ii)::value] = cx<T>{p.x * p.x - p.y * p.y, (p.x + p.x) * p.y};
    });
  }

  // the product itself, conj(acc), back in the load order: load register u R0 + t holds line index jA + (u + t E/R0) TPL,
  // and the last stage left that index in register u' RL + bitrev(t') with u' + t' E/RL = u + t E/R0
  static_for<0, E>([&](auto ii) {
    constexpr int u = decltype(ii)::value / R0, t = decltype(ii)::value % R0;
    constexpr int m = u + t * (E / R0);
    constexpr int ul = m % (E / RL), tl = m / (E / RL);
    const cx<T> x = acc[ul * RL + bitrev(tl, LRL)];
    v[decltype(ii)::value] = cx<T>{x.x, -x.y};
  });

  stages();

  V2 *sline = dst + lo;
  const T sc = (T)a.scale;
  static_for<0, E>([&](auto ii) {
    constexpr int u = decltype(ii)::value / RL, t = decltype(ii)::value % RL;
    constexpr int cn = u * TPL + t * (N / RL);
    const cx<T> x = v[u * RL + bitrev(t, LRL)];
    V2 w;
    w.x = x.x * sc;
    w.y = x.y * sc;
    if (valid) gstore(sline + (long long)cn * a.in_axis, w);
  });
}

// (v[E] and acc[E] live together as in conv_sum_body: the same bound on the waves per SIMD)
template <typename T, int N, int E, int R0, int R1, int R2, int COLS, bool SPLIT>
__global__ void __launch_bounds__((N / E) * COLS, (conv_sum_wps<T, N, E, R0, R1, R2, COLS, SPLIT>()))
fft_prod_panel_k(PassArgs a, const typename vec2<T>::type *src0, const typename vec2<T>::type *src1, typename vec2<T>::type *dst,
                 const typename vec2<T>::type *twq) {
  prod_body<T, N, E, R0, R1, R2, COLS, SPLIT>(a, src0, src1, dst, twq);
}

// (one v[E] and no accumulator: bounded like the fused convolution, which runs its stages twice over one array as well;
//  WPS = 0 asks for that bound, anything else states the waves per SIMD of an instance -- offt_reg_prod_real_*.hip)
template <typename T, int N, int E, int R0, int R1, int R2, int COLS, bool SPLIT, int WPS>
constexpr int prod_real_wps() { return WPS > 0 ? WPS : conv_wps<T, N, E, R0, R1, R2, COLS, SPLIT>(); }

template <typename T, int N, int E, int R0, int R1, int R2, int COLS, bool SPLIT, int WPS = 0>
__global__ void __launch_bounds__((N / E) * COLS, (prod_real_wps<T, N, E, R0, R1, R2, COLS, SPLIT, WPS>()))
fft_prod_real_panel_k(PassArgs a, const typename vec2<T>::type *src0, const typename vec2<T>::type *src1, typename vec2<T>::type *dst,
                      const typename vec2<T>::type *twq) {
  prod_body<T, N, E, R0, R1, R2, COLS, SPLIT, true>(a, src0, src1, dst, twq);
}

// ---------------------------------------------------------------------------
// variant registry: every instantiation registers itself under a VariantKey (which kernel it is) and an id
// ---------------------------------------------------------------------------
// what an instance does to a line
enum class Role {
  Plain,    // complex lines: fft_panel_k / fft_panelx_k, on half lines fft_half_panel_k / fft_half_panelx_k
  R2C,      // real-input z pass (offt_pass_desc::real_input = 1); on half lines fft_half_r2c_panel_k / fft_half_r2c_panelx_k
  C2R,      // real-output z pass (real_input = 2): fft_c2r_panel_k / fft_c2r_panelx_k; on half lines fft_half_c2r_panel(x)_k
  TW4,      // four-step twiddles on the stores (offt_pass_desc::tw4): the first sub-pass of a long line
  Conv,     // fused convolution in place (offt_hipk_conv_pass): fft_conv_panel_k, fft_conv_half_panel_k and their panelx twins
  ConvOop,  // ... with a separate store base (offt_hipk_conv_pass_oop): fft_conv_oop_panel_k, fft_conv_oop_half_panel_k, ...
  ConvSum,  // several sources summed into one destination (offt_hipk_conv_pass_sum): fft_conv_sum_panel_k, fft_conv_sum_half_panel_k
            // and their panelx twins
  FiltFwd,  // forward x pass with the filter on its stores, in place (offt_hipk_filt_pass_fwd): fft_filt_fwd_panel_k, fft_filt_fwd_panelx_k
  FiltInv,  // inverse x pass with the filter on its loads, src -> dst (offt_hipk_filt_pass_inv): fft_filt_inv_panel_k, fft_filt_inv_panelx_k
  PairYX,   // two passes in one grid (offt_hipk_fft_pass_pair): fft_pair_yx_k, the x pass of one group of planes next to the y pass
            // of the next.  key.n is the y length, the entry's id the x length.
  Prod,     // pseudo-spectral product (offt_hipk_prod_pass): fft_prod_panel_k, two inverse passes, their product and a forward pass
            // over strided lines, stored at the load offsets
  ProdReal, // ... of real fields held as half spectra (offt_hipk_prod_real_pass): fft_prod_real_panel_k, key.n the REAL length, lines
            // of n/2+1 complex values, both inverses from one packed complex FFT
};
// column-pair instances (T = f32x2) are kept under their own precision so that the one-column variants and their ids stay
// what they were
enum { OFFT_PREC_F32_PAIR = 3, VARIANT_PAIR0 = 200 };  // descriptor variant 200 + id forces pair variant `id`
template <typename T>
constexpr int prec_of() { return std::is_same<T, double>::value ? OFFT_PREC_F64 : (lanes<T>::n == 2 ? OFFT_PREC_F32_PAIR : OFFT_PREC_F32); }

// The identity of an instance: a lookup compares all of it, so whoever asks for a key gets that kernel or none.  `mixed`
// (fft_panel_k or fft_panelx_k) is NOT part of it: the any-split fft_panelx_k instance of a power-of-two length shares the
// bucket of the fft_panel_k ones and is told apart by its id, VARIANT_ANYSPLIT.
struct VariantKey {
  int n, prec;     // prec: OFFT_PREC_F64, OFFT_PREC_F32 or OFFT_PREC_F32_PAIR
  bool inc, outc;  // the (in_contig, out_contig) flavour
  Role role;
  bool keep;       // KEEP instantiation (offt_pass_desc::out_keep): default-policy stores.  (The TW4 instance is compiled with
                   // TW4_KEEP but registered without: nobody asks for a TW4 twin.)
  int half;        // the offt_pass_desc::half it implements: 0 full lines; 1, 2; Conv / ConvOop / ConvSum: 3
  bool operator==(const VariantKey &o) const {
    return n == o.n && prec == o.prec && inc == o.inc && outc == o.outc && role == o.role && keep == o.keep && half == o.half;
  }
};
struct VariantKeyHash {
  size_t operator()(const VariantKey &k) const {
    return ((size_t)(unsigned)k.n << 16) ^ ((size_t)(unsigned)k.half << 8) ^ ((size_t)k.role << 5) ^ ((size_t)(unsigned)k.prec << 3) ^
           (k.inc ? 4u : 0u) ^ (k.outc ? 2u : 0u) ^ (k.keep ? 1u : 0u);
  }
};

struct Variant {
  VariantKey key;
  int id;
  bool is_default;  // the default of its key: what a lookup without a matching id gets
  int cols, threads, e;
  size_t lds;
  const void *fn;
  void *modfn;      // hipFunction_t of an instance compiled at plan time (hipRTC), launched instead of fn
  bool attr_set;
  bool mixed;       // fft_panelx_k family (any split length incl. uneven, quarter or full twiddle table)
  bool full_table;
  const char *kernel;  // the __global__ template it is an instance of ("<pairs>" appended for T = f32x2)
  std::string name;
  // Role::PairYX only: the two plain entries whose bodies the kernel carries -- the KEEP contig-in / strided-out one of key.n
  // (its shape is cols, threads, e above) and the contig / contig one of the x length -- by registry id, and the x body's columns
  int pair_y_id = -1, pair_x_id = -1, pair_x_cols = 0;
};
// id of the fft_panelx_k instance a power-of-two length keeps for per-peer splits fft_panel_k cannot address
// (uneven, or not a power of two: grids split over 3, 6, ... ranks)
enum { VARIANT_ANYSPLIT = 100 };

std::vector<Variant> &registry();  // defined in offt_kernels.hip

// the launch shape of an instance and what its name says about it: from a PanelCfg, a PanelXCfg (mixed) or a shape chosen
// at plan time
struct VariantShape {
  int cols, threads, e;
  size_t lds;
  bool mixed, full_table;
  int r0, r1, r2, tpl;  // tpl: threads per line (mixed)
  const char *layout;   // of the exchange through LDS
};
inline const char *layout_name(bool split) { return split ? "split-re/im" : "packed"; }
template <typename T, int N, int E, int R0, int R1, int R2, int COLS, bool SPLIT>
VariantShape panel_shape() {
  using Cfg = PanelCfg<N, E, R0, R1, R2, COLS, SPLIT, T>;
  return VariantShape{lanes<T>::n * COLS, Cfg::NT, E, Cfg::LDS_BYTES, false, false, R0, R1, R2, 0, layout_name(SPLIT)};
}
template <typename T, int N, int TPL, int R0, int R1, int R2, int COLS, bool SPLIT>
VariantShape panelx_shape() {
  using Cfg = PanelXCfg<N, TPL, R0, R1, R2, COLS, SPLIT, T>;
  return VariantShape{COLS, Cfg::NT, Cfg::EMAX, Cfg::LDS_BYTES, true, !Cfg::QUARTER, R0, R1, R2, TPL, layout_name(SPLIT)};
}

// THE way into the registry.  `kernel`: the __global__ template `fn` (or `modfn`) is an instance of; `suffix`: what the
// name says after the layout (" half lines", " convolution", ...)
inline void add_variant(const VariantKey &key, const VariantShape &s, const void *fn, const char *kernel, const char *suffix, int id = 0,
                        bool is_default = true, void *modfn = nullptr) {
  const char *p = key.prec ? "f32" : "f64";
  char nm[224];
  if (s.mixed)
    snprintf(nm, sizeof nm, "%s N=%d mixed radix=%dx%dx%d threads/line=%d (<=%d elems/thread) cols=%d %s%s lds=%zuB%s", p, key.n, s.r0, s.r1,
             s.r2, s.tpl, s.e, s.cols, s.layout, suffix, s.lds, modfn ? " [plan-time hipRTC]" : "");
  else
    snprintf(nm, sizeof nm, "%s N=%d E=%d radix=%dx%dx%d cols=%d%s %s%s lds=%zuB", p, key.n, s.e, s.r0, s.r1, s.r2, s.cols,
             key.prec == OFFT_PREC_F32_PAIR ? " (column pairs)" : "", s.layout, suffix, s.lds);
  registry().push_back(Variant{key, id, is_default, s.cols, s.threads, s.e, s.lds, fn, modfn, false, s.mixed, s.full_table, kernel, nm});
}

// flavour bits for `defmask`: which (in_contig, out_contig) kernels use this variant by default
enum { F_CC = 1, F_SS = 2, F_CS = 4, F_SC = 8, F_ALL = 15 };

// T = f32x2: the column-pair instances (reg_variant_pair), which have no real-input or real-output form
template <typename T, int N, int E, int R0, int R1, int R2, int COLS, bool SPLIT>
void reg_variant(int id, int defmask = -1) {
  if (defmask < 0) defmask = id == 0 ? F_ALL : 0;
  constexpr bool PAIRS = lanes<T>::n == 2;
  const VariantShape s = panel_shape<T, N, E, R0, R1, R2, COLS, SPLIT>();
  auto add = [&](bool inc, bool outc, int bit, const void *fn, Role role = Role::Plain, bool keep = false, const char *kernel = nullptr) {
    add_variant(VariantKey{N, prec_of<T>(), inc, outc, role, keep, 0}, s, fn, kernel ? kernel : PAIRS ? "fft_panel_k<pairs>" : "fft_panel_k", "",
                id, (defmask & bit) != 0);
  };
  add(true, true, F_CC, (const void *)fft_panel_k<T, N, E, R0, R1, R2, COLS, true, true, SPLIT>);
  add(false, false, F_SS, (const void *)fft_panel_k<T, N, E, R0, R1, R2, COLS, false, false, SPLIT>);
  add(true, false, F_CS, (const void *)fft_panel_k<T, N, E, R0, R1, R2, COLS, true, false, SPLIT>);
  add(false, true, F_SC, (const void *)fft_panel_k<T, N, E, R0, R1, R2, COLS, false, true, SPLIT>);
  if constexpr (!PAIRS) {
    // real-input z pass: only the contiguous-read flavours of the default variant need it
    if (defmask & F_CC) add(true, true, F_CC, (const void *)fft_panel_k<T, N, E, R0, R1, R2, COLS, true, true, SPLIT, true>, Role::R2C);
    if (defmask & F_CS) add(true, false, F_CS, (const void *)fft_panel_k<T, N, E, R0, R1, R2, COLS, true, false, SPLIT, true>, Role::R2C);
    // real-output z pass (the mirror image): only the contiguous-write flavours of the default variant
    if (defmask & F_CC) add(true, true, F_CC, (const void *)fft_c2r_panel_k<T, N, E, R0, R1, R2, COLS, true, SPLIT>, Role::C2R, false, "fft_c2r_panel_k");
    if (defmask & F_SC) add(false, true, F_SC, (const void *)fft_c2r_panel_k<T, N, E, R0, R1, R2, COLS, false, SPLIT>, Role::C2R, false, "fft_c2r_panel_k");
  }
  // cache-keeping stores (out_keep): the contig-in / strided-out default, i.e. the y pass of the z-y-x schedules ...
  if (defmask & F_CS) add(true, false, F_CS, (const void *)fft_panel_k<T, N, E, R0, R1, R2, COLS, true, false, SPLIT, false, true>, Role::Plain, true);
  // ... and the contig / contig default: the x pass of the INVERSE z-y-x transform, whose planes the y pass re-reads
  if (defmask & F_CC) add(true, true, F_CC, (const void *)fft_panel_k<T, N, E, R0, R1, R2, COLS, true, true, SPLIT, false, true>, Role::Plain, true);
}

// strided / strided instance with the four-step twiddles on its stores (the first sub-pass of a long line, offt_kernels.hip)
#ifndef OFFT_TW4_KEEP
#define OFFT_TW4_KEEP 1
#endif
constexpr bool TW4_KEEP = OFFT_TW4_KEEP != 0;  // its stores go to the scratch the second sub-pass reads right away: default cache policy
template <typename T, int N, int E, int R0, int R1, int R2, int COLS, bool SPLIT>
void reg_variant_tw4(int id) {
  VariantShape s = panel_shape<T, N, E, R0, R1, R2, COLS, SPLIT>();
  s.layout = "four-step twiddles on the stores";  // (its name says this where the others say the layout)
  add_variant(VariantKey{N, prec_of<T>(), false, false, Role::TW4, false, 0}, s,
              (const void *)fft_panel_k<T, N, E, R0, R1, R2, COLS, false, false, SPLIT, false, TW4_KEEP, true>, "fft_panel_k", "", id);
}

// column-pair instances of fft_panel_k (T = f32x2, under OFFT_PREC_F32_PAIR); `defmask` says for which flavours an eligible
// descriptor prefers the pair kernel.
template <int N, int E, int R0, int R1, int R2, int COLS, bool SPLIT>
void reg_variant_pair(int id, int defmask) {
  reg_variant<f32x2, N, E, R0, R1, R2, COLS, SPLIT>(id, defmask);
}

// fused convolution instances (fft_conv_panel_k, offt_reg_conv_*.hip): contiguous lines, plus a twin with cache-keeping
// stores for the alternating launches over groups of z-planes (offt_host.c)
template <typename T, int N, int E, int R0, int R1, int R2, int COLS, bool SPLIT>
void reg_variant_conv() {
  const VariantShape s = panel_shape<T, N, E, R0, R1, R2, COLS, SPLIT>();
  auto add = [&](bool keep, const void *fn) {
    add_variant(VariantKey{N, prec_of<T>(), true, true, Role::Conv, keep, 0}, s, fn, "fft_conv_panel_k", " convolution");
  };
  add(false, (const void *)fft_conv_panel_k<T, N, E, R0, R1, R2, COLS, SPLIT, false>);
  add(true, (const void *)fft_conv_panel_k<T, N, E, R0, R1, R2, COLS, SPLIT, true>);
}

// half-line instances (fft_half_panel_k, offt_reg_half_*.hip).  FLAV says which of the four (flavour, bit) forms of the
// z-y-x half-box schedule and its mirror this shape is instantiated for; T = f32x2 registers column-pair instances.
enum { H_CS1 = 1, H_CC1 = 2, H_CC2 = 4, H_SC2 = 8, H_ALL = 15 };
template <typename T, int N, int E, int R0, int R1, int R2, int COLS, bool SPLIT, int FLAV = H_ALL>
void reg_variant_half() {
  const VariantShape s = panel_shape<T, N, E, R0, R1, R2, COLS, SPLIT>();
  auto add = [&](bool inc, bool outc, int half, const void *fn) {
    add_variant(VariantKey{N, prec_of<T>(), inc, outc, Role::Plain, false, half}, s, fn,
                lanes<T>::n == 2 ? "fft_half_panel_k<pairs>" : "fft_half_panel_k", " half lines");
  };
  if constexpr ((FLAV & H_CS1) != 0) add(true, false, 1, (const void *)fft_half_panel_k<T, N, E, R0, R1, R2, COLS, true, false, SPLIT, 1>);
  if constexpr ((FLAV & H_CC1) != 0) add(true, true, 1, (const void *)fft_half_panel_k<T, N, E, R0, R1, R2, COLS, true, true, SPLIT, 1>);
  if constexpr ((FLAV & H_CC2) != 0) add(true, true, 2, (const void *)fft_half_panel_k<T, N, E, R0, R1, R2, COLS, true, true, SPLIT, 2>);
  if constexpr ((FLAV & H_SC2) != 0) add(false, true, 2, (const void *)fft_half_panel_k<T, N, E, R0, R1, R2, COLS, false, true, SPLIT, 2>);
}

// the real ends of a half-box chain (fft_half_r2c_panel_k, fft_half_c2r_panel_k; offt_reg_half_real_*.hip): one column per
// lane, keyed by R2C / C2R together with half, so that no complex or full-line lookup finds them
template <typename T, int N, int E, int R0, int R1, int R2, int COLS, bool SPLIT>
void reg_variant_half_real() {
  static_assert(lanes<T>::n == 1, "real rows: one column per lane");
  const VariantShape s = panel_shape<T, N, E, R0, R1, R2, COLS, SPLIT>();
  add_variant(VariantKey{N, prec_of<T>(), true, false, Role::R2C, false, 1}, s, (const void *)fft_half_r2c_panel_k<T, N, E, R0, R1, R2, COLS, SPLIT>,
              "fft_half_r2c_panel_k", " half lines, real rows");
  add_variant(VariantKey{N, prec_of<T>(), false, true, Role::C2R, false, 2}, s, (const void *)fft_half_c2r_panel_k<T, N, E, R0, R1, R2, COLS, SPLIT>,
              "fft_half_c2r_panel_k", " half lines, real rows");
}

// fused convolution on half lines (fft_conv_half_panel_k): the shapes of reg_variant_conv
template <typename T, int N, int E, int R0, int R1, int R2, int COLS, bool SPLIT>
void reg_variant_conv_half() {
  add_variant(VariantKey{N, prec_of<T>(), true, true, Role::Conv, false, 3}, panel_shape<T, N, E, R0, R1, R2, COLS, SPLIT>(),
              (const void *)fft_conv_half_panel_k<T, N, E, R0, R1, R2, COLS, SPLIT, false>, "fft_conv_half_panel_k", " convolution on half lines");
}

// out-of-place fused convolution (fft_conv_oop_panel_k, fft_conv_oop_half_panel_k; offt_reg_conv_oop_*.hip): the shapes of
// reg_variant_conv, full lines and half lines, each plain and with cache-keeping stores
template <typename T, int N, int E, int R0, int R1, int R2, int COLS, bool SPLIT>
void reg_variant_conv_oop() {
  const VariantShape s = panel_shape<T, N, E, R0, R1, R2, COLS, SPLIT>();
  auto add = [&](bool keep, int half, const void *fn) {
    add_variant(VariantKey{N, prec_of<T>(), true, true, Role::ConvOop, keep, half}, s, fn, half ? "fft_conv_oop_half_panel_k" : "fft_conv_oop_panel_k",
                half ? " out-of-place convolution on half lines" : " out-of-place convolution");
  };
  add(false, 0, (const void *)fft_conv_oop_panel_k<T, N, E, R0, R1, R2, COLS, SPLIT, false>);
  add(true, 0, (const void *)fft_conv_oop_panel_k<T, N, E, R0, R1, R2, COLS, SPLIT, true>);
  add(false, 3, (const void *)fft_conv_oop_half_panel_k<T, N, E, R0, R1, R2, COLS, SPLIT, false>);
  add(true, 3, (const void *)fft_conv_oop_half_panel_k<T, N, E, R0, R1, R2, COLS, SPLIT, true>);
}

// multi-input fused convolution (fft_conv_sum_panel_k, fft_conv_sum_half_panel_k; offt_reg_conv_sum_*.hip): shapes of their
// own (the accumulator doubles the data registers: fewer columns where that buys the register budget), full lines and half
// lines, each plain and with cache-keeping stores
template <typename T, int N, int E, int R0, int R1, int R2, int COLS, bool SPLIT>
void reg_variant_conv_sum() {
  const VariantShape s = panel_shape<T, N, E, R0, R1, R2, COLS, SPLIT>();
  auto add = [&](bool keep, int half, const void *fn) {
    add_variant(VariantKey{N, prec_of<T>(), true, true, Role::ConvSum, keep, half}, s, fn, half ? "fft_conv_sum_half_panel_k" : "fft_conv_sum_panel_k",
                half ? " multi-input convolution on half lines" : " multi-input convolution");
  };
  add(false, 0, (const void *)fft_conv_sum_panel_k<T, N, E, R0, R1, R2, COLS, SPLIT, false>);
  add(true, 0, (const void *)fft_conv_sum_panel_k<T, N, E, R0, R1, R2, COLS, SPLIT, true>);
  add(false, 3, (const void *)fft_conv_sum_half_panel_k<T, N, E, R0, R1, R2, COLS, SPLIT, false>);
  add(true, 3, (const void *)fft_conv_sum_half_panel_k<T, N, E, R0, R1, R2, COLS, SPLIT, true>);
}

// pseudo-spectral product (fft_prod_panel_k; offt_reg_prod_*.hip): strided lines on both sides, full lines, no cache-keeping
// twin; shapes of their own (the accumulator doubles the data registers, as in reg_variant_conv_sum)
template <typename T, int N, int E, int R0, int R1, int R2, int COLS, bool SPLIT>
void reg_variant_prod() {
  add_variant(VariantKey{N, prec_of<T>(), false, false, Role::Prod, false, 0}, panel_shape<T, N, E, R0, R1, R2, COLS, SPLIT>(),
              (const void *)fft_prod_panel_k<T, N, E, R0, R1, R2, COLS, SPLIT>, "fft_prod_panel_k", " product");
}
// ... of real fields (fft_prod_real_panel_k; offt_reg_prod_real_*.hip): N the real length.  WPS: prod_real_wps
template <typename T, int N, int E, int R0, int R1, int R2, int COLS, bool SPLIT, int WPS = 0>
void reg_variant_prod_real() {
  add_variant(VariantKey{N, prec_of<T>(), false, false, Role::ProdReal, false, 0}, panel_shape<T, N, E, R0, R1, R2, COLS, SPLIT>(),
              (const void *)fft_prod_real_panel_k<T, N, E, R0, R1, R2, COLS, SPLIT, WPS>, "fft_prod_real_panel_k", " real product");
}

// filtered forward and filtered inverse (fft_filt_fwd_panel_k, fft_filt_inv_panel_k; offt_reg_spec_*.hip): the shapes of
// reg_variant_conv, each plain and with cache-keeping stores
template <typename T, int N, int E, int R0, int R1, int R2, int COLS, bool SPLIT>
void reg_variant_filt() {
  const VariantShape s = panel_shape<T, N, E, R0, R1, R2, COLS, SPLIT>();
  auto add = [&](Role role, bool keep, const void *fn) {
    add_variant(VariantKey{N, prec_of<T>(), true, true, role, keep, 0}, s, fn, role == Role::FiltFwd ? "fft_filt_fwd_panel_k" : "fft_filt_inv_panel_k",
                role == Role::FiltFwd ? " filtered forward" : " filtered inverse");
  };
  add(Role::FiltFwd, false, (const void *)fft_filt_fwd_panel_k<T, N, E, R0, R1, R2, COLS, SPLIT, false>);
  add(Role::FiltFwd, true, (const void *)fft_filt_fwd_panel_k<T, N, E, R0, R1, R2, COLS, SPLIT, true>);
  add(Role::FiltInv, false, (const void *)fft_filt_inv_panel_k<T, N, E, R0, R1, R2, COLS, SPLIT, false>);
  add(Role::FiltInv, true, (const void *)fft_filt_inv_panel_k<T, N, E, R0, R1, R2, COLS, SPLIT, true>);
}

// mixed-radix (2^a 3^b 5^c) panel kernel: TPL threads per line instead of elements per thread.
// FLAV limits which (in_contig, out_contig) flavours are instantiated at all (compile time), defmask says for
// which of them this variant is the default.
template <typename T, int N, int TPL, int R0, int R1, int R2, int COLS, bool SPLIT, int FLAV = F_ALL>
void reg_variantx(int id, int defmask = -1) {
  if (defmask < 0) defmask = id == 0 ? F_ALL : 0;
  defmask &= FLAV;
  const VariantShape s = panelx_shape<T, N, TPL, R0, R1, R2, COLS, SPLIT>();
  auto add = [&](bool inc, bool outc, int bit, const void *fn, Role role = Role::Plain) {
    add_variant(VariantKey{N, prec_of<T>(), inc, outc, role, false, 0}, s, fn, role == Role::C2R ? "fft_c2r_panelx_k" : "fft_panelx_k", "", id,
                (defmask & bit) != 0);
  };
  if constexpr ((FLAV & F_CC) != 0) {
    add(true, true, F_CC, (const void *)fft_panelx_k<T, N, TPL, R0, R1, R2, COLS, true, true, SPLIT>);
    if (defmask & F_CC) add(true, true, F_CC, (const void *)fft_panelx_k<T, N, TPL, R0, R1, R2, COLS, true, true, SPLIT, true>, Role::R2C);
    // (real output: also the any-split instances of the power-of-two lengths, so that the inverse's z pass of a grid split
    //  over 3, 5, 6 ... ranks runs here rather than on the any-length kernel)
    if ((defmask & F_CC) || id == VARIANT_ANYSPLIT) add(true, true, F_CC, (const void *)fft_c2r_panelx_k<T, N, TPL, R0, R1, R2, COLS, true, SPLIT>, Role::C2R);
  }
  if constexpr ((FLAV & F_SS) != 0) add(false, false, F_SS, (const void *)fft_panelx_k<T, N, TPL, R0, R1, R2, COLS, false, false, SPLIT>);
  if constexpr ((FLAV & F_CS) != 0) {
    add(true, false, F_CS, (const void *)fft_panelx_k<T, N, TPL, R0, R1, R2, COLS, true, false, SPLIT>);
    if (defmask & F_CS) add(true, false, F_CS, (const void *)fft_panelx_k<T, N, TPL, R0, R1, R2, COLS, true, false, SPLIT, true>, Role::R2C);
  }
  if constexpr ((FLAV & F_SC) != 0) {
    add(false, true, F_SC, (const void *)fft_panelx_k<T, N, TPL, R0, R1, R2, COLS, false, true, SPLIT>);
    if ((defmask & F_SC) || id == VARIANT_ANYSPLIT) add(false, true, F_SC, (const void *)fft_c2r_panelx_k<T, N, TPL, R0, R1, R2, COLS, false, SPLIT>, Role::C2R);
  }
}

// half-line instances of the mixed-radix kernel (fft_half_panelx_k, offt_reg_half_mixed_*.hip): the four forms of
// reg_variant_half, one column per lane.  FLAV as there: a length whose full-line kernel has a narrow contiguous /
// contiguous shape registers that shape for H_CC1 | H_CC2 and the wide one for H_CS1 | H_SC2.
template <typename T, int N, int TPL, int R0, int R1, int R2, int COLS, bool SPLIT, int FLAV = H_ALL>
void reg_variantx_half() {
  static_assert(PanelXCfg<N, TPL, R0, R1, R2, COLS, SPLIT, T>::QUARTER, "half lines: N is a multiple of 4");
  const VariantShape s = panelx_shape<T, N, TPL, R0, R1, R2, COLS, SPLIT>();
  auto add = [&](bool inc, bool outc, int half, const void *fn) {
    add_variant(VariantKey{N, prec_of<T>(), inc, outc, Role::Plain, false, half}, s, fn, "fft_half_panelx_k", " half lines");
  };
  if constexpr ((FLAV & H_CS1) != 0) add(true, false, 1, (const void *)fft_half_panelx_k<T, N, TPL, R0, R1, R2, COLS, true, false, SPLIT, 1>);
  if constexpr ((FLAV & H_CC1) != 0) add(true, true, 1, (const void *)fft_half_panelx_k<T, N, TPL, R0, R1, R2, COLS, true, true, SPLIT, 1>);
  if constexpr ((FLAV & H_CC2) != 0) add(true, true, 2, (const void *)fft_half_panelx_k<T, N, TPL, R0, R1, R2, COLS, true, true, SPLIT, 2>);
  if constexpr ((FLAV & H_SC2) != 0) add(false, true, 2, (const void *)fft_half_panelx_k<T, N, TPL, R0, R1, R2, COLS, false, true, SPLIT, 2>);
}

// the real ends of a half-box chain at a mixed-radix length (fft_half_r2c_panelx_k, fft_half_c2r_panelx_k;
// offt_reg_half_real_mixed_*.hip): keyed by R2C / C2R together with half, so that no complex or full-line lookup finds
// them; they are `mixed`, and pick_half hands them out only to a descriptor that carries bit 4 of offt_pass_desc::half
template <typename T, int N, int TPL, int R0, int R1, int R2, int COLS, bool SPLIT>
void reg_variantx_half_real() {
  static_assert(PanelXCfg<N, TPL, R0, R1, R2, COLS, SPLIT, T>::QUARTER, "half lines: N is a multiple of 4");
  const VariantShape s = panelx_shape<T, N, TPL, R0, R1, R2, COLS, SPLIT>();
  add_variant(VariantKey{N, prec_of<T>(), true, false, Role::R2C, false, 1}, s, (const void *)fft_half_r2c_panelx_k<T, N, TPL, R0, R1, R2, COLS, SPLIT>,
              "fft_half_r2c_panelx_k", " half lines, real rows");
  add_variant(VariantKey{N, prec_of<T>(), false, true, Role::C2R, false, 2}, s, (const void *)fft_half_c2r_panelx_k<T, N, TPL, R0, R1, R2, COLS, SPLIT>,
              "fft_half_c2r_panelx_k", " half lines, real rows");
}

// fused convolution instances of the mixed-radix kernel (fft_conv_panelx_k, offt_reg_conv_mixed_*.hip; picked only with
// offt_filter_desc::mixed): contiguous lines, no cache-keeping twin ...
template <typename T, int N, int TPL, int R0, int R1, int R2, int COLS, bool SPLIT>
void reg_variantx_conv() {
  add_variant(VariantKey{N, prec_of<T>(), true, true, Role::Conv, false, 0}, panelx_shape<T, N, TPL, R0, R1, R2, COLS, SPLIT>(),
              (const void *)fft_conv_panelx_k<T, N, TPL, R0, R1, R2, COLS, SPLIT>, "fft_conv_panelx_k", " convolution");
}

// ... and on half lines (fft_conv_half_panelx_k): the same shapes
template <typename T, int N, int TPL, int R0, int R1, int R2, int COLS, bool SPLIT>
void reg_variantx_conv_half() {
  add_variant(VariantKey{N, prec_of<T>(), true, true, Role::Conv, false, 3}, panelx_shape<T, N, TPL, R0, R1, R2, COLS, SPLIT>(),
              (const void *)fft_conv_half_panelx_k<T, N, TPL, R0, R1, R2, COLS, SPLIT>, "fft_conv_half_panelx_k", " convolution on half lines");
}

// ... and out of place (fft_conv_oop_panelx_k, fft_conv_oop_half_panelx_k; offt_reg_conv_oop_mixed_*.hip; picked only with
// both bits of offt_filter_desc::mixed): the shapes of reg_variantx_conv, full lines and half lines, no cache-keeping twin
template <typename T, int N, int TPL, int R0, int R1, int R2, int COLS, bool SPLIT>
void reg_variantx_conv_oop() {
  const VariantShape s = panelx_shape<T, N, TPL, R0, R1, R2, COLS, SPLIT>();
  add_variant(VariantKey{N, prec_of<T>(), true, true, Role::ConvOop, false, 0}, s, (const void *)fft_conv_oop_panelx_k<T, N, TPL, R0, R1, R2, COLS, SPLIT>,
              "fft_conv_oop_panelx_k", " out-of-place convolution");
  add_variant(VariantKey{N, prec_of<T>(), true, true, Role::ConvOop, false, 3}, s, (const void *)fft_conv_oop_half_panelx_k<T, N, TPL, R0, R1, R2, COLS, SPLIT>,
              "fft_conv_oop_half_panelx_k", " out-of-place convolution on half lines");
}

// multi-input fused convolution at a mixed-radix length (fft_conv_sum_panelx_k, fft_conv_sum_half_panelx_k;
// offt_reg_conv_sum_mixed_*.hip; picked only with bits 1 and 3 of offt_filter_desc::mixed): shapes of their own (the
// accumulator on top of convx_body's registers), full lines and half lines, no cache-keeping twin
template <typename T, int N, int TPL, int R0, int R1, int R2, int COLS, bool SPLIT>
void reg_variantx_conv_sum() {
  const VariantShape s = panelx_shape<T, N, TPL, R0, R1, R2, COLS, SPLIT>();
  add_variant(VariantKey{N, prec_of<T>(), true, true, Role::ConvSum, false, 0}, s, (const void *)fft_conv_sum_panelx_k<T, N, TPL, R0, R1, R2, COLS, SPLIT>,
              "fft_conv_sum_panelx_k", " multi-input convolution");
  add_variant(VariantKey{N, prec_of<T>(), true, true, Role::ConvSum, false, 3}, s, (const void *)fft_conv_sum_half_panelx_k<T, N, TPL, R0, R1, R2, COLS, SPLIT>,
              "fft_conv_sum_half_panelx_k", " multi-input convolution on half lines");
}

// filtered forward and filtered inverse at a mixed-radix length (fft_filt_fwd_panelx_k, fft_filt_inv_panelx_k;
// offt_reg_spec_mixed_*.hip; picked only with bit 4 of offt_filter_desc::mixed): full lines, no cache-keeping twin
template <typename T, int N, int TPL, int R0, int R1, int R2, int COLS, bool SPLIT>
void reg_variantx_spec() {
  const VariantShape s = panelx_shape<T, N, TPL, R0, R1, R2, COLS, SPLIT>();
  add_variant(VariantKey{N, prec_of<T>(), true, true, Role::FiltFwd, false, 0}, s, (const void *)fft_filt_fwd_panelx_k<T, N, TPL, R0, R1, R2, COLS, SPLIT>,
              "fft_filt_fwd_panelx_k", " filtered forward");
  add_variant(VariantKey{N, prec_of<T>(), true, true, Role::FiltInv, false, 0}, s, (const void *)fft_filt_inv_panelx_k<T, N, TPL, R0, R1, R2, COLS, SPLIT>,
              "fft_filt_inv_panelx_k", " filtered inverse");
}

// instantiation groups (offt_reg_*.hip)
void reg_pow2_f64();
void reg_pow2_f64_1024();
void reg_pow2_f64_anysplit();
void reg_pair_yx_f64();
void reg_pow2_f32();
void reg_pow2_f32_big();
void reg_pow2_f32_anysplit();
void reg_pow2_f32_pair();
void reg_pow2_tw4();
void reg_mixed_f64_a();
void reg_mixed_f64_b();
void reg_mixed_f64_c();
void reg_mixed_f64_d();
void reg_mixed_f64_e();
void reg_mixed_f32_a();
void reg_mixed_f32_b();
void reg_conv_f64();
void reg_conv_f32();
void reg_conv_oop_f64();
void reg_conv_oop_f32();
void reg_conv_mixed_f64();
void reg_conv_mixed_f32();
void reg_conv_oop_mixed_f64();
void reg_conv_oop_mixed_f32();
void reg_conv_sum_f64();
void reg_conv_sum_f32();
void reg_conv_sum_mixed_f64();
void reg_conv_sum_mixed_f32();
void reg_spec_f64();
void reg_spec_f32();
void reg_spec_mixed_f64();
void reg_spec_mixed_f32();
void reg_prod_f64();
void reg_prod_f32();
void reg_prod_real_f64();
void reg_prod_real_f32();
void reg_half_f64();
void reg_half_f32();
void reg_half_real_f64();
void reg_half_real_f32();
void reg_half_mixed_f64();
void reg_half_mixed_f32();
void reg_half_real_mixed_f64();
void reg_half_real_mixed_f32();
void reg_dev();

}  // namespace offtk
