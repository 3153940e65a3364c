// offt_kernels.hip -- C ABI (offt_hipk.h), kernel registry, twiddle tables and launchers of the
// hand-written CDNA4 (gfx950) kernels; the panel kernels themselves are in offt_panel.hpp.
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

#include <hip/hip_runtime.h>
#include <type_traits>
#include <mutex>
#include <map>
#include <vector>
#include <string>
#include <cstdio>
#include <cmath>
#include <cstring>
#include <cstdlib>
#include <dlfcn.h>
#include <unordered_map>
#include <algorithm>
#include <hip/hiprtc.h>
#include "offt_hipk.h"
#include "offt_panel.hpp"
#include "offt_bluestein.hpp"
#include "offt_rtc_source.inc"

namespace offtk {
std::vector<Variant> &registry() {
  static std::vector<Variant> r;
  return r;
}
std::vector<BlueVariant> &blue_registry() {
  static std::vector<BlueVariant> r;
  return r;
}
}  // namespace offtk

namespace {
using namespace offtk;

thread_local char g_err[512] = "";
#define HIPK_CHECK(call)                                                          \
  do {                                                                            \
    hipError_t e_ = (call);                                                       \
    if (e_ != hipSuccess) {                                                       \
      snprintf(g_err, sizeof g_err, "%s:%d: %s -> %s", __FILE__, __LINE__, #call, \
               hipGetErrorString(e_));                                            \
      return -1;                                                                  \
    }                                                                             \
  } while (0)
// ---------------------------------------------------------------------------
// Any-length kernel: mixed-radix Stockham in LDS with run-time radices.
// It exists so that every length the reference accepts (FFTW takes any N) is
// transformed correctly and at a tolerable cost; lengths with a compile-time
// register kernel never come here, nor do power-of-two splits.
//
// N = r0 * r1 * ... (prime factors, pairs of 2 merged to 4).  One workgroup owns
// COLS lines in two ping-pong LDS images.  A work item of stage s produces ONE
// output of one radix-r butterfly:
//   y[(q-k) r + k + j Ns] = sum_t x[q + t N/r] * w_N^(k t M) * w_r^(j t),
//   k = q mod Ns, M = N / (Ns r)
// with exact table twiddles w_N^m (m = 0..N-1, staged in LDS when it fits).
// Radices 2, 3, 4, 5 are done as whole butterflies (r loads, r-1 twiddles, a
// constant-coefficient DFT, r stores); any other prime radix produces one
// output per work item with r multiply-adds, so a line costs at most
// N * sum(r_s) instead of N^2 and a prime N degenerates to the plain DFT.
// Also handles the reference's uneven A2AV per-peer splits on either side and
// the real-input and real-output z passes.
// ---------------------------------------------------------------------------
#define OFFT_MIX_MAXFAC 16
struct GenArgs {
  long long in_axis, in_col, in_b1, in_b2, in_blk;
  long long out_axis, out_col, out_b1, out_b2, out_blk;
  int in_split, in_nfloor, out_split, out_nfloor;
  int n, ncols, nb1, ncp, cols;
  int in_contig, out_contig;
  int conj;
  int real_in;      // offt_pass_desc::real_input: 1 real input, 2 real output
  int tw_in_lds;
  unsigned xcd_lim, xcd_gshift;
  int nfac;
  int fac[OFFT_MIX_MAXFAC];
  double scale;
  const long long *in_tab, *out_tab;  // per-block element offsets (offt_pass_desc::in_block_tab / out_block_tab) or nullptr
};

__device__ __forceinline__ long long split_off(int k, int split, int nfloor, long long blk, long long axis, const long long *tab) {
  if (split == 0 && nfloor == 0) return (long long)k * axis;  // no split
  int a, r;
  if (nfloor > 0 && k >= split * nfloor) {
    int kk = k - split * nfloor;
    a = nfloor + kk / (split + 1);
    r = kk % (split + 1);
  } else {
    a = k / split;
    r = k % split;
  }
  return (tab ? tab[a] : (long long)a * blk) + (long long)r * axis;
}

// one radix-R butterfly of the any-length kernel: inputs xin[t * is], t = 0..R-1, twiddled by
// w_N^(kM t) from the table, outputs yout[j * os]
template <typename T, int R>
__device__ __forceinline__ void mixed_butterfly(const typename vec2<T>::type *xin, typename vec2<T>::type *yout,
                                                int is, int os, int kM, const typename vec2<T>::type *tw) {
  using V2 = typename vec2<T>::type;
  cx<T> v[R];
#pragma unroll
  for (int t = 0; t < R; ++t) {
    const V2 a = xin[t * is];
    if (t == 0) { v[0] = cx<T>{a.x, a.y}; }
    else {
      const V2 w = tw[kM * t];
      v[t] = cx<T>{a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x};
    }
  }
  cx<T> o[R];
  if constexpr (R == 2) {
    o[0] = cx<T>{v[0].x + v[1].x, v[0].y + v[1].y};
    o[1] = cx<T>{v[0].x - v[1].x, v[0].y - v[1].y};
  } else if constexpr (R == 3) {
    constexpr T S3 = (T)0.86602540378443864676;  // sin(2 pi / 3)
    const cx<T> s{v[1].x + v[2].x, v[1].y + v[2].y}, d{v[1].x - v[2].x, v[1].y - v[2].y};
    const cx<T> t{v[0].x - (T)0.5 * s.x, v[0].y - (T)0.5 * s.y};
    const cx<T> e{S3 * d.y, -S3 * d.x};  // -i * S3 * d
    o[0] = cx<T>{v[0].x + s.x, v[0].y + s.y};
    o[1] = cx<T>{t.x + e.x, t.y + e.y};
    o[2] = cx<T>{t.x - e.x, t.y - e.y};
  } else if constexpr (R == 4) {
    const cx<T> a{v[0].x + v[2].x, v[0].y + v[2].y}, b{v[0].x - v[2].x, v[0].y - v[2].y};
    const cx<T> c{v[1].x + v[3].x, v[1].y + v[3].y}, d{v[1].x - v[3].x, v[1].y - v[3].y};
    o[0] = cx<T>{a.x + c.x, a.y + c.y};
    o[2] = cx<T>{a.x - c.x, a.y - c.y};
    o[1] = cx<T>{b.x + d.y, b.y - d.x};  // b - i d
    o[3] = cx<T>{b.x - d.y, b.y + d.x};  // b + i d
  } else {
    static_assert(R == 5, "radix");
    constexpr T C1 = (T)0.30901699437494742410, C2 = (T)-0.80901699437494742410;   // cos(2 pi/5), cos(4 pi/5)
    constexpr T S1 = (T)0.95105651629515357212, S2 = (T)0.58778525229247312917;    // sin(2 pi/5), sin(4 pi/5)
    const cx<T> s1{v[1].x + v[4].x, v[1].y + v[4].y}, s2{v[2].x + v[3].x, v[2].y + v[3].y};
    const cx<T> d1{v[1].x - v[4].x, v[1].y - v[4].y}, d2{v[2].x - v[3].x, v[2].y - v[3].y};
    const cx<T> p1{v[0].x + C1 * s1.x + C2 * s2.x, v[0].y + C1 * s1.y + C2 * s2.y};
    const cx<T> p2{v[0].x + C2 * s1.x + C1 * s2.x, v[0].y + C2 * s1.y + C1 * s2.y};
    const cx<T> q1{S1 * d1.x + S2 * d2.x, S1 * d1.y + S2 * d2.y};
    const cx<T> q2{S2 * d1.x - S1 * d2.x, S2 * d1.y - S1 * d2.y};
    o[0] = cx<T>{v[0].x + s1.x + s2.x, v[0].y + s1.y + s2.y};
    o[1] = cx<T>{p1.x + q1.y, p1.y - q1.x};  // p1 - i q1
    o[4] = cx<T>{p1.x - q1.y, p1.y + q1.x};
    o[2] = cx<T>{p2.x + q2.y, p2.y - q2.x};
    o[3] = cx<T>{p2.x - q2.y, p2.y + q2.x};
  }
#pragma unroll
  for (int j = 0; j < R; ++j) { V2 w; w.x = o[j].x; w.y = o[j].y; yout[j * os] = w; }
}

template <typename T>
__global__ void __launch_bounds__(1024)
fft_mixed_k(GenArgs a, const typename vec2<T>::type *in, typename vec2<T>::type *out,
            const typename vec2<T>::type *twf) {
  using V2 = typename vec2<T>::type;
  extern __shared__ __align__(16) unsigned char smem[];
  const int N = a.n, C = a.cols;
  V2 *buf0 = reinterpret_cast<V2 *>(smem);
  V2 *buf1 = buf0 + (size_t)C * N;
  V2 *twl = buf1 + (size_t)C * N;
  const V2 *tw = a.tw_in_lds ? twl : twf;
  const int tid = threadIdx.x, NT = blockDim.x;
  const unsigned bid = panel_of_block(blockIdx.x, a.xcd_lim, a.xcd_gshift);
  const int cp = bid % (unsigned)a.ncp;
  const unsigned rest = bid / (unsigned)a.ncp;
  const int b1 = rest % (unsigned)a.nb1;
  const int b2 = rest / (unsigned)a.nb1;
  const int c0 = cp * C;
  const int nc = (a.ncols - c0 < C) ? a.ncols - c0 : C;  // valid columns of this panel
  const long long ibase = (long long)b1 * a.in_b1 + (long long)b2 * a.in_b2;
  const long long obase = (long long)b1 * a.out_b1 + (long long)b2 * a.out_b2;

  if (a.tw_in_lds)
    for (int i = tid; i < N; i += NT) twl[i] = twf[i];
  const float invN = 1.0f / (float)N, invnc = 1.0f / (float)nc;
  for (int i = tid; i < nc * N; i += NT) {
    int c, n;
    if (a.in_contig) { c = fdiv(i, N, invN); n = i - c * N; } else { n = fdiv(i, nc, invnc); c = i - n * nc; }
    const V2 *src = in + ibase + (long long)(c0 + c) * a.in_col;
    V2 x;
    if (a.real_in == 1) { x.x = reinterpret_cast<const T *>(src)[n]; x.y = 0; }
    else if (a.real_in == 2) {  // the conjugate-symmetric extension of the n/2+1 stored values
      const bool lo = 2 * n <= N;
      x = src[split_off(lo ? n : N - n, a.in_split, a.in_nfloor, a.in_blk, a.in_axis, a.in_tab)];
      if (!lo) x.y = -x.y;
    } else x = src[split_off(n, a.in_split, a.in_nfloor, a.in_blk, a.in_axis, a.in_tab)];
    if (a.conj) x.y = -x.y;
    buf0[c * N + n] = x;
  }
  __syncthreads();

  V2 *x = buf0, *y = buf1;
  int Ns = 1;
  for (int s = 0; s < a.nfac; ++s) {
    const int r = a.fac[s];
    const int nq = N / r;        // butterflies per line
    const int M = N / (Ns * r);  // twiddle step
    if (r <= 5) {
      // whole radix-2/3/4/5 butterflies: r loads, r-1 table twiddles, constant-coefficient DFT, r stores
      const float invnq = 1.0f / (float)nq, invNs = 1.0f / (float)Ns;
      for (int i = tid; i < nc * nq; i += NT) {
        const int c = fdiv(i, nq, invnq), q = i - c * nq, k = q - fdiv(q, Ns, invNs) * Ns;
        switch (r) {
          case 2: mixed_butterfly<T, 2>(x + c * N + q, y + c * N + (q - k) * 2 + k, nq, Ns, k * M, tw); break;
          case 3: mixed_butterfly<T, 3>(x + c * N + q, y + c * N + (q - k) * 3 + k, nq, Ns, k * M, tw); break;
          case 4: mixed_butterfly<T, 4>(x + c * N + q, y + c * N + (q - k) * 4 + k, nq, Ns, k * M, tw); break;
          default: mixed_butterfly<T, 5>(x + c * N + q, y + c * N + (q - k) * 5 + k, nq, Ns, k * M, tw); break;
        }
      }
    } else {
      // any other (prime) radix: one output per work item, r multiply-adds
      for (int i = tid; i < nc * N; i += NT) {
        const int c = i / N;
        const int o = i - c * N;   // (q, j) of this output
        const int q = o % nq, j = o / nq;
        const int k = q % Ns;
        const V2 *xc = x + c * N + q;
        T sr = 0, si = 0;
        int e1 = 0;                // k * t * M       (< N)
        int jt = 0;                // (j * t) mod r
        const int kM = k * M;
        for (int t = 0; t < r; ++t) {
          int e = e1 + jt * nq;    // + (N/r) * ((j t) mod r)
          if (e >= N) e -= N;
          const V2 w = tw[e];
          const V2 v = xc[t * nq];
          sr += v.x * w.x - v.y * w.y;
          si += v.x * w.y + v.y * w.x;
          e1 += kM;
          jt += j;
          if (jt >= r) jt -= r;
        }
        V2 res; res.x = sr; res.y = si;
        y[c * N + (q - k) * r + k + j * Ns] = res;
      }
    }
    __syncthreads();
    V2 *tmp = x; x = y; y = tmp;
    Ns *= r;
  }

  const int kend = a.real_in == 1 ? N / 2 + 1 : N;
  const float invkend = 1.0f / (float)kend;
  for (int i = tid; i < nc * kend; i += NT) {
    int c, k;
    if (a.out_contig) { c = fdiv(i, kend, invkend); k = i - c * kend; } else { k = fdiv(i, nc, invnc); c = i - k * nc; }
    V2 v = x[c * N + k];
    V2 w;
    w.x = v.x * (T)a.scale;
    w.y = (a.conj ? -v.y : v.y) * (T)a.scale;
    V2 *dst = out + obase + (long long)(c0 + c) * a.out_col;
    if (a.real_in == 2) reinterpret_cast<T *>(dst)[k] = w.x;  // n reals at the head of the row
    else dst[split_off(k, a.out_split, a.out_nfloor, a.out_blk, a.out_axis, a.out_tab)] = w;
  }
}

// ---------------------------------------------------------------------------
// strided 3-D copy (permutation); tile-transposed through LDS when the unit
// strides of input and output sit on different dimensions.
// ---------------------------------------------------------------------------
template <typename V2>
__global__ void __launch_bounds__(256)
copy3d_k(const V2 *in, V2 *out, int n0, int n1, int n2, long long is0, long long is1, long long is2,
         long long os0, long long os1, long long os2) {
  long long total = (long long)n0 * n1 * n2;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    int i2 = (int)(i % n2);
    long long r = i / n2;
    int i1 = (int)(r % n1);
    int i0 = (int)(r / n1);
    out[i0 * os0 + i1 * os1 + i2 * os2] = in[i0 * is0 + i1 * is1 + i2 * is2];
  }
}

// out = in * filter over a strided box (offt_hipk_pointwise_oop): pointwise_k with a separate destination at the same
// offsets -- the source stays as it was, so that several filters can be applied to one spectrum.  16 B per lane,
// non-temporal both ways.
template <typename T, bool CPLX, int EPL>
__global__ void __launch_bounds__(256)
pointwise_oop_k(const typename vec2<T>::type *in, typename vec2<T>::type *out, const void *filter, int n1, int n2, long long s0, long long s1,
                long long s2, long long rows) {
  using V2 = typename vec2<T>::type;
  const int i2 = (blockIdx.x * 256 + threadIdx.x) * EPL;
  if (i2 >= n2) return;
  for (long long r = blockIdx.y; r < rows; r += gridDim.y) {
    const long long i1 = r % n1, i0 = r / n1;
    const long long o = i0 * s0 + i1 * s1 + (long long)i2 * s2;
    if constexpr (EPL == 2) {  // (s2 == 1, n2 even, 16-B aligned rows: two float2 as one float4)
      typedef float f4 __attribute__((ext_vector_type(4)));
      typedef float f2v __attribute__((ext_vector_type(2)));
      f4 x = __builtin_nontemporal_load(reinterpret_cast<const f4 *>(in + o));
      if constexpr (CPLX) {
        const f4 h = __builtin_nontemporal_load(reinterpret_cast<const f4 *>(reinterpret_cast<const V2 *>(filter) + o));
        x = f4{x.x * h.x - x.y * h.y, x.x * h.y + x.y * h.x, x.z * h.z - x.w * h.w, x.z * h.w + x.w * h.z};
      } else {
        const f2v h = __builtin_nontemporal_load(reinterpret_cast<const f2v *>(reinterpret_cast<const T *>(filter) + o));
        x = f4{x.x * h.x, x.y * h.x, x.z * h.y, x.w * h.y};
      }
      __builtin_nontemporal_store(x, reinterpret_cast<f4 *>(out + o));
    } else {
      V2 x = gload(in + o);
      if constexpr (CPLX) {
        const V2 h = gload(reinterpret_cast<const V2 *>(filter) + o);
        const T re = x.x * h.x - x.y * h.y, im = x.x * h.y + x.y * h.x;
        x.x = re; x.y = im;
      } else {
        const T h = __builtin_nontemporal_load(reinterpret_cast<const T *>(filter) + o);
        x.x *= h; x.y *= h;
      }
      gstore(out + o, x);
    }
  }
}

// pointwise multiply of a spectrum block by a filter at the same element index (offt_hipk_pointwise): rows along the
// smallest stride, 16 B per lane (two single-precision elements when that stride is 1), non-temporal both ways --
// every byte is touched once
template <typename T, bool CPLX, int EPL>
__global__ void __launch_bounds__(256)
pointwise_k(typename vec2<T>::type *data, const void *filter, int n1, int n2, long long s0, long long s1, long long s2, long long rows) {
  using V2 = typename vec2<T>::type;
  const int i2 = (blockIdx.x * 256 + threadIdx.x) * EPL;
  if (i2 >= n2) return;
  for (long long r = blockIdx.y; r < rows; r += gridDim.y) {
    const long long i1 = r % n1, i0 = r / n1;
    const long long o = i0 * s0 + i1 * s1 + (long long)i2 * s2;
    if constexpr (EPL == 2) {  // (s2 == 1, n2 even, 16-B aligned rows: two float2 as one float4)
      typedef float f4 __attribute__((ext_vector_type(4)));
      typedef float f2v __attribute__((ext_vector_type(2)));
      f4 x = __builtin_nontemporal_load(reinterpret_cast<const f4 *>(data + o));
      if constexpr (CPLX) {
        const f4 h = __builtin_nontemporal_load(reinterpret_cast<const f4 *>(reinterpret_cast<const V2 *>(filter) + o));
        x = f4{x.x * h.x - x.y * h.y, x.x * h.y + x.y * h.x, x.z * h.z - x.w * h.w, x.z * h.w + x.w * h.z};
      } else {
        const f2v h = __builtin_nontemporal_load(reinterpret_cast<const f2v *>(reinterpret_cast<const T *>(filter) + o));
        x = f4{x.x * h.x, x.y * h.x, x.z * h.y, x.w * h.y};
      }
      __builtin_nontemporal_store(x, reinterpret_cast<f4 *>(data + o));
    } else {
      V2 x = gload(data + o);
      if constexpr (CPLX) {
        const V2 h = gload(reinterpret_cast<const V2 *>(filter) + o);
        const T re = x.x * h.x - x.y * h.y, im = x.x * h.y + x.y * h.x;
        x.x = re; x.y = im;
      } else {
        const T h = __builtin_nontemporal_load(reinterpret_cast<const T *>(filter) + o);
        x.x *= h; x.y *= h;
      }
      gstore(data + o, x);
    }
  }
}

// out = sum_k in_k * H_k over a strided box (offt_hipk_pointwise_sum): ONE sweep, 16 B per lane, non-temporal, the terms added
// in the order k = 0 ... nin-1.  A lane has loaded its element from every input before its only store, and no other lane
// touches that element: out may be one of the inputs.  The pointers travel by value and are read through compares on
// compile-time indices (sum_pick, offt_panel.hpp); k is uniform.
template <typename T, bool CPLX, int EPL>
__global__ void __launch_bounds__(256)
pointwise_sum_k(SumArgs sa, typename vec2<T>::type *out, int n1, int n2, long long s0, long long s1, long long s2, long long rows) {
  using V2 = typename vec2<T>::type;
  const int i2 = (blockIdx.x * 256 + threadIdx.x) * EPL;
  if (i2 >= n2) return;
  for (long long r = blockIdx.y; r < rows; r += gridDim.y) {
    const long long i1 = r % n1, i0 = r / n1;
    const long long o = i0 * s0 + i1 * s1 + (long long)i2 * s2;
    if constexpr (EPL == 2) {  // (s2 == 1, n2 even, 16-B aligned rows: two float2 as one float4)
      typedef float f4 __attribute__((ext_vector_type(4)));
      typedef float f2v __attribute__((ext_vector_type(2)));
      f4 acc = f4{0.f, 0.f, 0.f, 0.f};
      for (int k = 0; k < sa.nin; k++) {
        const V2 *in = reinterpret_cast<const V2 *>(sum_pick(sa.src, k));
        const void *filter = sum_pick(sa.filter, k);
        const f4 x = __builtin_nontemporal_load(reinterpret_cast<const f4 *>(in + o));
        if constexpr (CPLX) {
          const f4 h = __builtin_nontemporal_load(reinterpret_cast<const f4 *>(reinterpret_cast<const V2 *>(filter) + o));
          acc += f4{x.x * h.x - x.y * h.y, x.x * h.y + x.y * h.x, x.z * h.z - x.w * h.w, x.z * h.w + x.w * h.z};
        } else {
          const f2v h = __builtin_nontemporal_load(reinterpret_cast<const f2v *>(reinterpret_cast<const T *>(filter) + o));
          acc += f4{x.x * h.x, x.y * h.x, x.z * h.y, x.w * h.y};
        }
      }
      __builtin_nontemporal_store(acc, reinterpret_cast<f4 *>(out + o));
    } else {
      V2 acc;
      acc.x = 0; acc.y = 0;
      for (int k = 0; k < sa.nin; k++) {
        const V2 *in = reinterpret_cast<const V2 *>(sum_pick(sa.src, k));
        const void *filter = sum_pick(sa.filter, k);
        const V2 x = gload(in + o);
        if constexpr (CPLX) {
          const V2 h = gload(reinterpret_cast<const V2 *>(filter) + o);
          acc.x += x.x * h.x - x.y * h.y; acc.y += x.x * h.y + x.y * h.x;
        } else {
          const T h = __builtin_nontemporal_load(reinterpret_cast<const T *>(filter) + o);
          acc.x += x.x * h; acc.y += x.y * h;
        }
      }
      gstore(out + o, acc);
    }
  }
}

// out = x * y over a strided box (offt_hipk_pointwise_prod): ONE sweep, non-temporal.  A lane works on W scalars that are
// contiguous in memory -- EPL complex elements (REAL = false: W = 2 EPL, a complex product per pair) or W real scalars of
// an r2c plan's rows (REAL = true: offsets and extents count scalars) -- 16 B where the rows allow.  It has loaded both
// operands before its only store and no other lane touches its scalars: out may be either operand.  y == x (uniform):
// the square from one load.
template <typename T, int W>
struct prod_vec { typedef T type __attribute__((ext_vector_type(W))); };
template <typename T>
struct prod_vec<T, 1> { typedef T type; };
template <typename T, bool REAL, int W>
__global__ void __launch_bounds__(256)
pointwise_prod_k(const T *x, const T *y, T *out, int n1, int n2, long long s0, long long s1, long long s2, long long rows) {
  using VT = typename prod_vec<T, W>::type;
  constexpr int U = REAL ? 1 : 2;    // scalars per element
  constexpr int EPL = W / U;         // elements per lane
  static_assert(W % U == 0 && EPL >= 1, "whole elements per lane");
  const int i2 = (blockIdx.x * 256 + threadIdx.x) * EPL;
  if (i2 >= n2) return;
  const bool square = y == x;
  for (long long r = blockIdx.y; r < rows; r += gridDim.y) {
    const long long i1 = r % n1, i0 = r / n1;
    const long long o = (i0 * s0 + i1 * s1 + (long long)i2 * s2) * U;
    const VT a = __builtin_nontemporal_load(reinterpret_cast<const VT *>(x + o));
    const VT b = square ? a : __builtin_nontemporal_load(reinterpret_cast<const VT *>(y + o));
    VT p;
    if constexpr (REAL) p = a * b;
    else if constexpr (W == 2) p = VT{a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x};
    else p = VT{a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x, a.z * b.z - a.w * b.w, a.z * b.w + a.w * b.z};
    __builtin_nontemporal_store(p, reinterpret_cast<VT *>(out + o));
  }
}

// ---------------------------------------------------------------------------
// shell-binned power / cross spectrum of a strided box (offt_hipk_spectrum_shells): a read-only sweep that ends in a keyed
// reduction, every floating-point addition in an order fixed by the geometry alone.
// ---------------------------------------------------------------------------
// the box after the stride sort (axis 2 = smallest stride), each axis with what its wavenumber needs
struct ShellArgs {
  int n[3];          // extents
  long long st[3];   // strides in elements
  int g0[3];         // global index of local index 0
  int N[3];          // global length of the axis (the FULL Nz on the halved axis of an r2c plan)
  int km[3];         // integer multiplier of the axis' wavenumber
  int zaxis;         // the halved axis of an r2c plan (weights 2 / 1), -1: complex plan
  int Nz;            // ... and its full length N[zaxis]
  int nb;            // bins kept: min(nbins, largest shell of the grid + 1)
  int n2l;           // lane slots per row: n[2] / EPL
  int step[3];       // the slots between two chunks of one wave, as (axis-0 rows, axis-1 rows, slots of a row)
  int with_counts;
};

// nearest integer to sqrt(k2): the s with (2s-1)^2 <= 4 k2 < (2s+1)^2.  k2 is clamped first (every shell the table can hold
// is far below the clamp, and the shell is monotone in k2), so that the decision runs in 32-bit integers.  The hardware
// square root is the first guess only: at c <= 2^27 it is off by less than 0.01 (float(c) and v_sqrt_f32 are each good to
// 2^-23 relative, sqrt(c) < 11586), so the guess is at most one off and one step either way settles it.
__device__ __forceinline__ int shell_of(unsigned long long k2) {
  const unsigned c = k2 < (1ull << 27) ? (unsigned)k2 : (1u << 27);
  const unsigned four = 4u * c;
  unsigned s = (unsigned)(__builtin_amdgcn_sqrtf((float)c) + 0.5f);
  s += (2u * s + 1u) * (2u * s + 1u) <= four ? 1u : 0u;
  s -= s > 0u && (2u * s - 1u) * (2u * s - 1u) > four ? 1u : 0u;
  return (int)s;
}

// lane i reads lane i + D of its row of 16 lanes (zero past the row's end): DPP row_shl, no LDS traffic
template <int D>
__device__ __forceinline__ double row_above(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), 0x100 + D, 0xf, 0xf, true);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), 0x100 + D, 0xf, 0xf, true);
  return __hiloint2double(hi, lo);
}

// One wave, one element per lane (consecutive lanes = consecutive elements of the sweep): add `term` into tab[key], lanes
// with key < 0 into nothing.  Lanes of equal key that follow one another form a run.  Inside each row of 16 lanes a run is
// summed towards its first lane by a doubling scan of DPP moves; the piece of a run that starts a row of 16 is then handed to
// the run's head in the rows below, rows 3, 2, 1 in that order.  The run heads update the table with a plain
// read-modify-write.  Two heads of one wave can hold the same key only in different monotone segments `seg` of the sweep
// (|k| along a row rises up to the fold and falls after it), so the heads go segment by segment, in lane order, and the
// slots of one round are distinct.  Every addition has its place fixed by the keys alone.
__device__ __forceinline__ void shells_add(double *tab, int lane, int key, int seg, double term) {
  const int prev = __builtin_amdgcn_update_dpp(key, key, 0x138, 0xf, 0xf, false);   // wave_shr:1: the key of lane - 1
  const bool head = lane == 0 || prev != key;
  const unsigned long long heads = __ballot(head);
  // the last lane of this lane's piece: before the next head, and inside the row of 16
  const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);
  int last = above ? lane + __ffsll((long long)above) - 1 : 63;
  last = last < (lane | 15) ? last : (lane | 15);
  double v = key >= 0 ? term : 0.0;
  { const double o = row_above<1>(v); if (lane + 1 <= last) v += o; }
  { const double o = row_above<2>(v); if (lane + 2 <= last) v += o; }
  { const double o = row_above<4>(v); if (lane + 4 <= last) v += o; }
  { const double o = row_above<8>(v); if (lane + 8 <= last) v += o; }
#pragma unroll
  for (int r = 3; r >= 1; r--) {
    if ((heads >> (16 * r)) & 1ull) continue;   // (uniform) a run starts there: nothing to hand down
    const int h = 63 - __clzll((long long)(heads & ((1ull << (16 * r)) - 1ull)));   // the head of the run that goes on into row r
    const double o = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), 16 * r), __builtin_amdgcn_readlane(__double2loint(v), 16 * r));
    if (lane == h) v += o;
  }
  const bool hk = head && key >= 0;
  unsigned long long pend = __ballot(hk);
  while (pend) {
    const int sg = __builtin_amdgcn_readlane(seg, __ffsll((long long)pend) - 1);
    const bool mine = hk && seg == sg;
    if (mine) tab[key] += v;
    pend &= ~__ballot(mine);
  }
}

// the sweep: every wave walks chunks of 64 lane slots (EPL elements each, 16 B per lane, non-temporal) of the rows in
// storage order, the next chunk's load in flight while this one is binned.  LDS: one table of nb doubles per wave, one table
// of nb integer counts per workgroup.  At the end the waves' tables are added in wave order and stored, with the counts, as
// this workgroup's line of the partials.
template <typename T, bool CROSS, int EPL>
__global__ void __launch_bounds__(256)
shells_sweep_k(ShellArgs sa, const typename vec2<T>::type *a, const typename vec2<T>::type *b, double *psum, unsigned *pcnt) {
  using V2 = typename vec2<T>::type;
  typedef T vt __attribute__((ext_vector_type(2 * EPL)));
  extern __shared__ double shells_lds[];
  const int nb = sa.nb, waves = blockDim.x >> 6, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double *tab = shells_lds + (size_t)wave * nb;
  unsigned *cnt = reinterpret_cast<unsigned *>(shells_lds + (size_t)waves * nb);
  for (int i = threadIdx.x; i < waves * nb; i += blockDim.x) shells_lds[i] = 0.0;
  for (int i = threadIdx.x; i < nb; i += blockDim.x) cnt[i] = 0u;
  __syncthreads();

  const long long slot = ((long long)blockIdx.x * waves + wave) * 64 + lane;
  const long long row = slot / sa.n2l;
  int i2 = (int)(slot % sa.n2l), i1 = (int)(row % sa.n[1]);
  long long i0 = row / sa.n[1];
  auto load = [&](const V2 *p, bool live, long long o) {
    vt x = {};
    if (live) x = __builtin_nontemporal_load(reinterpret_cast<const vt *>(p + o));
    return x;
  };
  bool live = i0 < sa.n[0];
  long long o = i0 * sa.st[0] + i1 * sa.st[1] + (long long)i2 * EPL * sa.st[2];
  vt xa = load(a, live, o), xb = {};
  if constexpr (CROSS) xb = load(b, live, o);
  while (__builtin_amdgcn_readfirstlane((int)(i0 < sa.n[0]))) {   // lane 0 holds the wave's first slot
    // this lane's slot of the wave's next chunk, and its load
    int j2 = i2 + sa.step[2], j1 = i1 + sa.step[1];
    long long j0 = i0 + sa.step[0];
    if (j2 >= sa.n2l) { j2 -= sa.n2l; ++j1; }
    if (j1 >= sa.n[1]) { j1 -= sa.n[1]; ++j0; }
    const bool nlive = j0 < sa.n[0];
    const long long no = j0 * sa.st[0] + j1 * sa.st[1] + (long long)j2 * EPL * sa.st[2];
    const vt na = load(a, nlive, no);
    vt nbv = {};
    if constexpr (CROSS) nbv = load(b, nlive, no);

    // wavenumbers of the row, then per element the shell, the weight and the term
    const int ga = (int)i0 + sa.g0[0], gb = i1 + sa.g0[1];
    // (|multiplier . wavenumber| <= 2^30 by the launcher's check: squares of 32-bit magnitudes)
    const unsigned qa = (unsigned)abs(sa.km[0] * (2 * ga <= sa.N[0] ? ga : ga - sa.N[0]));
    const unsigned qb = (unsigned)abs(sa.km[1] * (2 * gb <= sa.N[1] ? gb : gb - sa.N[1]));
    const unsigned long long k01 = (unsigned long long)qa * qa + (unsigned long long)qb * qb;
    const int rowid = (int)i0 * sa.n[1] + i1;
    const int row0 = __builtin_amdgcn_readfirstlane(rowid);
#pragma unroll
    for (int e = 0; e < EPL; e++) {
      const int gc = i2 * EPL + e + sa.g0[2];
      const unsigned qc = (unsigned)abs(sa.km[2] * (2 * gc <= sa.N[2] ? gc : gc - sa.N[2]));
      const int s = shell_of(k01 + (unsigned long long)qc * qc);
      const int key = live && s < nb ? s : -1;
      const int gz = sa.zaxis == 0 ? ga : sa.zaxis == 1 ? gb : gc;
      const int w = sa.zaxis >= 0 && gz > 0 && 2 * gz != sa.Nz ? 2 : 1;
      const double ar = (double)xa[2 * e], ai = (double)xa[2 * e + 1];
      double term;
      if constexpr (CROSS) term = ar * (double)xb[2 * e] + ai * (double)xb[2 * e + 1];
      else term = ar * ar + ai * ai;
      if (sa.with_counts && key >= 0) atomicAdd(&cnt[key], (unsigned)w);
      shells_add(tab, lane, key, 2 * (rowid - row0) + (2 * gc > sa.N[2] ? 1 : 0), (double)w * term);
    }
    i0 = j0; i1 = j1; i2 = j2; live = nlive; xa = na;
    if constexpr (CROSS) xb = nbv;
  }
  __syncthreads();
  for (int s = threadIdx.x; s < nb; s += blockDim.x) {
    double acc = 0.0;
    for (int w = 0; w < waves; w++) acc += shells_lds[(size_t)w * nb + s];
    psum[(size_t)blockIdx.x * nb + s] = acc;
    pcnt[(size_t)blockIdx.x * nb + s] = cnt[s];
  }
}

// the partials of nwg workgroups added in workgroup order: a workgroup owns 8 bins, each of its 32 thread groups adds a
// contiguous range of the workgroups, and the 32 sub-sums are added in group order.  Bins nb ... nbins-1 hold no mode.
#define SHELLS_COMBINE_GROUPS 32
__global__ void __launch_bounds__(256)
shells_combine_k(const double *psum, const unsigned *pcnt, int nwg, int nb, int nbins, double *sums, long long *counts) {
  __shared__ double ssum[SHELLS_COMBINE_GROUPS][8];
  __shared__ long long scnt[SHELLS_COMBINE_GROUPS][8];
  const int bin = threadIdx.x & 7, grp = threadIdx.x >> 3, s = blockIdx.x * 8 + bin;
  const int per = (nwg + SHELLS_COMBINE_GROUPS - 1) / SHELLS_COMBINE_GROUPS;
  const int g0 = grp * per, g1 = g0 + per < nwg ? g0 + per : nwg;
  double acc = 0.0;
  long long c = 0;
  if (s < nb)
    for (int g = g0; g < g1; g++) { acc += psum[(size_t)g * nb + s]; c += pcnt[(size_t)g * nb + s]; }
  ssum[grp][bin] = acc; scnt[grp][bin] = c;
  __syncthreads();
  if (grp == 0 && s < nbins) {
    acc = 0.0; c = 0;
    for (int g = 0; g < SHELLS_COMBINE_GROUPS; g++) { acc += ssum[g][bin]; c += scnt[g][bin]; }
    sums[s] = acc;
    if (counts) counts[s] = c;
  }
}

// zero a strided 3-D block outside the kept sub-box [0,k0) x [0,k1) x [0,k2) (offt_hipk_zero_outside): rows along i2, one
// workgroup row per (i0, i1).  W = scalars of type S per 16-B store; VEC: the rows are unit-stride and 16-B aligned, a lane
// clears 16 B at W-scalar boundaries (the first store of a row that starts inside the kept part is split into scalars)
template <typename S, int SPE, bool VEC>
__global__ void __launch_bounds__(256)
zero_outside_k(S *buf, int n1, int n2, int k0, int k1, int k2, long long s0, long long s1, long long s2, long long rows) {
  constexpr int W = VEC ? 16 / (int)sizeof(S) : SPE;  // scalars per lane
  typedef S vt __attribute__((ext_vector_type(W)));
  // extents, strides and the kept length along i2 count elements of SPE scalars
  const long long len = (long long)n2 * SPE, keep = (long long)k2 * SPE;
  for (long long r = blockIdx.y; r < rows; r += gridDim.y) {
    const long long i1 = r % n1, i0 = r / n1;
    const bool inside = i0 < k0 && i1 < k1;   // rows of the kept slab: only their tail [k2, n2) goes
    const long long from = inside ? keep : 0;
    S *row = buf + (i0 * s0 + i1 * s1) * SPE;
    if constexpr (VEC) {
      const long long a = ((long long)blockIdx.x * 256 + threadIdx.x) * W;
      if (a + W <= from || a >= len) continue;
      if (a >= from && a + W <= len) {
        vt z = {};
        __builtin_nontemporal_store(z, reinterpret_cast<vt *>(row + a));
      } else {
        for (long long i = a < from ? from : a; i < a + W && i < len; ++i) row[i] = (S)0;
      }
    } else {
      const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
      if (e * SPE < from || e >= n2) continue;
      for (int q = 0; q < SPE; ++q) row[e * s2 * SPE + q] = (S)0;
    }
  }
}

__device__ __forceinline__ double hash_val(int x, int y, int z, int c) {
  unsigned h = (unsigned)x * 73856093u ^ (unsigned)y * 19349663u ^ (unsigned)z * 83492791u ^
               (unsigned)c * 2654435761u;
  h ^= h >> 13; h *= 0x5bd1e995u; h ^= h >> 15;
  return (double)(h & 0xffffffu) / 8388608.0 - 1.0;
}

template <typename V2>
__global__ void __launch_bounds__(256)
fill_k(V2 *buf, int kind, int n0, int n1, int n2, int s0, int s1, int s2,
       long long st0, long long st1, long long st2) {
  long long total = (long long)n0 * n1 * n2;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    int i2 = (int)(i % n2);
    long long r = i / n2;
    int i1 = (int)(r % n1);
    int i0 = (int)(r / n1);
    V2 v;
    if (kind == 0) {  // run-fft.c:56-57 ramp
      v.x = (decltype(v.x))((i2 + s2) + 10 * (i1 + s1) + 100 * (i0 + s0));
      v.y = 0;
    } else {
      v.x = (decltype(v.x))hash_val(i0 + s0, i1 + s1, i2 + s2, 0);
      v.y = (decltype(v.y))hash_val(i0 + s0, i1 + s1, i2 + s2, 1);
    }
    buf[i0 * st0 + i1 * st1 + i2 * st2] = v;
  }
}

template <typename T>
__global__ void __launch_bounds__(256)
fill_real_k(T *buf, int kind, int n0, int n1, int n2, int s0, int s1, int s2, long long st0, long long st1, long long st2) {
  long long total = (long long)n0 * n1 * n2;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    int i2 = (int)(i % n2);
    long long r = i / n2;
    int i1 = (int)(r % n1), i0 = (int)(r / n1);
    buf[i0 * st0 + i1 * st1 + i2 * st2] = kind == 0 ? (T)((i2 + s2) + 10 * (i1 + s1) + 100 * (i0 + s0))
                                                    : (T)hash_val(i0 + s0, i1 + s1, i2 + s2, 0);
  }
}

// ---------------------------------------------------------------------------
// host side: kernel registry lookup, twiddle tables, launchers
// ---------------------------------------------------------------------------
// Environment switches of the launcher, read once at first use.  A switch that is "on" by default is on when unset or
// non-zero (atoi); the hipRTC library path (OFFT_HIPRTC_LIB) stays with its loader, rtc_load().
struct Env {
  static int num(const char *name, int dflt) { const char *s = getenv(name); return s ? atoi(s) : dflt; }
  static int positive(const char *name, int dflt) { const int v = num(name, dflt); return v > 0 ? v : dflt; }
  const bool rtc = num("OFFT_RTC", 1) != 0;                              // plan-time kernels through hipRTC
  const int rtc_shapes = num("OFFT_RTC_SHAPES", 1);                      // shapes compiled per plan-time length (static sweep: up to 8)
  const bool bluestein = num("OFFT_BLUESTEIN", 1) != 0;                  // Bluestein panel kernel, and the Bluestein lines through scratch
  const int xcd_remap = num("OFFT_XCD_REMAP", 32);                       // XCD-aware panel order: 0 off, a power of two = run length G
  const bool f32_pairs = num("OFFT_F32_PAIRS", 1) != 0;                  // single-precision column-pair kernels
  const bool keep_stores = num("OFFT_KEEP_STORES", 1) != 0;              // cache-keeping twins for out_keep descriptors
  const bool fourstep = num("OFFT_FOURSTEP", 1) != 0;                    // four-step decomposition
  const int fourstep_n1 = num("OFFT_FOURSTEP_N1", 0);                    // force the first factor of a four-step split (sweeps)
  const int fourstep_chunk_mib = positive("OFFT_FOURSTEP_CHUNK_MIB", 192);  // scratch per four-step chunk
  const bool fourstep_fuse = num("OFFT_FOURSTEP_FUSE", 1) != 0;          // four-step twiddles on the first sub-pass's stores
  const bool bluestein_long = num("OFFT_BLUESTEIN_LONG", 1) != 0;        // Bluestein lines through scratch for lengths without a split
  const bool bluestein_long_pow2 = num("OFFT_BLUESTEIN_LONG_POW2", 0) != 0;  // ... on M = 2^k only, not the shortest (64 | 32) x L
  const bool r2c_bluestein = num("OFFT_R2C_BLUESTEIN", 1) != 0;          // real lines of a Bluestein length through scratch (0: any-length kernel)
  const int mix_threads = num("OFFT_MIX_THREADS", 0);                    // workgroup size of the any-length kernel (64 .. 1024), 0 = by LDS footprint
  const int pair_run = num("OFFT_PAIR_RUN", 0);                           // fft_pair_yx_k: blocks per run of one role (a power of two >= 8), 0 = one period of the XCD order
};
const Env &env() { static const Env e; return e; }

// LDS of a CU: what the any-length kernel can use, and the budget of the plan-time panel shapes
constexpr size_t LDS_BYTES = 160 * 1024;

std::once_flag g_reg_once;
void build_registry() {
  registry().reserve(8192);  // plan-time instances are appended later: no reallocation under a concurrent lookup
#ifdef OFFT_DEV_REGISTRY  /* the static-sweep tool (tools/sweep_mixed.py) builds the library with ONLY its candidate kernels, in a reg_dev.hip it generates */
  reg_dev();
#else
  reg_pow2_f64();
  reg_pow2_f64_1024();
  reg_pow2_f64_anysplit();
  reg_pair_yx_f64();
  reg_pow2_f32();
  reg_pow2_f32_big();
  reg_pow2_f32_anysplit();
  reg_pow2_f32_pair();
  reg_pow2_tw4();
  reg_mixed_f64_a();
  reg_mixed_f64_b();
  reg_mixed_f64_c();
  reg_mixed_f64_d();
  reg_mixed_f64_e();
  reg_mixed_f32_a();
  reg_mixed_f32_b();
  reg_conv_f64();
  reg_conv_f32();
  reg_conv_oop_f64();
  reg_conv_oop_f32();
  reg_conv_mixed_f64();
  reg_conv_mixed_f32();
  reg_conv_oop_mixed_f64();
  reg_conv_oop_mixed_f32();
  reg_conv_sum_mixed_f64();
  reg_conv_sum_mixed_f32();
  reg_conv_sum_f64();
  reg_conv_sum_f32();
  reg_spec_f64();
  reg_spec_f32();
  reg_spec_mixed_f64();
  reg_spec_mixed_f32();
  reg_half_f64();
  reg_half_f32();
  reg_half_real_f64();
  reg_half_real_f32();
  reg_half_mixed_f64();
  reg_half_mixed_f32();
  reg_half_real_mixed_f64();
  reg_half_real_mixed_f32();
  reg_prod_f64();
  reg_prod_f32();
  reg_prod_real_f64();
  reg_prod_real_f32();
  reg_bluestein_all();
#endif
}

// VariantKey -> registry entries, rebuilt when the registry has grown (plan-time instances): a launch must not scan
// several hundred variants
std::mutex g_idx_mu;
std::unordered_map<VariantKey, std::vector<int>, VariantKeyHash> g_idx;
size_t g_idx_size = 0;

// the entry of `key` with this id, else the key's default, else nullptr.  The key is compared whole: what comes back IS
// that kernel, and a caller checks only what is not part of the key (id, is_default, mixed)
Variant *find_variant(const VariantKey &key, int id = -1) {
  std::call_once(g_reg_once, build_registry);
  std::lock_guard<std::mutex> lk(g_idx_mu);
  auto &reg = registry();
  if (g_idx_size != reg.size()) {
    g_idx.clear();
    for (size_t i = 0; i < reg.size(); ++i) g_idx[reg[i].key].push_back((int)i);
    g_idx_size = reg.size();
  }
  auto it = g_idx.find(key);
  if (it == g_idx.end()) return nullptr;
  Variant *def = nullptr;
  for (int i : it->second) {
    Variant &v = reg[i];
    if (v.id == id) return &v;
    if (v.is_default) def = &v;
  }
  return def;
}
// the keys most lookups ask for: the plain full-line kernel of a flavour, and the four-step twin of a short first factor
VariantKey plain_key(int n, int prec, bool inc, bool outc) { return VariantKey{n, prec, inc, outc, Role::Plain, false, 0}; }
Variant *find_tw4(int n, int prec) { return find_variant(VariantKey{n, prec, false, false, Role::TW4, false, 0}); }

// ---------------------------------------------------------------------------
// Plan-time specialisation.  A length without a precompiled panel kernel whose prime factors are <= 31 gets
// its own fft_panelx_k instances at offt_hipk_prepare(): the device part of offt_panel.hpp travels inside
// the library as a string, a shape (radix order, threads per line, panel width) is picked with the scoring of
// tools/sweep_mixed.py, hipRTC compiles the four (in_contig, out_contig) flavours and the two real-input ones (2-4 s in all) and the
// code object is loaded as a module.  The two real-output flavours (the c2r inverse's z pass) are a module of their own,
// compiled only for the z length of a real-input plan (offt_hipk_prepare with OFFT_HIPK_PREP_C2R): complex plans do not
// wait for them.  OFFT_RTC=0 turns it off; any failure leaves the any-length kernel in
// charge and says why on stderr once.
// ---------------------------------------------------------------------------
struct RtcApi {
  void *h = nullptr;
  hiprtcResult (*CreateProgram)(hiprtcProgram *, const char *, const char *, int, const char **, const char **) = nullptr;
  hiprtcResult (*AddNameExpression)(hiprtcProgram, const char *) = nullptr;
  hiprtcResult (*CompileProgram)(hiprtcProgram, int, const char **) = nullptr;
  hiprtcResult (*GetProgramLogSize)(hiprtcProgram, size_t *) = nullptr;
  hiprtcResult (*GetProgramLog)(hiprtcProgram, char *) = nullptr;
  hiprtcResult (*GetLoweredName)(hiprtcProgram, const char *, const char **) = nullptr;
  hiprtcResult (*GetCodeSize)(hiprtcProgram, size_t *) = nullptr;
  hiprtcResult (*GetCode)(hiprtcProgram, char *) = nullptr;
  hiprtcResult (*DestroyProgram)(hiprtcProgram *) = nullptr;
};
RtcApi g_rtc;
std::mutex g_rtc_mu;
int g_rtc_state = 0;  // 0 untried, 1 ready, -1 unavailable

bool rtc_load() {
  if (g_rtc_state) return g_rtc_state > 0;
  g_rtc_state = -1;
  // the hipRTC that belongs to the HIP runtime this process already uses (PyTorch bundles both), else the system one
  std::vector<std::string> cand;
  Dl_info di;
  if (dladdr((void *)&hipModuleLoadData, &di) && di.dli_fname) {
    std::string dir(di.dli_fname);
    const size_t sl = dir.rfind('/');
    if (sl != std::string::npos) cand.push_back(dir.substr(0, sl + 1) + "libhiprtc.so");
  }
  if (const char *lib = getenv("OFFT_HIPRTC_LIB")) cand.insert(cand.begin(), lib);
  cand.push_back("libhiprtc.so");
  cand.push_back("/opt/rocm/lib/libhiprtc.so");
  for (auto &c : cand) {
    g_rtc.h = dlopen(c.c_str(), RTLD_NOW | RTLD_LOCAL);
    if (g_rtc.h) break;
  }
  if (!g_rtc.h) return false;
#define RTC_SYM(name) \
  g_rtc.name = (decltype(g_rtc.name))dlsym(g_rtc.h, "hiprtc" #name); \
  if (!g_rtc.name) return false;
  RTC_SYM(CreateProgram) RTC_SYM(AddNameExpression) RTC_SYM(CompileProgram) RTC_SYM(GetProgramLogSize) RTC_SYM(GetProgramLog)
  RTC_SYM(GetLoweredName) RTC_SYM(GetCodeSize) RTC_SYM(GetCode) RTC_SYM(DestroyProgram)
#undef RTC_SYM
  g_rtc_state = 1;
  return true;
}

struct Shape { int tpl, r0, r1, r2, cols; double score; int emax; size_t lds; };

// lengths the panel kernels can factor into register radices <= 32: every prime factor <= 31
bool smooth13(int n) {
  for (int p : {2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31}) while (n % p == 0) n /= p;
  return n == 1;
}
int cdiv_i(int a, int b) { return (a + b - 1) / b; }

// the candidate scoring of tools/sweep_mixed.py (live butterfly slots, waves per CU, panel width, radix size)
bool choose_shapes(int N, int prec, int want, std::vector<Shape> *out) {
  const int esz = prec == OFFT_PREC_F64 ? 8 : 4, emax_cap = 32, emax_soft = prec == OFFT_PREC_F64 ? 24 : 32;
  std::vector<int> rad;
  for (int r = 2; r <= 32; ++r) if (smooth13(r)) rad.push_back(r);
  std::vector<Shape> all;
  auto consider = [&](int r0, int r1, int r2) {
    const int rs[3] = {r0, r1, r2};
    const int nst = r2 > 1 ? 3 : (r1 > 1 ? 2 : 1);
    for (int cols : {8, 16, 4}) {
      for (int tpl = 1; tpl <= 256; ++tpl) {
        const int nt = tpl * cols;
        if (nt > 1024 || nt < 64) continue;
        int emax = 0; double eff = 0;
        for (int s = 0; s < nst; ++s) {
          const int nb = cdiv_i(N / rs[s], tpl);
          emax = nb * rs[s] > emax ? nb * rs[s] : emax;
          eff += (double)N / ((double)tpl * nb * rs[s]);
        }
        eff /= nst;
        if ((nt % 64) && !(eff == 1.0 && nt % 16 == 0)) continue;
        const bool swz = r0 % 16 == 0 && N % 16 == 0;
        const int paddiv = (r0 % 2 == 0 && !swz) ? r0 : 0;
        const int npad = paddiv ? N + N / paddiv : N;
        const int lstride = (npad + 31) / 32 * 32 + 4;
        const size_t ex = nst > 1 ? (size_t)cols * lstride * esz : 0;
        const size_t qt = N % 4 == 0 ? N / 4 + 1 : N;
        const size_t lds = nst > 1 ? (ex + 15) / 16 * 16 + qt * 2 * esz : 0;
        if (emax > emax_cap || emax < 6 || lds > LDS_BYTES || eff < 0.74) continue;
        size_t wg = lds ? LDS_BYTES / lds : 4;
        wg = wg < 1 ? 1 : (wg > 4 ? 4 : wg);
        const int waves = (int)wg * cdiv_i(nt, 64);
        if (waves < 4) continue;
        double sc = eff * std::sqrt(waves >= 8 ? 1.0 : waves / 8.0) * (cols * esz * 2 >= 128 ? 1.0 : 0.8);
        sc *= (emax >= 12 ? 1.0 : 0.85) * (nst > 2 ? 0.97 : 1.0) * (emax > emax_soft ? 0.8 : 1.0);  // > 24 f64 points per thread: 2 waves/SIMD
        const int rmax = r0 > r1 ? (r0 > r2 ? r0 : r2) : (r1 > r2 ? r1 : r2);
        sc *= rmax > 16 ? 0.92 : 1.0;
        sc *= (double)nt / (64.0 * cdiv_i(nt, 64));
        all.push_back(Shape{tpl, r0, r1, r2, cols, sc, emax, lds});
      }
    }
  };
  for (int r0 : rad) {
    if (N % r0) continue;
    const int m = N / r0;
    if (m == 1) consider(r0, 1, 1);
    for (int r1 : rad) {
      if (m % r1) continue;
      const int r2 = m / r1;
      if (r2 == 1) consider(r0, r1, 1);
      else if (r2 <= 32 && smooth13(r2)) consider(r0, r1, r2);
    }
  }
  std::stable_sort(all.begin(), all.end(), [](const Shape &a, const Shape &b) { return a.score > b.score; });
  // the best shape, then (for a plan-time sweep, OFFT_RTC_SHAPES > 1) the next ones that differ in radix set, thread count
  // or panel width
  auto key = [](const Shape &s) { int r[3] = {s.r0, s.r1, s.r2}; std::sort(r, r + 3); return r[0] * 10000 + r[1] * 100 + r[2]; };
  for (const Shape &c : all) {
    if ((int)out->size() >= want) break;
    bool dup = false;
    int same_set = 0;
    for (const Shape &o : *out) {
      if (key(o) == key(c)) {
        ++same_set;
        if (o.cols == c.cols && std::abs(o.tpl - c.tpl) < 16 && !(o.r0 != c.r0 && o.tpl == c.tpl)) dup = true;
      }
    }
    if (!dup && same_set < 2) out->push_back(c);
  }
  return !out->empty();
}

// compile and register fft_panelx_k<T, n, shape> for the four flavours; 0 on success.  c2r: the two real-output flavours
// of the default shape instead (the complex instances exist already)
int rtc_build(int n, int prec, bool c2r = false) {
  std::lock_guard<std::mutex> lk(g_rtc_mu);
  if (find_variant(VariantKey{n, prec, true, true, c2r ? Role::C2R : Role::Plain, false, 0})) return 0;  // somebody was faster
  static bool warned = false;
  auto fail = [&](const char *what, const std::string &detail) {
    if (!warned) fprintf(stderr, "offt(hip): no plan-time kernel for n=%d (%s%s%s); using the any-length kernel\n", n, what,
                         detail.empty() ? "" : ": ", detail.c_str());
    warned = true;
    return -1;
  };
  if (!rtc_load()) return fail("hipRTC library not found", "");
  const int nshapes = env().rtc_shapes;
  std::vector<Shape> shapes;
  if (!choose_shapes(n, prec, c2r || nshapes < 1 ? 1 : (nshapes > 8 ? 8 : nshapes), &shapes)) return fail("no panel shape fits", "");
  const char *T = prec == OFFT_PREC_F64 ? "double" : "float";
  std::string src;
  for (const char *p : k_rtc_source_pieces) src += p;
  hiprtcProgram prog;
  if (g_rtc.CreateProgram(&prog, src.c_str(), "offt_panel_rtc.hip", 0, nullptr, nullptr) != HIPRTC_SUCCESS)
    return fail("hiprtcCreateProgram failed", "");
  // four (in_contig, out_contig) flavours per shape, plus the two real-input z-pass flavours of the default shape; or (c2r)
  // the two real-output flavours of the default shape (the shape choice is deterministic: the same one as the complex instances')
  const bool flav[8][4] = {{true, true, false, false}, {false, false, false, false}, {true, false, false, false}, {false, true, false, false},
                           {true, true, true, false}, {true, false, true, false}, {true, true, false, true}, {false, true, false, true}};
  struct Inst { int shape, f; };
  std::vector<Inst> inst;
  std::vector<std::string> expr;
  for (size_t k = 0; k < shapes.size(); ++k)
    for (int f = c2r ? 6 : 0; f < (c2r ? 8 : k == 0 ? 6 : 4); ++f) {
      const Shape &sh = shapes[k];
      char b[256];
      if (flav[f][3])
        snprintf(b, sizeof b, "offtk::fft_c2r_panelx_k<%s, %d, %d, %d, %d, %d, %d, %s, true>", T, n, sh.tpl, sh.r0, sh.r1, sh.r2, sh.cols,
                 flav[f][0] ? "true" : "false");
      else
        snprintf(b, sizeof b, "offtk::fft_panelx_k<%s, %d, %d, %d, %d, %d, %d, %s, %s, true, %s>", T, n, sh.tpl, sh.r0, sh.r1, sh.r2,
                 sh.cols, flav[f][0] ? "true" : "false", flav[f][1] ? "true" : "false", flav[f][2] ? "true" : "false");
      expr.push_back(b);
      inst.push_back(Inst{(int)k, f});
      g_rtc.AddNameExpression(prog, expr.back().c_str());
    }
  const char *opts[] = {"--offload-arch=gfx950", "-O3", "-std=c++17"};
  if (g_rtc.CompileProgram(prog, 3, opts) != HIPRTC_SUCCESS) {
    size_t ls = 0;
    g_rtc.GetProgramLogSize(prog, &ls);
    std::string log(ls, '\0');
    if (ls) g_rtc.GetProgramLog(prog, &log[0]);
    g_rtc.DestroyProgram(&prog);
    return fail("hipRTC compile failed", log.substr(0, 600));
  }
  size_t cs = 0;
  g_rtc.GetCodeSize(prog, &cs);
  std::vector<char> code(cs);
  g_rtc.GetCode(prog, code.data());
  hipModule_t mod;
  if (hipModuleLoadData(&mod, code.data()) != hipSuccess) {
    (void)hipGetLastError();
    g_rtc.DestroyProgram(&prog);
    return fail("hipModuleLoadData failed", "");
  }
  std::vector<hipFunction_t> fn(expr.size());
  for (size_t e = 0; e < expr.size(); ++e) {
    const char *low = nullptr;
    if (g_rtc.GetLoweredName(prog, expr[e].c_str(), &low) != HIPRTC_SUCCESS || hipModuleGetFunction(&fn[e], mod, low) != hipSuccess) {
      (void)hipGetLastError();
      g_rtc.DestroyProgram(&prog);
      return fail("kernel symbol not found in the compiled module", "");
    }
  }
  g_rtc.DestroyProgram(&prog);
  // variant 0 = the best-scored shape = the default; the others are there for the static sweep (offt_hip_set_variant, -l N)
  std::lock_guard<std::mutex> lk_idx(g_idx_mu);  // lookups index the registry under this lock
  for (size_t e = 0; e < inst.size(); ++e) {
    const Shape &sh = shapes[inst[e].shape];
    const bool *fl = flav[inst[e].f];
    const Role role = fl[3] ? Role::C2R : fl[2] ? Role::R2C : Role::Plain;
    add_variant(VariantKey{n, prec, fl[0], fl[1], role, false, 0},
                VariantShape{sh.cols, sh.tpl * sh.cols, sh.emax, sh.lds, true, n % 4 != 0, sh.r0, sh.r1, sh.r2, sh.tpl, layout_name(true)}, nullptr,
                fl[3] ? "fft_c2r_panelx_k" : "fft_panelx_k", "", inst[e].shape, inst[e].shape == 0, (void *)fn[e]);
  }
  return 0;
}

struct Tables {
  void *quarter = nullptr;  // w^r, r = 0..N/4      (fast path)
  void *full = nullptr;     // w^m, m = 0..N-1      (generic path)
};
std::mutex g_tab_mu;
std::map<std::pair<int, int>, Tables> g_tabs;  // (n, prec) per current device is enough: one device per process

template <typename T>
int make_tables(int n, Tables &tb) {
  using V2 = typename vec2<T>::type;
  const long double pi = 3.14159265358979323846264338327950288419716939937510L;
  auto tw = [&](long long m) {
    // exact octant reduction, then cosl/sinl on [0, pi/4]
    long long mm = ((m % n) + n) % n;
    // angle = 2 pi mm / n ; reduce by octants using exact integer arithmetic on 8*mm/n
    long long oct = (8 * mm) / n;
    long long rem = 8 * mm - oct * n;  // angle = (oct + rem/n) * pi/4
    long double c, s;
    long double a = (long double)rem / (long double)n * (pi / 4);
    switch (oct & 7) {
      case 0: c = cosl(a); s = sinl(a); break;
      case 1: { long double b = pi / 4 - a; c = sinl(b); s = cosl(b); if (rem == 0) { c = s = sqrtl(0.5L); } break; }
      case 2: c = -sinl(a); s = cosl(a); break;
      case 3: { long double b = pi / 4 - a; c = -cosl(b); s = sinl(b); if (rem == 0) { c = -sqrtl(0.5L); s = sqrtl(0.5L); } break; }
      case 4: c = -cosl(a); s = -sinl(a); break;
      case 5: { long double b = pi / 4 - a; c = -sinl(b); s = -cosl(b); if (rem == 0) { c = s = -sqrtl(0.5L); } break; }
      case 6: c = sinl(a); s = -cosl(a); break;
      default: { long double b = pi / 4 - a; c = cosl(b); s = -sinl(b); if (rem == 0) { c = sqrtl(0.5L); s = -sqrtl(0.5L); } break; }
    }
    V2 w;
    w.x = (T)c;
    w.y = (T)(-s);  // forward: exp(-i theta)
    return w;
  };
  std::vector<V2> q(n / 4 + 1), f(n);
  for (int r = 0; r <= n / 4; ++r) q[r] = tw(r);
  for (int m = 0; m < n; ++m) f[m] = tw(m);
  HIPK_CHECK(hipMalloc(&tb.quarter, q.size() * sizeof(V2)));
  HIPK_CHECK(hipMemcpy(tb.quarter, q.data(), q.size() * sizeof(V2), hipMemcpyHostToDevice));
  HIPK_CHECK(hipMalloc(&tb.full, f.size() * sizeof(V2)));
  HIPK_CHECK(hipMemcpy(tb.full, f.data(), f.size() * sizeof(V2), hipMemcpyHostToDevice));
  return 0;
}

int get_tables(int n, int prec, Tables &out, bool create) {
  std::lock_guard<std::mutex> lk(g_tab_mu);
  auto key = std::make_pair(n, prec);
  auto it = g_tabs.find(key);
  if (it != g_tabs.end()) { out = it->second; return 0; }
  if (!create) {
    snprintf(g_err, sizeof g_err, "offt_hipk: no twiddle tables for n=%d (call offt_hipk_prepare at plan time)", n);
    return -1;
  }
  Tables tb;
  int rc = prec == OFFT_PREC_F64 ? make_tables<double>(n, tb) : make_tables<float>(n, tb);
  if (rc) return rc;
  g_tabs[key] = tb;
  out = tb;
  return 0;
}

bool is_pow2(int n) { return n > 0 && (n & (n - 1)) == 0; }

// ---------------------------------------------------------------------------
// Bluestein (offt_bluestein.hpp): per (n, precision) the chirp a[n] = exp(-i pi n^2 / n_len) and the spectrum
// B^ = FFT_M(b wrapped) / M, b[m] = exp(+i pi m^2 / n_len), M = the power of two >= 2 n_len - 1.
// ---------------------------------------------------------------------------
struct BlueTab { void *chirp = nullptr, *bhat = nullptr; int m = 0; };
std::mutex g_blue_mu;
std::map<std::pair<int, int>, BlueTab> g_blue;

int blue_m(int n) {
  int m = 256;
  while (m < 2 * n - 1) m <<= 1;
  return m;
}
BlueVariant *find_blue(int m, int prec, bool inc, bool outc) {
  std::call_once(g_reg_once, build_registry);
  for (auto &b : blue_registry())
    if (b.m == m && b.prec == prec && b.inc == inc && b.outc == outc) return &b;
  return nullptr;
}
bool blue_lookup(int n, int prec, BlueTab *out) {
  std::lock_guard<std::mutex> lk(g_blue_mu);
  auto it = g_blue.find(std::make_pair(n, prec));
  if (it == g_blue.end()) return false;
  *out = it->second;
  return true;
}

// ---- length facts: what a length can run on, as far as the registry and the switches say (no device state) ----
size_t elem_size(int prec) { return prec == OFFT_PREC_F64 ? sizeof(double2) : sizeof(float2); }
// two images of a line fit the LDS of the any-length kernel (5120 double / 10240 single points)
bool fits_any_length(int n, int prec) { return 2 * (size_t)n * elem_size(prec) <= LDS_BYTES; }
bool has_panel(int n, int prec) { return find_variant(plain_key(n, prec, true, true)) != nullptr; }
int max_prime_factor(int n) {
  int maxp = 1;
  for (int p = 2; p * p <= n; ++p) while (n % p == 0) { maxp = p > maxp ? p : maxp; n /= p; }
  return n > maxp ? n : maxp;
}
// a 31-smooth length of 256 .. 4096 points can get a panel kernel compiled at plan time
bool rtc_candidate(int n) { return env().rtc && n >= 256 && n <= 4096 && smooth13(n); }
// a length with a prime factor > 13 runs as a Bluestein convolution on a power-of-two panel kernel when 2n - 1 <= 4096
// (lengths built from primes <= 13 stay on the any-length kernel, whose small-radix stages are whole butterflies)
bool blue_panel_candidate(int n, int prec, bool inc, bool outc) {
  return env().bluestein && n >= 32 && n <= 2048 && max_prime_factor(n) > 13 && find_blue(blue_m(n), prec, inc, outc) != nullptr;
}

// convolution length of a Bluestein line through scratch (long_pass): not the next power of two -- up to twice 2n - 1 -- but
// the shortest M >= 2n - 1 of the form (64 | 32) x L, L a precompiled register length: a fused four-step line (10007 points:
// M = 20480 instead of 32768).  0: none found, use the power of two
int blue_m_long(int n, int prec) {
  const long long need = 2LL * n - 1;
  const int n1 = prec == OFFT_PREC_F64 ? 64 : 32;
  if (!find_tw4(n1, prec)) return 0;
  long long best = 0;
  for (auto &v : registry()) {
    const VariantKey &k = v.key;
    if (k.prec != prec || !k.inc || !k.outc || k.role != Role::Plain || v.id != 0 || k.n < 64 || k.n > 4096) continue;
    const long long m = (long long)n1 * k.n;
    if (m >= need && m < (1LL << 24) && (!best || m < best)) best = m;
  }
  return best && best < blue_m(n) ? (int)best : 0;
}

template <typename T>
int blue_build(int n, int prec, BlueTab &tb, int m_override = 0) {
  using V2 = typename vec2<T>::type;
  const int m = m_override ? m_override : blue_m(n);
  const long double pi = 3.14159265358979323846264338327950288419716939937510L;
  // angle pi k^2 / n with k^2 reduced mod 2n in integers: exact argument reduction
  auto ang = [&](long long k) { return pi * (long double)((k * k) % (2LL * n)) / (long double)n; };
  std::vector<V2> a(n), b(m);
  for (int k = 0; k < n; ++k) { a[k].x = (T)cosl(ang(k)); a[k].y = (T)(-sinl(ang(k))); }
  for (int k = 0; k < m; ++k) { b[k].x = 0; b[k].y = 0; }
  for (int k = 0; k < n; ++k) {
    V2 w; w.x = (T)cosl(ang(k)); w.y = (T)sinl(ang(k));
    b[k] = w;
    if (k) b[m - k] = w;
  }
  HIPK_CHECK(hipMalloc(&tb.chirp, a.size() * sizeof(V2)));
  HIPK_CHECK(hipMemcpy(tb.chirp, a.data(), a.size() * sizeof(V2), hipMemcpyHostToDevice));
  HIPK_CHECK(hipMalloc(&tb.bhat, b.size() * sizeof(V2)));
  HIPK_CHECK(hipMemcpy(tb.bhat, b.data(), b.size() * sizeof(V2), hipMemcpyHostToDevice));
  tb.m = m;
  // B^ = FFT_M(b) / M with the M-point panel kernel itself, in place, one line
  if (offt_hipk_prepare(m, prec)) return -1;
  offt_pass_desc d;
  memset(&d, 0, sizeof d);
  d.n = m; d.precision = prec; d.direction = -1; d.ncols = 1; d.nb1 = d.nb2 = 1;
  d.in_axis_stride = d.out_axis_stride = 1; d.in_col_stride = d.out_col_stride = m;
  d.in_contig = d.out_contig = 1; d.variant = -1; d.scale = 1.0 / (double)m;
  if (offt_hipk_fft_pass(&d, tb.bhat, tb.bhat, nullptr)) return -1;
  HIPK_CHECK(hipStreamSynchronize(nullptr));
  return 0;
}

// XCD-aware panel order (panel_of_block): runs of G = 32 neighbouring panels per XCD by default,
// OFFT_XCD_REMAP=0 turns it off, OFFT_XCD_REMAP=<power of two> sets G
void xcd_order(long long nblk, unsigned *lim, unsigned *gshift) {
  const int g = env().xcd_remap;
  unsigned gs = 0;
  while (g > 1 && (2 << gs) <= g) ++gs;
  *gshift = gs;
  *lim = g > 0 ? (unsigned)((nblk >> (gs + 3)) << (gs + 3)) : 0u;
}

// Column-pair kernels (T = f32x2, offt_panel.hpp) take a descriptor with an even column count whose strided sides put the
// two columns of a pair into 16 contiguous, 16-B aligned bytes: unit column stride, every other stride even (the base
// pointers are checked at launch).  A contiguous side moves the two columns separately and needs nothing.
bool pair_ok(const offt_pass_desc *d) {
  if (d->precision != OFFT_PREC_F32 || d->real_input || (d->ncols & 1)) return false;
  auto even = [](long long x) { return (x & 1) == 0; };
  // (a per-block base table replaces the block stride; its entries are the host's to keep even: offt_host.c elem_delta)
  if (!d->in_contig && !(d->in_col_stride == 1 && even(d->in_axis_stride) && even(d->in_b1_stride) && even(d->in_b2_stride) &&
                         ((d->in_split && d->in_block_tab) || even(d->in_block_stride))))
    return false;
  if (!d->out_contig && !(d->out_col_stride == 1 && even(d->out_axis_stride) && even(d->out_b1_stride) && even(d->out_b2_stride) &&
                          ((d->out_split && d->out_block_tab) || even(d->out_block_stride))))
    return false;
  return true;
}

// the panel-kernel variant that will run this descriptor, or nullptr (-> any-length kernel)
Variant *pick_variant0(const offt_pass_desc *d, bool allow_pair) {
  if (d->real_input == 1 && (!d->in_contig || d->in_axis_stride != 1 || d->in_split || d->direction > 0)) return nullptr;
  // real output: n reals at the head of a row, no split on the store side (the mirror image of the real-input restrictions)
  if (d->real_input == 2 && (!d->out_contig || d->out_axis_stride != 1 || d->out_split || d->out_split_nfloor)) return nullptr;
  const bool inc = d->in_contig != 0, outc = d->out_contig != 0, r2c = d->real_input == 1, c2r = d->real_input == 2;
  const bool uneven = d->in_split_nfloor > 0 || d->out_split_nfloor > 0;
  const bool odd_split = (d->in_split && !is_pow2(d->in_split)) || (d->out_split && !is_pow2(d->out_split));
  int want = d->variant;
  if (want >= VARIANT_PAIR0 || (want < 0 && env().f32_pairs && !d->no_pairs)) {
    if (allow_pair && !uneven && !odd_split && pair_ok(d)) {
      Variant *p = find_variant(plain_key(d->n, OFFT_PREC_F32_PAIR, inc, outc), want < 0 ? -1 : want - VARIANT_PAIR0);
      if (p && (want >= 0 ? p->id == want - VARIANT_PAIR0 : p->is_default)) return p;
    }
    if (want >= VARIANT_PAIR0) want = -1;
  }
  const VariantKey key{d->n, d->precision, inc, outc, r2c ? Role::R2C : c2r ? Role::C2R : Role::Plain, false, 0};
  Variant *v = find_variant(key, r2c || c2r ? -1 : want);
  if (!v) return nullptr;
  if (v->mixed || !(uneven || odd_split)) return v;
  // fft_panel_k addresses per-peer blocks with shifts: other block lengths go to the length's fft_panelx_k instance
  Variant *w = find_variant(key, VARIANT_ANYSPLIT);
  return (w && w->id == VARIANT_ANYSPLIT) ? w : nullptr;
}

// ... and its cache-keeping twin when the descriptor asks for one (out_keep) and one is registered
Variant *pick_variant(const offt_pass_desc *d, bool allow_pair = true) {
  if (d->tw4) {  // first sub-pass of a four-step line: the strided / strided kernel with the twiddles on its stores, or nothing
    if (d->in_contig || d->out_contig || d->real_input || d->in_split_nfloor || d->out_split_nfloor) return nullptr;
    if ((d->in_split && !is_pow2(d->in_split)) || (d->out_split && !is_pow2(d->out_split))) return nullptr;
    return find_tw4(d->n, d->precision);
  }
  Variant *v = pick_variant0(d, allow_pair);
  if (v && d->out_keep && env().keep_stores && !v->mixed && v->key.role == Role::Plain) {
    VariantKey twin = v->key;
    twin.keep = true;
    Variant *k = find_variant(twin, v->id);
    if (k && k->id == v->id) return k;
  }
  return v;
}

// Zero-padded half lines (offt_pass_desc::half = 1 or 2): the fft_half_panel_k instance (a power of two from 64 to 1024
// points) or the fft_half_panelx_k instance (the mixed-radix lengths of offt_reg_half_mixed_*.hip, one column per lane)
// that takes the descriptor, or
// nullptr -- there is no other route for such a pass.  Complex lines without a split or four-step twiddles, in the forms
// the z-y-x half-box schedule and its mirror launch: bit 1 on a contiguous load side, bit 2 on a contiguous store side,
// never strided on both sides.  Single precision: the column-pair instance where the descriptor is eligible (pair_ok)
// and one is registered, else the one-column one.  No cache-keeping twins: out_keep is ignored.
// Real rows, the two ends of that schedule on a real-input plan, in exactly two forms: the real-input pass with bit 1,
// contiguous in / strided out (fft_half_r2c_panel_k), and the real-output pass with bit 2, strided in / contiguous out
// (fft_half_c2r_panel_k), with the restrictions the full-line real passes have (pick_variant0).  Every other real form: none.
// Bit 4 of offt_pass_desc::half is a permission, not a form: the two real forms at a mixed-radix length
// (fft_half_r2c_panelx_k, fft_half_c2r_panelx_k) are handed out only to a descriptor that carries it.  A power-of-two real
// row resolves with it as without it; on a complex descriptor, or without bit 1 or 2, it has no kernel.
Variant *pick_half(const offt_pass_desc *d, bool allow_pair = true) {
  if (!d || (d->half & ~7) || d->n < 2 || (d->n & 1)) return nullptr;
  const int half = d->half & 3;
  const bool real_mixed = (d->half & 4) != 0;
  if ((half != 1 && half != 2) || (real_mixed && !d->real_input)) return nullptr;
  if (d->precision != OFFT_PREC_F64 && d->precision != OFFT_PREC_F32) return nullptr;
  if (d->tw4 || d->in_split || d->in_split_nfloor || d->out_split || d->out_split_nfloor) return nullptr;
  const bool inc = d->in_contig != 0, outc = d->out_contig != 0;
  if (d->real_input) {
    const bool r2c = d->real_input == 1 && half == 1 && inc && !outc && d->in_axis_stride == 1 && d->direction <= 0;
    const bool c2r = d->real_input == 2 && half == 2 && !inc && outc && d->out_axis_stride == 1;
    if (!r2c && !c2r) return nullptr;
    Variant *v = find_variant(VariantKey{d->n, d->precision, inc, outc, r2c ? Role::R2C : Role::C2R, false, half});
    return v && (!v->mixed || real_mixed) ? v : nullptr;
  }
  if (half == 1 ? !inc : !outc) return nullptr;
  if (allow_pair && env().f32_pairs && !d->no_pairs && pair_ok(d)) {
    Variant *p = find_variant(VariantKey{d->n, OFFT_PREC_F32_PAIR, inc, outc, Role::Plain, false, half});
    if (p) return p;
  }
  return find_variant(VariantKey{d->n, d->precision, inc, outc, Role::Plain, false, half});
}

// 1 if the descriptor, with out_keep set, runs on a kernel whose stores stay cached (a KEEP twin exists for its shape)
extern "C" int offt_hipk_keeps_output(const offt_pass_desc *d) {
  if (d->half) return 0;  // the half-line kernels have no cache-keeping twins
  offt_pass_desc k = *d;
  k.out_keep = 1;
  const Variant *v = pick_variant(&k);
  return v && v->key.keep;
}

// ---------------------------------------------------------------------------
// Four-step decomposition: lines no single kernel takes.
//
// FFTW plans any length (offt-compute.c:335-341, 416-425); the panel kernels end at 4096 points (8192 with one column per
// workgroup), the any-length kernel where two images of a line fill the LDS (5120 double / 10240 single points).  A longer
// line of n = n1 n2 points is transformed as  X[k1 + n1 k2] = sum_{j2} w_n^(j2 k1) [ sum_{j1} x[j1 n2 + j2] w_n1^(j1 k1) ] w_n2^(j2 k2):
//   A  n2 x (n1-point FFTs over j1)   -- any kernel of the library, reading the caller's layout (splits, block tables)
//   T  times w_n^(j2 k1)              -- the exact full-wave table of n; j2 k1 < n, so no reduction
//   C  n1 x (n2-point FFTs over j2)   -- any kernel, writing the caller's layout
// through a dense scratch S[column][k1][j2] (j2 contiguous).  A side whose unit-stride dimension is the axis takes the
// j2 / k1 index as the sub-pass's columns; a side whose columns are unit-stride keeps them as columns -- every access
// stays a 128-B segment.  For a strided-in pass step A writes S'[k1][j2][column] and T transposes on the way.
// Three sweeps over the data instead of one: a correctness net with decent bandwidth, not a tuned path.
// ---------------------------------------------------------------------------
struct FourStep { int n1 = 0, n2 = 0; void *t4 = nullptr; bool all = false; };  // all: every flavour goes this way (no register kernel for n)  // t4[k1][j2] = w_n^(k1 j2), from the exact full-wave table
std::mutex g_four_mu;
std::map<std::pair<int, int>, FourStep> g_four;
// scratch per caller stream and per NESTING DEPTH of the decomposing paths: a four-step line whose sub-pass goes through scratch
// lines (a real-input line gathered as complex; a factor that runs as a Bluestein convolution), whose power-of-two lines are
// four-step lines again ... every level keeps its own buffers while the levels below it run.  Slots 3 d + {0, 1}: four-step of
// depth d, 3 d + 2: lines through scratch of depth d
enum { SCRATCH_DEPTHS = 4 };
struct Scratch { void *p[3 * SCRATCH_DEPTHS] = {}; size_t bytes[3 * SCRATCH_DEPTHS] = {}; };
thread_local int g_scratch_depth = 0;
struct DepthGuard {
  int d;
  DepthGuard() : d(g_scratch_depth++) {}
  ~DepthGuard() { --g_scratch_depth; }
};
std::map<void *, Scratch> g_four_scratch;  // per stream

bool four_lookup(int n, int prec, FourStep *out) {
  std::lock_guard<std::mutex> lk(g_four_mu);
  auto it = g_four.find(std::make_pair(n, prec));
  if (it == g_four.end()) return false;
  if (out) *out = it->second;
  return true;
}

// a single launch can transform lines of n points: a panel kernel, the Bluestein kernel, or the any-length kernel
bool direct_ok(int n, int prec) {
  BlueTab bt;
  return has_panel(n, prec) || blue_lookup(n, prec, &bt) || fits_any_length(n, prec);
}

void *four_scratch(void *stream, int which, size_t bytes) {
  std::lock_guard<std::mutex> lk(g_four_mu);
  Scratch &sc = g_four_scratch[stream];
  if (sc.bytes[which] < bytes) {
    if (sc.p[which]) { (void)hipStreamSynchronize((hipStream_t)stream); (void)hipFree(sc.p[which]); }
    sc.p[which] = nullptr; sc.bytes[which] = 0;
    if (hipMalloc(&sc.p[which], bytes) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    sc.bytes[which] = bytes;
  }
  return sc.p[which];
}

// t4[k1][j2] = tw[k1 j2] (k1 j2 < n)
template <typename V2>
__global__ void __launch_bounds__(256) four_table_k(V2 *t4, const V2 *tw, int n, int n2) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) t4[i] = tw[(long long)(i / n2) * (i % n2)];
}
// T, in place: S[q][k1][j2] *= w_n^(+-(k1 j2))
template <typename V2>
__global__ void __launch_bounds__(256) four_twiddle_k(V2 *s, const V2 *tw, long long total, int n1, int n2, int conj) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int j2 = (int)(i % n2), k1 = (int)((i / n2) % n1);
  const V2 w = tw[k1 * j2];
  const V2 x = s[i];
  const auto wy = conj ? -w.y : w.y;
  V2 r;
  r.x = x.x * w.x - x.y * wy;
  r.y = x.x * wy + x.y * w.x;
  s[i] = r;
}
// T for a strided-in pass: S'[b][m][c] (m = k1 n2 + j2 < n, c < cc) -> S[b][c][m] times w_n^(+-(k1 j2)), 32 x 32 tiles through LDS
template <typename V2>
__global__ void __launch_bounds__(256) four_twiddle_t_k(const V2 *sp, V2 *s, const V2 *tw, int n, int cc, int n2, int conj) {
  __shared__ V2 tile[32][33];
  const long long b = blockIdx.z;
  const int m0 = blockIdx.y * 32, c0 = blockIdx.x * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int r = ty; r < 32; r += 8) {
    const int m = m0 + r, c = c0 + tx;
    if (m < n && c < cc) tile[r][tx] = sp[(b * n + m) * cc + c];
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    const int c = c0 + r, m = m0 + tx;
    if (m < n && c < cc) {
      const V2 x = tile[tx][r];
      const int k1 = m / n2, j2 = m - k1 * n2;
      const V2 w = tw[k1 * j2];
      const auto wy = conj ? -w.y : w.y;
      V2 o;
      o.x = x.x * w.x - x.y * wy;
      o.y = x.x * wy + x.y * w.x;
      s[(b * cc + c) * n + m] = o;
    }
  }
}

// ---------------------------------------------------------------------------
// Lines through a dense scratch: the last net under "FFTW plans any length".
//   * a line no single launch takes and no four-step split fits (a prime beyond the any-length kernel, or a prime factor
//     too large itself) runs as a Bluestein convolution on M-point lines, M the power of two >= 2n - 1:
//       gather x[j] a[j] into U[line][0..M) (zero padded) | FFT_M | times B^ | FFT_M^-1 | scatter a[k] U[line][k], k < n
//     with the library's own M-point path (a panel kernel or the four-step decomposition) on contiguous lines;
//   * a real-input line too long for the r2c kernels is gathered as complex, transformed by the complex path of the same
//     length, and its first n/2 + 1 outputs scattered; a real-output line (c2r) is gathered as the conjugate-symmetric
//     extension of its n/2 + 1 values, and the real parts of the n outputs scattered.
// Seven (three) sweeps over scratch lines of twice the length: a few per cent of the roofline -- it exists so that no
// grid the reference accepts is refused, not to be fast.
// ---------------------------------------------------------------------------
struct LongTab { void *chirp = nullptr, *bhat = nullptr; int m = 0; };
std::mutex g_long_mu;  // (its own lock: blue_build runs an M-point pass while the Bluestein registry's is held, and every pass looks here)
std::map<std::pair<int, int>, LongTab> g_long;
bool long_lookup(int n, int prec, LongTab *out) {
  std::lock_guard<std::mutex> lk(g_long_mu);
  auto it = g_long.find(std::make_pair(n, prec));
  if (it == g_long.end()) return false;
  if (out) *out = it->second;
  return true;
}

// U[l][j] = x_line(line0 + l)[j] (* chirp[j]), j < n; 0 for n <= j < m.  Lines are numbered (b2, b1, column), column fastest
template <typename T>
__global__ void __launch_bounds__(256)
long_gather_k(GenArgs a, const typename vec2<T>::type *in, typename vec2<T>::type *U, const typename vec2<T>::type *chirp, int m,
              long long line0, long long total) {
  using V2 = typename vec2<T>::type;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int j = (int)(i % m);
  const long long L = line0 + i / m;
  const int c = (int)(L % a.ncols);
  const long long r = L / a.ncols;
  const int b1 = (int)(r % a.nb1), b2 = (int)(r / a.nb1);
  V2 x; x.x = 0; x.y = 0;
  if (j < a.n) {
    const V2 *src = in + (long long)b1 * a.in_b1 + (long long)b2 * a.in_b2 + (long long)c * a.in_col;
    if (a.real_in == 1) x.x = reinterpret_cast<const T *>(src)[j];
    else if (a.real_in == 2) {  // real output: the conjugate-symmetric extension of the n/2+1 stored values
      const bool lo = 2 * j <= a.n;
      x = src[split_off(lo ? j : a.n - j, a.in_split, a.in_nfloor, a.in_blk, a.in_axis, a.in_tab)];
      if (!lo) x.y = -x.y;
    } else x = src[split_off(j, a.in_split, a.in_nfloor, a.in_blk, a.in_axis, a.in_tab)];
    if (a.conj) x.y = -x.y;
    if (chirp) { const V2 w = chirp[j]; V2 t; t.x = x.x * w.x - x.y * w.y; t.y = x.x * w.y + x.y * w.x; x = t; }
  }
  U[i] = x;
}
// U[l][k] *= bhat[k]
template <typename V2>
__global__ void __launch_bounds__(256) long_mul_k(V2 *U, const V2 *bhat, int m, long long total) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const V2 w = bhat[(int)(i % m)], x = U[i];
  V2 t; t.x = x.x * w.x - x.y * w.y; t.y = x.x * w.y + x.y * w.x;
  U[i] = t;
}
// out_line(line0 + l)[k] = U[l][k] (* chirp[k]) * scale, k < kend
template <typename T>
__global__ void __launch_bounds__(256)
long_scatter_k(GenArgs a, const typename vec2<T>::type *U, typename vec2<T>::type *out, const typename vec2<T>::type *chirp, int m, int kend,
               long long line0, long long total) {
  using V2 = typename vec2<T>::type;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int k = (int)(i % kend);
  const long long l = i / kend, L = line0 + l;
  const int c = (int)(L % a.ncols);
  const long long r = L / a.ncols;
  const int b1 = (int)(r % a.nb1), b2 = (int)(r / a.nb1);
  V2 x = U[l * m + k];
  if (chirp) { const V2 w = chirp[k]; V2 t; t.x = x.x * w.x - x.y * w.y; t.y = x.x * w.y + x.y * w.x; x = t; }
  V2 o;
  o.x = x.x * (T)a.scale;
  o.y = (a.conj ? -x.y : x.y) * (T)a.scale;
  V2 *dst = out + (long long)b1 * a.out_b1 + (long long)b2 * a.out_b2 + (long long)c * a.out_col;
  if (a.real_in == 2) reinterpret_cast<T *>(dst)[k] = o.x;  // real output: n reals at the head of the row
  else dst[split_off(k, a.out_split, a.out_nfloor, a.out_blk, a.out_axis, a.out_tab)] = o;
}

// ---------------------------------------------------------------------------
// Which kernel runs a pass.  resolve() is the one place that decides it, and its body IS the order of precedence; the
// launchers below only pack arguments.  Two layers: the decomposing routes (four-step, lines through scratch) launch
// sub-passes that come back through offt_hipk_fft_pass, the direct routes are one launch.
// ---------------------------------------------------------------------------
enum class Via { FourStep, ScratchLines, Panel, BluePanel, AnyLength };
struct Route {
  Via via = Via::AnyLength;
  Variant *v = nullptr;       // Panel
  BlueVariant *bv = nullptr;  // BluePanel, on the tables bt
  BlueTab bt;
  FourStep fs;                // FourStep
  LongTab lt;                 // ScratchLines; lt.m == 0: plain complex lines of n points, no Bluestein convolution
};

// the direct layer: the single launch that takes the descriptor (what offt_hipk_kernel_name names)
void resolve_direct(const offt_pass_desc *d, const void *in, const void *out, Route *r) {
  // 1. a panel kernel (column pairs, any-split instance, cache-keeping twin, plan-time instance: pick_variant)
  r->v = pick_variant(d);
  if (r->v && r->v->key.prec == OFFT_PREC_F32_PAIR &&
      ((!d->in_contig && ((uintptr_t)in & 15)) || (!d->out_contig && ((uintptr_t)out & 15))))
    r->v = pick_variant(d, false);  // a strided side off the 16-B grid: the one-column kernels
  if (r->v) { r->via = Via::Panel; return; }
  // 2. Bluestein: the M-point panel machinery on a complex line of n points (offt_bluestein.hpp)
  if (!d->real_input && blue_lookup(d->n, d->precision, &r->bt) &&
      (r->bv = find_blue(r->bt.m, d->precision, d->in_contig != 0, d->out_contig != 0)) != nullptr) {
    r->via = Via::BluePanel;
    return;
  }
  // 3. the any-length kernel
  r->via = Via::AnyLength;
}

Route resolve(const offt_pass_desc *d, const void *in, const void *out) {
  Route r;
  // 1. four-step: a length no single launch takes (no panel kernel, and two images of a line do not fit the LDS) always;
  //    8192 points (a register kernel with one column per workgroup) for its strided flavours; a length the any-length
  //    kernel could take as well stays there for what the decomposition does not follow
  if (four_lookup(d->n, d->precision, &r.fs)) {
    const bool no_direct = !has_panel(d->n, d->precision) && !fits_any_length(d->n, d->precision);
    // the decomposition follows complex lines whose per-peer split cuts the axis into whole runs of n2 inputs / n1 outputs
    const bool follows = !d->real_input && !(d->in_split && (d->in_split_nfloor || d->in_split % r.fs.n2)) &&
                         !(d->out_split && (d->out_split_nfloor || d->out_split % r.fs.n1));
    if (no_direct || (r.fs.all ? follows : !(d->in_contig && d->out_contig))) {
      // 2. ... and what it does not follow (real input or output: gathered as complex lines; uneven blocks: gathered with
      //    the split) goes through scratch as plain contiguous lines of the same length
      r.via = follows ? Via::FourStep : Via::ScratchLines;
      return r;
    }
  }
  // 3. a length without a split: a Bluestein convolution on M-point lines through scratch
  if (long_lookup(d->n, d->precision, &r.lt)) { r.via = Via::ScratchLines; return r; }
  // 4. one launch: panel kernel, Bluestein panel kernel, any-length kernel
  resolve_direct(d, in, out, &r);
  if (r.via != Via::AnyLength) return r;
  if (!d->real_input) {
    // 4b. a complex line with a register kernel of its own but blocks that kernel cannot address, beyond the any-length
    //     kernel (8192 double-precision points, contiguous / contiguous, uneven blocks -- the strided flavours took the
    //     four-step branch above): gathered with the split, transformed as plain contiguous lines
    if (has_panel(d->n, d->precision) && !fits_any_length(d->n, d->precision)) r.via = Via::ScratchLines;
    return r;
  }
  // 5. a REAL-input (or real-output) line of a Bluestein length: gathered as complex lines into scratch, transformed there by
  //    the Bluestein panel kernel, the first n/2 + 1 outputs (the n real parts) scattered -- three sweeps, against a radix of the
  //    size of its largest prime factor on the any-length kernel (OFFT_R2C_BLUESTEIN=0: that kernel, as in rounds 1-2)
  if (env().r2c_bluestein && blue_lookup(d->n, d->precision, &r.bt) && find_blue(r.bt.m, d->precision, true, true)) r.via = Via::ScratchLines;
  // 6. a real-output line of a length beyond the any-length kernel whose descriptor no panel kernel takes (8192 points with
  //    blocks fft_panel_k cannot address): through scratch lines, like the four-step route of such a line
  else if (d->real_input == 2 && !fits_any_length(d->n, d->precision)) r.via = Via::ScratchLines;
  return r;
}

// four-step twiddles ride on the stores of a TW4 panel instance and of nothing else: every other route would drop them
bool drops_tw4(const offt_pass_desc *d, const Route &r) { return d->tw4 && !(r.via == Via::Panel && r.v->key.role == Role::TW4); }

// ---- packing and launching ----
int log2i(int n) { int l = 0; while ((1 << l) < n) ++l; return l; }

// conv: fft_conv_panel_k works in place through the load side of contiguous lines without a split -- everything else stays zero
PassArgs pass_args(const offt_pass_desc *d, int cols, bool conv = false) {
  PassArgs a;
  memset(&a, 0, sizeof a);
  a.in_axis = d->in_axis_stride; a.in_col = d->in_col_stride; a.in_b1 = d->in_b1_stride; a.in_b2 = d->in_b2_stride;
  a.in_shift = a.out_shift = 31;
  a.ncols = d->ncols; a.ncp = (d->ncols + cols - 1) / cols; a.nb1 = d->nb1;
  a.scale = d->scale;
  if (conv) return a;
  a.out_axis = d->out_axis_stride; a.out_col = d->out_col_stride; a.out_b1 = d->out_b1_stride; a.out_b2 = d->out_b2_stride;
  a.in_blk = d->in_block_stride; a.out_blk = d->out_block_stride;
  if (d->in_split) a.in_shift = log2i(d->in_split);
  if (d->out_split) a.out_shift = log2i(d->out_split);
  a.in_split = d->in_split; a.out_split = d->out_split;
  a.in_inv = d->in_split ? 1.0f / (float)d->in_split : 0.0f;
  a.out_inv = d->out_split ? 1.0f / (float)d->out_split : 0.0f;
  a.in_nfloor = d->in_split_nfloor; a.out_nfloor = d->out_split_nfloor;
  a.in_lim = d->in_split_nfloor ? d->in_split * d->in_split_nfloor : d->n;   // even split: every index below lim
  a.out_lim = d->out_split_nfloor ? d->out_split * d->out_split_nfloor : d->n;
  a.in_inv1 = 1.0f / (float)(d->in_split + 1);
  a.out_inv1 = 1.0f / (float)(d->out_split + 1);
  a.conj = d->direction > 0;
  a.in_tab = d->in_split ? d->in_block_tab : nullptr;
  a.out_tab = d->out_split ? d->out_block_tab : nullptr;
  a.tw4 = d->tw4; a.tw4_b1 = d->tw4_b1; a.tw4_n2 = d->tw4_n2;
  return a;
}

// the addressing of a descriptor for the any-length kernel and the gather / scatter sweeps of the scratch lines
GenArgs gen_args(const offt_pass_desc *d) {
  GenArgs g;
  memset(&g, 0, sizeof g);
  g.in_axis = d->in_axis_stride; g.in_col = d->in_col_stride; g.in_b1 = d->in_b1_stride; g.in_b2 = d->in_b2_stride;
  g.out_axis = d->out_axis_stride; g.out_col = d->out_col_stride; g.out_b1 = d->out_b1_stride; g.out_b2 = d->out_b2_stride;
  g.in_blk = d->in_block_stride; g.out_blk = d->out_block_stride;
  g.in_split = d->in_split; g.in_nfloor = d->in_split_nfloor;
  g.out_split = d->out_split; g.out_nfloor = d->out_split_nfloor;
  g.n = d->n; g.ncols = d->ncols; g.nb1 = d->nb1;
  g.conj = d->direction > 0;
  g.real_in = d->real_input;
  g.scale = d->scale;
  g.in_tab = d->in_split ? d->in_block_tab : nullptr;
  g.out_tab = d->out_split ? d->out_block_tab : nullptr;
  return g;
}

// One launch of a kernel with dynamic LDS on a grid of nblk panels in XCD-aware order: the dynamic-LDS attribute is set
// once per kernel (lds_attr: the largest footprint it will be launched with), a plan-time instance is a module function
int launch(const char *who, const void *fn, void *modfn, bool *attr_set, size_t lds_attr, size_t lds, unsigned threads, long long nblk,
           unsigned *xcd_lim, unsigned *xcd_gshift, void **args, hipStream_t st) {
  if (nblk > 0x7fffffffLL) { snprintf(g_err, sizeof g_err, "%s: grid too large", who); return -1; }
  xcd_order(nblk, xcd_lim, xcd_gshift);
  if (modfn) {
    HIPK_CHECK(hipModuleLaunchKernel((hipFunction_t)modfn, (unsigned)nblk, 1, 1, threads, 1, 1, (unsigned)lds, st, args, nullptr));
    return 0;
  }
  if (!*attr_set) {
    if (lds_attr > 48 * 1024) HIPK_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_attr));
    *attr_set = true;
  }
  HIPK_CHECK(hipLaunchKernel(fn, dim3((unsigned)nblk), dim3(threads), args, lds, st));
  return 0;
}

// the small kernels exist once per precision: run a statement with T = double / float and V2 = double2 / float2
template <typename F>
void by_precision(int prec, F &&f) { if (prec == OFFT_PREC_F64) f(double{}); else f(float{}); }
#define FOR_PREC(prec, ...) \
  by_precision(prec, [&](auto t_) { using T = decltype(t_); using V2 = typename vec2<T>::type; (void)sizeof(V2); __VA_ARGS__; })

int launch_panel(const offt_pass_desc *d, const void *in, void *out, const Tables &tb, hipStream_t st, Variant *v) {
  if (d->tw4 && v->key.role != Role::TW4) { snprintf(g_err, sizeof g_err, "offt_hipk_fft_pass: no kernel with four-step twiddles for n=%d", d->n); return -1; }
  PassArgs a = pass_args(d, v->cols);
  // every panel kernel stages its twiddles from the exact full-wave table w^m, m < n (the quarter- and half-wave
  // tables they keep in LDS are prefixes of it)
  void *args[] = {(void *)&a, (void *)&in, (void *)&out, (void *)&tb.full};
  return launch("offt_hipk_fft_pass", v->fn, v->modfn, &v->attr_set, v->lds, v->lds, v->threads, (long long)a.ncp * d->nb1 * d->nb2,
                &a.xcd_lim, &a.xcd_gshift, args, st);
}

int launch_blue_panel(const offt_pass_desc *d, const void *in, void *out, hipStream_t st, BlueVariant *bv, const BlueTab &bt) {
  if (d->tw4) { snprintf(g_err, sizeof g_err, "offt_hipk_fft_pass: no kernel with four-step twiddles for n=%d", d->n); return -1; }
  PassArgs a = pass_args(d, bv->cols);
  Tables tm;
  if (get_tables(bt.m, d->precision, tm, false)) return -1;
  int nlen = d->n;
  void *args[] = {(void *)&a, (void *)&in, (void *)&out, (void *)&tm.full, (void *)&bt.chirp, (void *)&bt.bhat, (void *)&nlen};
  return launch("offt_hipk_fft_pass", bv->fn, nullptr, &bv->attr_set, bv->lds, bv->lds, bv->threads, (long long)a.ncp * d->nb1 * d->nb2,
                &a.xcd_lim, &a.xcd_gshift, args, st);
}

// the any-length kernel's panel for lines of n points: columns per workgroup, twiddles in LDS or not, LDS bytes, workgroup size
struct MixShape { int cols; bool tw_in_lds; size_t lds; unsigned threads; };
MixShape mix_shape(int n, int prec) {
  MixShape s;
  const size_t line = n * elem_size(prec);
  s.cols = 8;
  while (s.cols > 1 && (2 * (size_t)s.cols + 1) * line > LDS_BYTES) s.cols >>= 1;
  s.tw_in_lds = (2 * (size_t)s.cols + 1) * line <= LDS_BYTES;
  s.lds = (2 * (size_t)s.cols + (s.tw_in_lds ? 1 : 0)) * line;
  // the panel's LDS footprint allows one or two workgroups per CU: size the workgroup so that the CU still
  // holds 8-16 waves to cover the LDS round trips between stages
  s.threads = s.lds > 80 * 1024 ? 1024 : s.lds > 40 * 1024 ? 512 : 256;
  while (s.threads > 64 && (long long)s.threads * 2 > (long long)s.cols * n) s.threads >>= 1;  // at least two elements per thread
  if (env().mix_threads >= 64 && env().mix_threads <= 1024) s.threads = (unsigned)env().mix_threads;
  return s;
}

int launch_any_length(const offt_pass_desc *d, const void *in, void *out, const Tables &tb, hipStream_t st) {
  GenArgs g = gen_args(d);
  g.in_contig = d->in_contig; g.out_contig = d->out_contig;
  // radices: prime factors, pairs of 2 merged into 4 (fewer LDS round trips at equal cost)
  int m = d->n, twos = 0;
  while (m % 2 == 0) { twos++; m /= 2; }
  for (; twos >= 2; twos -= 2) g.fac[g.nfac++] = 4;
  if (twos) g.fac[g.nfac++] = 2;
  for (int f = 3; f * f <= m; f += 2)
    while (m % f == 0) {
      if (g.nfac >= OFFT_MIX_MAXFAC) { snprintf(g_err, sizeof g_err, "offt_hipk_fft_pass: n=%d has too many factors", d->n); return -1; }
      g.fac[g.nfac++] = f; m /= f;
    }
  if (m > 1) g.fac[g.nfac++] = m;
  if (d->n == 1) { g.nfac = 0; }
  if (g.nfac > OFFT_MIX_MAXFAC) { snprintf(g_err, sizeof g_err, "offt_hipk_fft_pass: n=%d has too many factors", d->n); return -1; }
  if (!fits_any_length(d->n, d->precision)) { snprintf(g_err, sizeof g_err, "offt_hipk_fft_pass: n=%d too long for the any-length kernel", d->n); return -1; }
  const MixShape ms = mix_shape(d->n, d->precision);
  g.tw_in_lds = ms.tw_in_lds;
  g.cols = ms.cols;
  g.ncp = (d->ncols + ms.cols - 1) / ms.cols;
  static bool attr_set[2] = {false, false};
  const bool f64 = d->precision == OFFT_PREC_F64;
  void *args[] = {(void *)&g, (void *)&in, (void *)&out, (void *)&tb.full};
  return launch("offt_hipk_fft_pass", f64 ? (const void *)fft_mixed_k<double> : (const void *)fft_mixed_k<float>, nullptr, &attr_set[f64 ? 0 : 1],
                LDS_BYTES, ms.lds, ms.threads, (long long)g.ncp * d->nb1 * d->nb2, &g.xcd_lim, &g.xcd_gshift, args, st);
}

int four_pass(const offt_pass_desc *d, const void *in, void *out, void *stream, const FourStep &fs, const Tables &tb) {
  const int N = d->n, N1 = fs.n1, N2 = fs.n2;
  const size_t esz = elem_size(d->precision);
  const bool inL = d->in_contig != 0, outL = d->out_contig != 0;
  // columns per chunk: whole rows of the caller's column dimension, as many b1 entries as fit the chunk's share of scratch
  const size_t cap = ((size_t)env().fourstep_chunk_mib << 20) / esz;
  int cc = d->ncols, cb1 = d->nb1;
  if ((size_t)cc * N > cap) { cc = (int)(cap / N); if (cc < 1) cc = 1; cb1 = 1; }
  else { const size_t fit = cap / ((size_t)cc * N); if ((size_t)cb1 > fit) cb1 = (int)(fit < 1 ? 1 : fit); }
  const size_t sbytes = (size_t)cc * cb1 * N * esz;
  const DepthGuard depth;
  if (depth.d >= SCRATCH_DEPTHS) { snprintf(g_err, sizeof g_err, "four-step path: decomposition nested too deep for n=%d", N); return -1; }
  char *S = (char *)four_scratch(stream, 3 * depth.d + 0, sbytes);
  char *Sp = inL ? nullptr : (char *)four_scratch(stream, 3 * depth.d + 1, sbytes);
  if (!S || (!inL && !Sp)) { snprintf(g_err, sizeof g_err, "four-step path: cannot allocate %zu bytes of scratch", sbytes); return -1; }
  for (int b2 = 0; b2 < d->nb2; ++b2)
    for (int b10 = 0; b10 < d->nb1; b10 += cb1)
      for (int c0 = 0; c0 < d->ncols; c0 += cc) {
        const int nb = d->nb1 - b10 < cb1 ? d->nb1 - b10 : cb1, nc = d->ncols - c0 < cc ? d->ncols - c0 : cc;
        const char *pin = (const char *)in + ((long long)b2 * d->in_b2_stride + (long long)b10 * d->in_b1_stride + (long long)c0 * d->in_col_stride) * (long long)esz;
        char *pout = (char *)out + ((long long)b2 * d->out_b2_stride + (long long)b10 * d->out_b1_stride + (long long)c0 * d->out_col_stride) * (long long)esz;
        // ---- A: n1-point transforms over j1 (input index j1 n2 + j2) ----
        offt_pass_desc a;
        memset(&a, 0, sizeof a);
        a.n = N1; a.precision = d->precision; a.direction = d->direction; a.variant = -1; a.scale = 1.0; a.no_pairs = d->no_pairs;
        a.in_axis_stride = (long long)N2 * d->in_axis_stride;
        if (d->in_split) { a.in_split = d->in_split / N2; a.in_block_stride = d->in_block_stride; a.in_block_tab = d->in_block_tab; }
        a.in_contig = 0; a.out_contig = 0;
        // twiddles fused into A's stores when the n1-point kernel has such a twin: two sweeps instead of three.  A strided-in
        // pass then leaves S'[k1][j2][c] as it is and C reads it with the caller's columns as its columns -- which needs a
        // strided-out pass as well; strided-in / contig-out keeps the transposing twiddle sweep.
        const bool fused = env().fourstep_fuse && (inL || !outL) && (!d->in_split || is_pow2(d->in_split / N2)) &&
                           find_tw4(N1, d->precision) != nullptr;
        if (fused) { a.tw4 = fs.t4; a.tw4_b1 = inL ? 0 : 1; a.tw4_n2 = N2; }
        if (inL) {  // the axis is the unit-stride dimension: j2 becomes the column dimension
          a.ncols = N2; a.in_col_stride = d->in_axis_stride;
          a.nb1 = nc; a.in_b1_stride = d->in_col_stride;
          a.nb2 = nb; a.in_b2_stride = d->in_b1_stride;
          a.out_axis_stride = N2; a.out_col_stride = 1; a.out_b1_stride = N; a.out_b2_stride = (long long)N * nc;  // S[q][k1][j2]
          if (offt_hipk_fft_pass(&a, pin, S, stream)) return -1;
        } else {    // the caller's columns are the unit-stride dimension and stay the columns: S'[b][k1][j2][c]
          a.ncols = nc; a.in_col_stride = d->in_col_stride;
          a.nb1 = N2; a.in_b1_stride = d->in_axis_stride;
          a.nb2 = nb; a.in_b2_stride = d->in_b1_stride;
          a.out_axis_stride = (long long)N2 * nc; a.out_col_stride = 1; a.out_b1_stride = nc; a.out_b2_stride = (long long)N * nc;
          if (offt_hipk_fft_pass(&a, pin, fused ? S : Sp, stream)) return -1;
        }
        // ---- T: twiddles w_n^(j2 k1) (and the transposition S' -> S) ----
        (void)hipGetLastError();
        const int conj = d->direction > 0;
        if (fused) {
          /* nothing: the twiddles rode on A's stores */
        } else if (inL) {
          const long long total = (long long)nc * nb * N;
          const unsigned blocks = (unsigned)((total + 255) / 256);
          FOR_PREC(d->precision, hipLaunchKernelGGL(four_twiddle_k<V2>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (V2 *)S, (const V2 *)tb.full, total, N1, N2, conj));
        } else {
          const dim3 grid((unsigned)((nc + 31) / 32), (unsigned)((N + 31) / 32), (unsigned)nb);
          FOR_PREC(d->precision, hipLaunchKernelGGL(four_twiddle_t_k<V2>, grid, dim3(256), 0, (hipStream_t)stream, (const V2 *)Sp, (V2 *)S, (const V2 *)tb.full, N, nc, N2, conj));
        }
        HIPK_CHECK(hipGetLastError());
        // ---- C: n2-point transforms over j2, output index k1 + n1 k2 ----
        offt_pass_desc c;
        memset(&c, 0, sizeof c);
        c.n = N2; c.precision = d->precision; c.direction = d->direction; c.variant = -1; c.scale = d->scale; c.no_pairs = d->no_pairs;
        c.out_keep = d->out_keep;
        c.in_axis_stride = 1; c.in_contig = 1; c.out_contig = 0;
        c.out_axis_stride = (long long)N1 * d->out_axis_stride;
        if (d->out_split) { c.out_split = d->out_split / N1; c.out_block_stride = d->out_block_stride; c.out_block_tab = d->out_block_tab; }
        if (fused && !inL) {  // S'[b][k1][j2][c] straight from A: the caller's columns are the columns on both sides
          c.in_contig = 0; c.in_axis_stride = nc;
          c.ncols = nc; c.in_col_stride = 1; c.out_col_stride = d->out_col_stride;
          c.nb1 = N1; c.in_b1_stride = (long long)N2 * nc; c.out_b1_stride = d->out_axis_stride;
          c.nb2 = nb; c.in_b2_stride = (long long)N * nc; c.out_b2_stride = d->out_b1_stride;
        } else if (outL) {  // k1 becomes the column dimension of the output
          c.ncols = N1; c.in_col_stride = N2; c.out_col_stride = d->out_axis_stride;
          c.nb1 = nc; c.in_b1_stride = N; c.out_b1_stride = d->out_col_stride;
          c.nb2 = nb; c.in_b2_stride = (long long)N * nc; c.out_b2_stride = d->out_b1_stride;
        } else {     // the caller's columns stay the columns
          c.ncols = nc; c.in_col_stride = N; c.out_col_stride = d->out_col_stride;
          c.nb1 = N1; c.in_b1_stride = N2; c.out_b1_stride = d->out_axis_stride;
          c.nb2 = nb; c.in_b2_stride = (long long)N * nc; c.out_b2_stride = d->out_b1_stride;
        }
        if (offt_hipk_fft_pass(&c, S, pout, stream)) return -1;
      }
  return 0;
}

int long_pass(const offt_pass_desc *d, const void *in, void *out, void *stream, const LongTab &lt) {
  const int N = d->n, M = lt.m ? lt.m : N;   // (lt.m == 0: plain complex lines of N points, the long real-input case)
  const size_t esz = elem_size(d->precision);
  const hipStream_t st = (hipStream_t)stream;
  const GenArgs g = gen_args(d);
  const int kend = d->real_input == 1 ? N / 2 + 1 : N;
  const long long nlines = (long long)d->ncols * d->nb1 * d->nb2;
  long long per = (long long)(((size_t)256 << 20) / ((size_t)M * esz));
  if (per < 1) per = 1;
  if (per > nlines) per = nlines;
  const DepthGuard depth;
  if (depth.d >= SCRATCH_DEPTHS) { snprintf(g_err, sizeof g_err, "lines of %d points through scratch: decomposition nested too deep", N); return -1; }
  char *U = (char *)four_scratch(stream, 3 * depth.d + 2, (size_t)per * M * esz);
  if (!U) { snprintf(g_err, sizeof g_err, "lines of %d points through scratch: cannot allocate %zu bytes", N, (size_t)per * M * esz); return -1; }
  // the M-point transforms of the scratch lines: contiguous lines, in place
  offt_pass_desc f;
  memset(&f, 0, sizeof f);
  f.n = M; f.precision = d->precision; f.variant = -1; f.scale = 1.0; f.no_pairs = d->no_pairs;
  f.in_axis_stride = f.out_axis_stride = 1; f.in_contig = f.out_contig = 1;
  f.in_col_stride = f.out_col_stride = M; f.nb1 = f.nb2 = 1;
  for (long long l0 = 0; l0 < nlines; l0 += per) {
    const long long nl = nlines - l0 < per ? nlines - l0 : per;
    const long long tot = nl * M, tote = nl * kend;
    if (tot > 0x7fffffffLL * 256) { snprintf(g_err, sizeof g_err, "lines of %d points through scratch: chunk too large", N); return -1; }
    const unsigned blocks = (unsigned)((tot + 255) / 256), blockse = (unsigned)((tote + 255) / 256);
    f.ncols = (int)nl;
    (void)hipGetLastError();
    FOR_PREC(d->precision, hipLaunchKernelGGL(long_gather_k<T>, dim3(blocks), dim3(256), 0, st, g, (const V2 *)in, (V2 *)U, (const V2 *)lt.chirp, M, l0, tot));
    HIPK_CHECK(hipGetLastError());
    f.direction = -1;
    if (offt_hipk_fft_pass(&f, U, U, stream)) return -1;
    if (lt.m) {
      FOR_PREC(d->precision, hipLaunchKernelGGL(long_mul_k<V2>, dim3(blocks), dim3(256), 0, st, (V2 *)U, (const V2 *)lt.bhat, M, tot));
      HIPK_CHECK(hipGetLastError());
      f.direction = +1;
      if (offt_hipk_fft_pass(&f, U, U, stream)) return -1;
    }
    FOR_PREC(d->precision, hipLaunchKernelGGL(long_scatter_k<T>, dim3(blockse), dim3(256), 0, st, g, (const V2 *)U, (V2 *)out, (const V2 *)lt.chirp, M, kend, l0, tote));
    HIPK_CHECK(hipGetLastError());
  }
  return 0;
}

// ---- plan time: the steps of offt_hipk_prepare ----
int blue_build_for(int n, int prec, BlueTab &bt, int m_override = 0) {
  return prec == OFFT_PREC_F64 ? blue_build<double>(n, prec, bt, m_override) : blue_build<float>(n, prec, bt, m_override);
}

// chirp and B^ of a length that runs on the Bluestein panel kernel
int blue_panel_build(int n, int prec) {
  std::lock_guard<std::mutex> lk(g_blue_mu);
  if (g_blue.count(std::make_pair(n, prec))) return 0;
  BlueTab bt;
  if (blue_build_for(n, prec, bt)) return -1;
  g_blue[std::make_pair(n, prec)] = bt;
  return 0;
}

// The first factor n1 of the four-step split n = n1 n2, or 0: a function of the registry and the switches only
// (candidates are looked up, not prepared).  fused_only: the length has the any-length kernel to fall back on and takes
// nothing but a FUSED split (score < 0)
int choose_four_split(int n, int precision, bool fused_only) {
  int best1 = 0;
  double best_score = 1e30;
  for (int n1 = 2; (long long)n1 * n1 <= n; ++n1) {
    if (n % n1) continue;
    const int n2 = n / n1;
    // both factors need a kernel of their own: prefer precompiled register kernels and a balanced split (candidates are
    // only looked up here, not prepared -- preparing may compile a plan-time kernel, seconds each)
    const bool f1 = has_panel(n1, precision), f2 = has_panel(n2, precision);
    if ((!f1 && !fits_any_length(n1, precision)) || (!f2 && !fits_any_length(n2, precision))) continue;
    double score = std::log((double)n2 / (double)n1);
    if (!f1) score += 4.0;
    if (!f2) score += 4.0;
    // ... except that a SHORT first sub-pass with the twiddles on its stores wins when the other factor still has a register
    // kernel: few points per line, one thread per line on 64 unit-stride columns (8 columns at 64 points).  Order of
    // preference, from sweeps over 8192 / 16384 / 32768 / 6000 / 10000 / 12000 points (profiles/r03_four_step.txt):
    //   double  64 (8192 = 64 x 128: 37.3 % of the roofline, 36.4 % for 32 x 256), then 16, 8, 4 (6000 = 16 x 375: 31.5 %, 10000 =
    //           16 x 625: 31.6 %, both 17-18 % as balanced unfused splits; 12000 = 16 x 750: 26.7 %, 20.1 % for 32 x 375), 32, 2
    //   single  32 (8192 = 32 x 256: 37.5 %, 31.9 % for 64 x 128), then 16, 8, 4, 2
    static const int pref64[] = {64, 16, 8, 4, 32, 2, 0}, pref32[] = {32, 16, 8, 4, 2, 0};
    const int *pref = precision == OFFT_PREC_F64 ? pref64 : pref32;
    // (second choice, behind every split whose long factor is precompiled: a long factor that gets its kernel compiled NOW --
    //  seconds of plan time for 10000 = 16 x 625 at 32 % instead of 100 x 100 at 18 %)
    const bool rtc2 = !f2 && rtc_candidate(n2);
    // (third: a long factor with a prime factor > 13 that runs on the Bluestein panel kernel -- 4076 = 4 x 1019)
    const bool blue2 = !f2 && !rtc2 && blue_panel_candidate(n2, precision, true, false) && blue_panel_candidate(n2, precision, false, false);
    for (int r = 0; pref[r]; ++r)
      if (n1 == pref[r] && (f2 || rtc2 || blue2) && find_tw4(n1, precision))
        score = (f2 ? -10.0 : rtc2 ? -5.0 : -3.0) + 0.1 * r;
    // a factor that would itself go through scratch lines (or the any-length kernel with a radix of hundreds) is a last resort
    if (!f1 && max_prime_factor(n1) > 61 && !(n1 <= 2048 && env().bluestein)) score += 8.0;
    if (!f2 && !rtc2 && !blue2 && max_prime_factor(n2) > 61 && !(n2 <= 2048 && env().bluestein)) score += 8.0;
    if (env().fourstep_n1 == n1) score = -100.0;  // (OFFT_FOURSTEP_N1, for sweeps: only among the splits that are possible at all)
    if (score < best_score) { best_score = score; best1 = n1; }
  }
  if (fused_only && best_score >= 0.0) best1 = 0;  // (unfused, three sweeps: the any-length kernel is no worse)
  return best1;
}

// prepare both factors and build t4[k1][j2] = w_n^(k1 j2); a split whose factors turn out to have no kernel is dropped (0)
int four_build(int n, int precision, int n1, const Tables &tb) {
  if (offt_hipk_prepare(n1, precision) || offt_hipk_prepare(n / n1, precision) || !direct_ok(n1, precision) || !direct_ok(n / n1, precision))
    return 0;
  FourStep fs; fs.n1 = n1; fs.n2 = n / n1;
  fs.all = !has_panel(n, precision);
  HIPK_CHECK(hipMalloc(&fs.t4, (size_t)n * elem_size(precision)));
  (void)hipGetLastError();
  FOR_PREC(precision, hipLaunchKernelGGL(four_table_k<V2>, dim3((n + 255) / 256), dim3(256), 0, nullptr, (V2 *)fs.t4, (const V2 *)tb.full, n, fs.n2));
  HIPK_CHECK(hipGetLastError());
  HIPK_CHECK(hipStreamSynchronize(nullptr));
  std::lock_guard<std::mutex> lk(g_four_mu);
  g_four[std::make_pair(n, precision)] = fs;
  return 0;
}

// chirp and B^ of a length that runs as a Bluestein convolution on lines of M >= 2n - 1 points through scratch (best effort)
void long_build(int n, int precision) {
  BlueTab bt;
  const int mlong = env().bluestein_long_pow2 ? 0 : blue_m_long(n, precision);
  if (blue_build_for(n, precision, bt, mlong)) return;
  std::lock_guard<std::mutex> lk(g_long_mu);
  LongTab lt; lt.chirp = bt.chirp; lt.bhat = bt.bhat; lt.m = bt.m;
  g_long[std::make_pair(n, precision)] = lt;
}

}  // namespace

extern "C" {

const char *offt_hipk_last_error(void) { return g_err; }

int offt_hipk_has_fast_path(int n, int precision) { return has_panel(n, precision); }

int offt_hipk_variant_count(int n, int precision) {
  std::call_once(g_reg_once, build_registry);
  const VariantKey key = plain_key(n, precision, true, true);
  int c = 0;
  for (auto &v : registry())
    if (v.key == key && v.id < VARIANT_ANYSPLIT) c = v.id + 1 > c ? v.id + 1 : c;
  return c;
}

const char *offt_hipk_variant_name(int n, int precision, int variant) {
  Variant *v = find_variant(plain_key(n, precision, true, true), variant);
  return v ? v->name.c_str() : "mixed-radix any-length";
}

int offt_hipk_variant_info(int n, int precision, int variant, int *elems_per_thread, int *cols) {
  Variant *v = find_variant(plain_key(n, precision, true, true), variant);
  if (!v || (variant >= 0 && v->id != variant)) return -1;
  if (elems_per_thread) *elems_per_thread = v->e;
  if (cols) *cols = v->cols;
  return v->id;
}

// the direct layer of resolve(): a pass that is decomposed (four-step, scratch lines) is named by what would launch it alone
// A panel kernel's name is the registry's: every entry carries the __global__ template it was instantiated from
// (Variant::kernel, "<pairs>" appended for the column-pair instances).  Only the two kernels outside that registry and
// the refusal of a half-line descriptor are spelled here.
const char *offt_hipk_kernel_name(const offt_pass_desc *d) {
  if (d->half) {
    const Variant *h = pick_half(d);
    return h ? h->kernel : "no half-line kernel";
  }
  Route r;
  resolve_direct(d, nullptr, nullptr, &r);
  if (r.via == Via::BluePanel) return "fft_bluestein_k";
  if (r.via == Via::AnyLength) return "fft_mixed_k";
  return r.v->kernel;
}

int offt_hipk_has_half(const offt_pass_desc *d) { return pick_half(d) != nullptr; }

// what offt_hipk_fft_pass does with a descriptor, step for step, with resolve()'s answer reported instead of launched
int offt_hipk_pass_route(const offt_pass_desc *d, int *variant_id, int *n1, int *n2) {
  if (variant_id) *variant_id = -1;
  if (n1) *n1 = 0;
  if (n2) *n2 = 0;
  if (!d || d->n < 1 || d->ncols < 1 || d->nb1 < 1 || d->nb2 < 1) return OFFT_ROUTE_NONE;
  auto panel = [&](const Variant *v) {
    if (variant_id) *variant_id = v->key.prec == OFFT_PREC_F32_PAIR ? VARIANT_PAIR0 + v->id : v->id;
    return (int)OFFT_ROUTE_PANEL;
  };
  if (d->half) {
    const Variant *h = pick_half(d);
    return h ? panel(h) : (int)OFFT_ROUTE_NONE;
  }
  const Route r = resolve(d, nullptr, nullptr);
  if (drops_tw4(d, r)) return OFFT_ROUTE_NONE;
  switch (r.via) {
    case Via::FourStep:
      if (n1) *n1 = r.fs.n1;
      if (n2) *n2 = r.fs.n2;
      return OFFT_ROUTE_FOUR_STEP;
    case Via::ScratchLines: return OFFT_ROUTE_SCRATCH_LINES;
    case Via::Panel: return panel(r.v);
    case Via::BluePanel: return OFFT_ROUTE_BLUESTEIN_PANEL;
    case Via::AnyLength: return fits_any_length(d->n, d->precision) ? (int)OFFT_ROUTE_ANY_LENGTH : (int)OFFT_ROUTE_NONE;
  }
  return OFFT_ROUTE_NONE;
}

int offt_hipk_prepare(int n, int precision) {
  const bool c2r = (precision & OFFT_HIPK_PREP_C2R) != 0;
  precision &= ~OFFT_HIPK_PREP_C2R;
  if (n < 1) { snprintf(g_err, sizeof g_err, "offt_hipk_prepare: bad n=%d", n); return -1; }
  if (c2r) {
    if (offt_hipk_prepare(n, precision)) return -1;
    // real-output instances for a length whose panel kernel was compiled at plan time (the precompiled lengths have theirs);
    // best effort like the complex ones: without them the real-output pass runs on the any-length kernel
    const Variant *v = find_variant(plain_key(n, precision, true, true));
    if (v && v->modfn && env().rtc) (void)rtc_build(n, precision, true);
    return 0;
  }
  // 1. twiddle tables
  Tables tb;
  if (get_tables(n, precision, tb, true)) return -1;
  // 2. a plan-time panel kernel for a candidate length without a precompiled one (best effort)
  if (rtc_candidate(n) && !has_panel(n, precision)) (void)rtc_build(n, precision);
  // 3. a length without any register kernel (a prime factor > 31, or outside 256 .. 4096 and not precompiled): the
  //    Bluestein panel kernel's tables
  if (!has_panel(n, precision) && blue_panel_candidate(n, precision, true, true) && blue_panel_build(n, precision)) return -1;
  // 4. a length no single launch takes (no panel kernel, and two images of a line do not fit the LDS of the any-length
  //    kernel) is split n = n1 n2 for the four-step path; 8192 has a register kernel, but with one column per
  //    workgroup: its strided flavours go the four-step way as well ...
  const bool no_direct = !has_panel(n, precision) && !fits_any_length(n, precision);
  // ... and so does a length that would otherwise run on the any-length kernel -- above the plan-time kernels' range (4800,
  // 5000; in single precision up to 10240 points: 10000 at 15 % of the roofline there) or above the Bluestein panel kernel's with
  // a large prime factor (4076 = 4 x 1019) -- if it has a FUSED split
  BlueTab bt_any;
  const bool any_only = !no_direct && n > 2048 && !has_panel(n, precision) && !blue_lookup(n, precision, &bt_any);
  if ((no_direct || n == 8192 || any_only) && env().fourstep && !four_lookup(n, precision, nullptr)) {
    const int n1 = choose_four_split(n, precision, any_only);
    if (n1 && four_build(n, precision, n1, tb)) return -1;
  }
  // 5. ... and a length without a split becomes a Bluestein convolution on lines of M >= 2n - 1 points through scratch
  //    (also a length the any-length kernel COULD take, but only with a radix of hundreds -- r multiply-adds per output: 3057 =
  //     3 x 1019 points ran at 0.6 % of the roofline there)
  if ((no_direct || (any_only && max_prime_factor(n) > 61)) && !four_lookup(n, precision, nullptr) && env().bluestein_long &&
      env().fourstep /* (its M-point lines need the four-step path) */ && env().bluestein && n < (1 << 24) && !long_lookup(n, precision, nullptr))
    long_build(n, precision);
  // 6. only a length without any of these -- a prime, or a prime factor too large itself, with the nets switched off -- is
  //    refused, HERE, at plan time: offt_3d_init returns NULL instead of every execute failing
  if (no_direct && !four_lookup(n, precision, nullptr) && !long_lookup(n, precision, nullptr)) {
    snprintf(g_err, sizeof g_err, "no kernel for lines of %d %s points: no register kernel, the any-length kernel holds at most %zu, and %d has no "
             "factorisation n1 n2 into lengths that have one", n, precision == OFFT_PREC_F64 ? "double-complex" : "single-complex",
             LDS_BYTES / (2 * elem_size(precision)), n);
    return -1;
  }
  return 0;
}

int offt_hipk_fft_pass(const offt_pass_desc *d, const void *in, void *out, void *stream) {
  if (d->n < 1 || d->ncols < 1 || d->nb1 < 1 || d->nb2 < 1) return 0;  // empty batch: nothing to do
  if (d->n == 1 && d->scale == 1.0 && in == out && d->in_axis_stride == d->out_axis_stride &&
      d->in_col_stride == d->out_col_stride && d->in_b1_stride == d->out_b1_stride &&
      d->in_b2_stride == d->out_b2_stride)
    return 0;
  Tables tb;
  if (get_tables(d->n, d->precision, tb, false)) return -1;
  if (d->half) {
    // half lines run on their own kernels or not at all: no other route knows the bits, and none may run the full line
    Variant *h = pick_half(d);
    if (h && h->key.prec == OFFT_PREC_F32_PAIR && ((!d->in_contig && ((uintptr_t)in & 15)) || (!d->out_contig && ((uintptr_t)out & 15))))
      h = pick_half(d, false);  // a strided side off the 16-B grid: the one-column kernel
    if (!h) {
      snprintf(g_err, sizeof g_err, "offt_hipk_fft_pass: no half-line kernel for this descriptor (n=%d, half=%d, in_contig=%d, out_contig=%d)",
               d->n, d->half, d->in_contig, d->out_contig);
      return -1;
    }
    return launch_panel(d, in, out, tb, (hipStream_t)stream, h);
  }
  const Route r = resolve(d, in, out);
  if (drops_tw4(d, r)) { snprintf(g_err, sizeof g_err, "offt_hipk_fft_pass: no kernel with four-step twiddles for n=%d", d->n); return -1; }
  switch (r.via) {
    case Via::FourStep: return four_pass(d, in, out, stream, r.fs, tb);
    case Via::ScratchLines: return long_pass(d, in, out, stream, r.lt);
    case Via::Panel: return launch_panel(d, in, out, tb, (hipStream_t)stream, r.v);
    case Via::BluePanel: return launch_blue_panel(d, in, out, (hipStream_t)stream, r.bv, r.bt);
    case Via::AnyLength: return launch_any_length(d, in, out, tb, (hipStream_t)stream);
  }
  return -1;
}

// ---- two passes in one grid (offt_hipk.h) ----
namespace {
// the fft_pair_yx_k entry for (dy, dx), or nullptr; *vy, *vx: the entries the two descriptors resolve to on their own (dy with
// out_keep), whose bodies the pair entry must carry
Variant *pick_pair(const offt_pass_desc *dy, const void *iny, const void *outy, const offt_pass_desc *dx, const void *inx, const void *outx,
                   Variant **vy, Variant **vx) {
  if (!dy || !dx) return nullptr;
  auto plain = [](const offt_pass_desc *d) {
    return d->precision == OFFT_PREC_F64 && d->direction < 0 && d->n >= 1 && d->ncols >= 1 && d->nb1 >= 1 && d->nb2 >= 1 && !d->half && !d->real_input &&
           !d->tw4 && !d->in_split && !d->in_split_nfloor && !d->out_split && !d->out_split_nfloor && d->in_contig;
  };
  if (!plain(dy) || !plain(dx) || dy->out_contig || !dx->out_contig || dx->out_keep) return nullptr;
  offt_pass_desc ky = *dy;
  ky.out_keep = 1;
  const Route ry = resolve(&ky, iny, outy), rx = resolve(dx, inx, outx);
  if (ry.via != Via::Panel || rx.via != Via::Panel) return nullptr;
  auto body = [](const Variant *v, bool keep) { return v->key.role == Role::Plain && v->key.keep == keep && !v->mixed && !v->modfn; };
  if (!body(ry.v, true) || !body(rx.v, false)) return nullptr;
  Variant *p = find_variant(VariantKey{dy->n, OFFT_PREC_F64, true, false, Role::PairYX, true, 0}, dx->n);
  if (!p || p->id != dx->n) return nullptr;
  // (equal lengths only, so one shape: the elements per thread of both bodies are the entry's too)
  if (dy->n != dx->n || p->e != ry.v->e || p->e != rx.v->e || p->pair_y_id != ry.v->id || p->pair_x_id != rx.v->id || p->cols != ry.v->cols ||
      p->pair_x_cols != rx.v->cols || p->threads != ry.v->threads || p->threads != rx.v->threads || p->lds < ry.v->lds || p->lds < rx.v->lds)
    return nullptr;
  *vy = ry.v; *vx = rx.v;
  return p;
}

// the grid of a paired launch: workgroups per role, each role's XCD-aware order (that of a launch of its own), and the
// dispatch order of fft_pair_yx_k -- runs of 2^run_shift blocks alternate while both roles have a whole run left (blocks
// below 2 * both).  A run is a whole period of the x role's order (8 XCDs times G panels) unless OFFT_PAIR_RUN says otherwise
struct PairGrid { long long nyb, nxb; unsigned run_shift, both; };
PairGrid pair_grid(const offt_pass_desc *dy, const offt_pass_desc *dx, PassArgs *ay, PassArgs *ax) {
  PairGrid g;
  g.nyb = (long long)ay->ncp * dy->nb1 * dy->nb2;
  g.nxb = (long long)ax->ncp * dx->nb1 * dx->nb2;
  xcd_order(g.nyb, &ay->xcd_lim, &ay->xcd_gshift);
  xcd_order(g.nxb, &ax->xcd_lim, &ax->xcd_gshift);
  g.run_shift = 3u + (env().xcd_remap > 0 ? ax->xcd_gshift : 0u);
  if (env().pair_run >= 8 && is_pow2(env().pair_run)) g.run_shift = (unsigned)log2i(env().pair_run);
  const long long least = g.nxb < g.nyb ? g.nxb : g.nyb;
  g.both = (unsigned)((least >> g.run_shift) << g.run_shift);
  return g;
}
}  // namespace

int offt_hipk_has_pass_pair(const offt_pass_desc *dy, const offt_pass_desc *dx) {
  Variant *vy, *vx;
  return pick_pair(dy, nullptr, nullptr, dx, nullptr, nullptr, &vy, &vx) != nullptr;
}

const char *offt_hipk_pair_kernel_name(const offt_pass_desc *dy, const offt_pass_desc *dx) {
  Variant *vy, *vx;
  const Variant *p = pick_pair(dy, nullptr, nullptr, dx, nullptr, nullptr, &vy, &vx);
  return p ? p->kernel : "no paired kernel";
}

int offt_hipk_fft_pass_pair(const offt_pass_desc *dy, const void *iny, void *outy, const offt_pass_desc *dx, const void *inx, void *outx,
                            void *stream) {
  Variant *vy, *vx;
  Variant *p = pick_pair(dy, iny, outy, dx, inx, outx, &vy, &vx);
  if (!p || !iny || !outy || !inx || !outx) {
    snprintf(g_err, sizeof g_err, "offt_hipk_fft_pass_pair: no paired kernel for these descriptors (n=%d and n=%d)", dy ? dy->n : 0, dx ? dx->n : 0);
    return -1;
  }
  Tables ty, tx;
  if (get_tables(dy->n, dy->precision, ty, false) || get_tables(dx->n, dx->precision, tx, false)) return -1;
  PassArgs ay = pass_args(dy, p->cols), ax = pass_args(dx, p->pair_x_cols);
  PairGrid g = pair_grid(dy, dx, &ay, &ax);
  if (g.nyb + g.nxb > 0x7fffffffLL) { snprintf(g_err, sizeof g_err, "offt_hipk_fft_pass_pair: grid too large"); return -1; }
  unsigned nx = (unsigned)g.nxb;
  unsigned total_lim = 0, total_gshift = 0;  // (launch() works out the order of the whole grid: no role uses it)
  void *args[] = {(void *)&ay, (void *)&iny, (void *)&outy, (void *)&ty.full, (void *)&ax, (void *)&inx, (void *)&outx, (void *)&tx.full,
                  (void *)&nx, (void *)&g.both, (void *)&g.run_shift};
  return launch("offt_hipk_fft_pass_pair", p->fn, nullptr, &p->attr_set, p->lds, p->lds, p->threads, g.nyb + g.nxb, &total_lim, &total_gshift, args,
                (hipStream_t)stream);
}

int offt_hipk_pass_pair_grid(const offt_pass_desc *dy, const offt_pass_desc *dx, long long *ny_blocks, long long *nx_blocks, long long *both) {
  Variant *vy, *vx;
  const Variant *p = pick_pair(dy, nullptr, nullptr, dx, nullptr, nullptr, &vy, &vx);
  if (!p) return -1;
  PassArgs ay = pass_args(dy, p->cols), ax = pass_args(dx, p->pair_x_cols);
  const PairGrid g = pair_grid(dy, dx, &ay, &ax);
  if (ny_blocks) *ny_blocks = g.nyb;
  if (nx_blocks) *nx_blocks = g.nxb;
  if (both) *both = g.both;
  return 1 << g.run_shift;
}

int offt_hipk_panel_order(long long nblk, long long *lim) {
  unsigned l = 0, gshift = 0;
  xcd_order(nblk, &l, &gshift);
  if (lim) *lim = l;
  return env().xcd_remap > 0 ? 1 << gshift : 0;
}

int offt_hipk_any_length_threads(int n, int precision) {
  return n >= 1 && fits_any_length(n, precision) ? (int)mix_shape(n, precision).threads : 0;
}

}  // extern "C"

extern "C" {

// ---- flags of the direct-store exchange (offt_hipk.h) ----
namespace {
struct FlagArgs {
  unsigned long long *addr[OFFT_HIPK_MAX_FLAGS];
  int n;
  unsigned long long value;
  unsigned long long *status;
  long long timeout_ticks;  // of the 100 MHz constant clock (wall_clock64)
};
__global__ void __launch_bounds__(64) flag_signal_k(FlagArgs a) {
  const int i = threadIdx.x;
  // system scope: the word lives in a peer's memory (another GPU over xGMI, or another process's buffer on this one)
  if (i < a.n) __hip_atomic_store(a.addr[i], a.value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
__global__ void __launch_bounds__(64) flag_wait_k(FlagArgs a) {
  const int i = threadIdx.x;
  if (i < a.n) {
    const long long t0 = wall_clock64();
    // every lane polls its own word; the loop ends for every lane: the value arrives or the clock runs out
    while (__hip_atomic_load(a.addr[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) < a.value) {
      if (wall_clock64() - t0 > a.timeout_ticks) {
        if (a.status) __hip_atomic_store(a.status, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        break;
      }
      __builtin_amdgcn_s_sleep(64);
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");  // system scope; the next kernel's start-of-kernel acquire does the rest
}
int flag_launch(bool wait, int n, unsigned long long *const *addr, unsigned long long value, unsigned long long *status, double timeout_s,
                void *stream) {
  if (n < 0 || n > OFFT_HIPK_MAX_FLAGS) { snprintf(g_err, sizeof g_err, "offt_hipk_flag_%s: %d words (at most %d)", wait ? "wait" : "signal", n, OFFT_HIPK_MAX_FLAGS); return -1; }
  if (n == 0) return 0;
  FlagArgs a;
  for (int i = 0; i < OFFT_HIPK_MAX_FLAGS; i++) a.addr[i] = i < n ? addr[i] : nullptr;
  a.n = n; a.value = value; a.status = status;
  a.timeout_ticks = (long long)(timeout_s * 1e8);
  (void)hipGetLastError();
  if (wait) hipLaunchKernelGGL(flag_wait_k, dim3(1), dim3(64), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(flag_signal_k, dim3(1), dim3(64), 0, (hipStream_t)stream, a);
  HIPK_CHECK(hipGetLastError());
  return 0;
}
__global__ void __launch_bounds__(64) delay_k(long long ticks) {
  const long long t0 = wall_clock64();
  while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(64);
}
}  // namespace
// one wave that holds `stream` for `ms` milliseconds (100 MHz constant clock; at most 1 s): test builds put it in front of
// their passes to make the device lag behind the host (offt_host.c, OFFT_TEST_SLOW_PASS_MS)
int offt_hipk_delay(double ms, void *stream) {
  if (ms <= 0) return 0;
  if (ms > 1000.0) ms = 1000.0;
  (void)hipGetLastError();
  hipLaunchKernelGGL(delay_k, dim3(1), dim3(64), 0, (hipStream_t)stream, (long long)(ms * 1e5));
  HIPK_CHECK(hipGetLastError());
  return 0;
}

int offt_hipk_flag_signal(int n, unsigned long long *const *addr, unsigned long long value, void *stream) {
  return flag_launch(false, n, addr, value, nullptr, 0.0, stream);
}
int offt_hipk_flag_wait(int n, unsigned long long *const *addr, unsigned long long value, unsigned long long *status, double timeout_s,
                        void *stream) {
  return flag_launch(true, n, addr, value, status, timeout_s, stream);
}

// ---- spectral convolution (offt_hipk.h) ----
namespace {
// what every fused whole-line kernel asks of (d, f): contiguous complex lines without a split, a unit-stride filter axis
bool whole_lines(const offt_pass_desc *d, const offt_filter_desc *f) {
  if (!d || !f || (f->kind != OFFT_FILTER_REAL && f->kind != OFFT_FILTER_COMPLEX)) return false;
  if (d->precision != OFFT_PREC_F64 && d->precision != OFFT_PREC_F32) return false;
  return d->in_contig && d->in_axis_stride == 1 && !d->in_split && !d->in_split_nfloor && !d->real_input && !d->tw4 && f->axis_stride == 1;
}

// the fused instance for (fwd, f), or nullptr.  The mixed-radix instances (fft_conv_panelx_k; lengths that have no
// power-of-two instance) only with bit 1 of f->mixed.
// oop: the out-of-place instances (fft_conv_oop_panel_k): the power-of-two lengths, each with a cache-keeping twin, half
// lines included, and the mixed-radix ones (fft_conv_oop_panelx_k, no keeping twin) only with bits 1 and 2 of f->mixed.
Variant *pick_conv(const offt_pass_desc *d, const offt_filter_desc *f, bool keep, bool oop = false) {
  if (!whole_lines(d, f)) return nullptr;
  if (d->half && d->half != 3) return nullptr;  // half lines: loads and stores together, or not at all
  if (d->half && keep && !oop) return nullptr;  // (no cache-keeping twin of the in-place half-line kernels)
  Variant *v = find_variant(VariantKey{d->n, d->precision, true, true, oop ? Role::ConvOop : Role::Conv, keep, d->half});
  if (v && v->mixed && (oop ? (f->mixed & 3) != 3 : !(f->mixed & 7))) return nullptr;  // (bit 4 is the filtered launches' alone)
  return v;
}
const char *conv_kernel_name(const Variant *v) { return v ? v->kernel : "no fused kernel"; }

// the launch of a fused whole-line instance v picked for (d, f): every such kernel takes (a, f, <mid>, twq), `mid` being
// the nmid arguments that are its own
int line_launch(const char *who, Variant *v, const offt_pass_desc *d, const offt_filter_desc *f, void *const *mid, int nmid, void *stream) {
  if (d->ncols < 1 || d->nb1 < 1 || d->nb2 < 1) return 0;
  Tables tb;
  if (get_tables(d->n, d->precision, tb, false)) return -1;
  PassArgs a = pass_args(d, v->cols, true);
  ConvArgs fa;
  fa.axis = f->axis_stride; fa.col = f->col_stride; fa.b1 = f->b1_stride; fa.b2 = f->b2_stride;
  fa.cplx = f->kind == OFFT_FILTER_COMPLEX;
  void *args[6];
  int na = 0;
  args[na++] = (void *)&a; args[na++] = (void *)&fa;
  for (int i = 0; i < nmid; i++) args[na++] = mid[i];
  args[na++] = (void *)&tb.full;
  return launch(who, v->fn, nullptr, &v->attr_set, v->lds, v->lds, v->threads, (long long)a.ncp * d->nb1 * d->nb2, &a.xcd_lim, &a.xcd_gshift,
                args, (hipStream_t)stream);
}

// offt_hipk_conv_pass (src == dst, oop = false) and offt_hipk_conv_pass_oop: the out-of-place kernels take (a, f, src, dst,
// filter, twt), the in-place ones (a, f, data, filter, twt)
int conv_launch(const char *who, const offt_pass_desc *d, const offt_filter_desc *f, const void *filter, const void *src, void *dst, bool oop,
                void *stream) {
  Variant *v = pick_conv(d, f, d && d->out_keep, oop);
  if (!v && d && d->out_keep) v = pick_conv(d, f, false, oop);
  if (!v) {
    snprintf(g_err, sizeof g_err, "%s: no %sfused convolution kernel for this descriptor (n=%d)", who, oop ? "out-of-place " : "", d ? d->n : 0);
    return -1;
  }
  void *mid[3];
  int nmid = 0;
  if (oop) mid[nmid++] = (void *)&src;
  mid[nmid++] = (void *)&dst; mid[nmid++] = (void *)&filter;
  return line_launch(who, v, d, f, mid, nmid, stream);
}

// rows along the smallest stride, and the grid of the pointwise kernels over them
struct PointRows {
  int n[3];
  long long st[3];
  long long rows;
  PointRows(int n0, int n1, int n2, long long s0, long long s1, long long s2) : n{n0, n1, n2}, st{s0, s1, s2} {
    for (int a = 0; a < 2; a++)
      for (int b = 0; b < 2 - a; b++)
        if (st[b] < st[b + 1]) { int tn = n[b]; n[b] = n[b + 1]; n[b + 1] = tn; long long ts = st[b]; st[b] = st[b + 1]; st[b + 1] = ts; }
    rows = (long long)n[0] * n[1];
  }
  // two single-precision elements per lane: unit stride, whole pairs, 16-B aligned rows (and bases: the caller's test)
  bool pair_rows(int precision) const { return precision == OFFT_PREC_F32 && st[2] == 1 && !(n[2] & 1) && !(st[1] & 1) && !(st[0] & 1); }
  dim3 grid(bool pair) const { return dim3((unsigned)((n[2] / (pair ? 2 : 1) + 255) / 256), (unsigned)(rows < 65535 ? rows : 65535)); }
};

// offt_hipk_pointwise (in == out, oop = false) and offt_hipk_pointwise_oop: rows along the smallest stride, the pair test, the grid
int pointwise_launch(const char *who, const void *in, void *out, bool oop, const void *filter, int precision, int kind, int n0, int n1, int n2,
                     long long s0, long long s1, long long s2, void *stream) {
  if (kind != OFFT_FILTER_REAL && kind != OFFT_FILTER_COMPLEX) { snprintf(g_err, sizeof g_err, "%s: bad filter kind %d", who, kind); return -1; }
  if (oop && (!in || !out || in == out)) { snprintf(g_err, sizeof g_err, "%s: needs two different arrays (in place: offt_hipk_pointwise)", who); return -1; }
  if (n0 < 1 || n1 < 1 || n2 < 1) return 0;
  const PointRows r(n0, n1, n2, s0, s1, s2);
  const bool pair = r.pair_rows(precision) && !((uintptr_t)in & 15) && !((uintptr_t)out & 15) &&
                    !((uintptr_t)filter & (kind == OFFT_FILTER_COMPLEX ? 15 : 7));
  hipStream_t sm = (hipStream_t)stream;
  (void)hipGetLastError();
  const bool cx = kind == OFFT_FILTER_COMPLEX;
#define DISPATCH(LAUNCH)                                                             \
  do {                                                                               \
    if (pair) { if (cx) LAUNCH(float, true, 2); else LAUNCH(float, false, 2); }      \
    else if (cx) FOR_PREC(precision, LAUNCH(T, true, 1));                            \
    else FOR_PREC(precision, LAUNCH(T, false, 1));                                   \
  } while (0)
#define IN_PLACE(T, CPLX, EPL) \
  hipLaunchKernelGGL((pointwise_k<T, CPLX, EPL>), r.grid(pair), dim3(256), 0, sm, (typename vec2<T>::type *)out, filter, r.n[1], r.n[2], r.st[0], r.st[1], r.st[2], r.rows)
#define OUT_OF_PLACE(T, CPLX, EPL) \
  hipLaunchKernelGGL((pointwise_oop_k<T, CPLX, EPL>), r.grid(pair), dim3(256), 0, sm, (const typename vec2<T>::type *)in, (typename vec2<T>::type *)out, filter, r.n[1], r.n[2], r.st[0], r.st[1], r.st[2], r.rows)
  if (!oop) DISPATCH(IN_PLACE);
  else DISPATCH(OUT_OF_PLACE);
#undef OUT_OF_PLACE
#undef IN_PLACE
#undef DISPATCH
  HIPK_CHECK(hipGetLastError());
  return 0;
}

// the filtered-forward (inv = false) or filtered-inverse instance for (d, f), or nullptr: full lines.  The power-of-two
// lengths whatever f->mixed says; the mixed-radix instances (fft_filt_fwd_panelx_k, fft_filt_inv_panelx_k, no keeping twin)
// only with bit 4 of f->mixed, which stands alone: bits 1-3 mean nothing here
Variant *pick_filt(const offt_pass_desc *d, const offt_filter_desc *f, bool keep, bool inv) {
  if (!whole_lines(d, f) || d->half) return nullptr;
  Variant *v = find_variant(VariantKey{d->n, d->precision, true, true, inv ? Role::FiltInv : Role::FiltFwd, keep, 0});
  if (v && v->mixed && !(f->mixed & 8)) return nullptr;
  return v;
}

// offt_hipk_filt_pass_fwd (inv = false: (a, f, data, filter, twq)) and offt_hipk_filt_pass_inv ((a, f, src, dst, filter, twq))
int filt_launch(const char *who, const offt_pass_desc *d, const offt_filter_desc *f, const void *filter, const void *src, void *dst, bool inv,
                void *stream) {
  if (!filter || !src || !dst) { snprintf(g_err, sizeof g_err, "%s: a NULL array", who); return -1; }
  Variant *v = pick_filt(d, f, d && d->out_keep, inv);
  if (!v && d && d->out_keep) v = pick_filt(d, f, false, inv);
  if (!v) {
    snprintf(g_err, sizeof g_err, "%s: no filtered %s kernel for this descriptor (n=%d)", who, inv ? "inverse" : "forward", d ? d->n : 0);
    return -1;
  }
  void *mid[3];
  int nmid = 0;
  if (inv) mid[nmid++] = (void *)&src;
  mid[nmid++] = (void *)&dst; mid[nmid++] = (void *)&filter;
  return line_launch(who, v, d, f, mid, nmid, stream);
}

// the multi-input instance for (fwd, f), or nullptr.  The power-of-two lengths whatever f->mixed says; the mixed-radix
// instances (fft_conv_sum_panelx_k, no keeping twin) only with bits 1 and 3 of f->mixed both set
Variant *pick_conv_sum(const offt_pass_desc *d, const offt_filter_desc *f, bool keep) {
  if (!whole_lines(d, f)) return nullptr;
  if (d->half && d->half != 3) return nullptr;
  Variant *v = find_variant(VariantKey{d->n, d->precision, true, true, Role::ConvSum, keep, d->half});
  if (v && v->mixed && (f->mixed & 5) != 5) return nullptr;
  return v;
}

bool fill_sum_args(const char *who, SumArgs &sa, int nin, const void *const *srcs, const void *const *filters) {
  if (nin < 1 || nin > OFFT_CONV_SUM_MAX) { snprintf(g_err, sizeof g_err, "%s: nin = %d (1 ... %d inputs)", who, nin, OFFT_CONV_SUM_MAX); return false; }
  if (!srcs || !filters) { snprintf(g_err, sizeof g_err, "%s: needs the arrays of %d sources and filters (got NULL)", who, nin); return false; }
  memset(&sa, 0, sizeof sa);
  sa.nin = nin;
  for (int k = 0; k < nin; k++) {
    if (!srcs[k] || !filters[k]) { snprintf(g_err, sizeof g_err, "%s: source or filter %d is NULL", who, k); return false; }
    sa.src[k] = srcs[k]; sa.filter[k] = filters[k];
  }
  return true;
}

int pointwise_sum_launch(const char *who, int nin, const void *const *ins, const void *const *filters, void *out, int precision, int kind,
                         int n0, int n1, int n2, long long s0, long long s1, long long s2, void *stream) {
  if (kind != OFFT_FILTER_REAL && kind != OFFT_FILTER_COMPLEX) { snprintf(g_err, sizeof g_err, "%s: bad filter kind %d", who, kind); return -1; }
  if (precision != OFFT_PREC_F64 && precision != OFFT_PREC_F32) { snprintf(g_err, sizeof g_err, "%s: bad precision %d", who, precision); return -1; }
  SumArgs sa;
  if (!fill_sum_args(who, sa, nin, ins, filters)) return -1;
  if (!out) { snprintf(g_err, sizeof g_err, "%s: out is NULL", who); return -1; }
  if (n0 < 1 || n1 < 1 || n2 < 1) return 0;
  const PointRows r(n0, n1, n2, s0, s1, s2);
  bool pair = r.pair_rows(precision) && !((uintptr_t)out & 15);
  for (int k = 0; k < nin; k++)
    pair = pair && !((uintptr_t)ins[k] & 15) && !((uintptr_t)filters[k] & (kind == OFFT_FILTER_COMPLEX ? 15 : 7));
  hipStream_t sm = (hipStream_t)stream;
  (void)hipGetLastError();
  const bool cx = kind == OFFT_FILTER_COMPLEX;
#define SUM(T, CPLX, EPL) \
  hipLaunchKernelGGL((pointwise_sum_k<T, CPLX, EPL>), r.grid(pair), dim3(256), 0, sm, sa, (typename vec2<T>::type *)out, r.n[1], r.n[2], r.st[0], r.st[1], r.st[2], r.rows)
  if (pair) { if (cx) SUM(float, true, 2); else SUM(float, false, 2); }
  else if (cx) FOR_PREC(precision, SUM(T, true, 1));
  else FOR_PREC(precision, SUM(T, false, 1));
#undef SUM
  HIPK_CHECK(hipGetLastError());
  return 0;
}

// the product instance for d, or nullptr: strided complex lines without a split, half lines or four-step twiddles, loads
// and stores through the in_* side; the power-of-two lengths that have a spill-free instance
Variant *pick_prod(const offt_pass_desc *d) {
  if (!d || (d->precision != OFFT_PREC_F64 && d->precision != OFFT_PREC_F32)) return nullptr;
  if (d->in_contig || d->in_split || d->in_split_nfloor || d->real_input || d->half || d->tw4) return nullptr;
  return find_variant(VariantKey{d->n, d->precision, false, false, Role::Prod, false, 0});
}

// ... and the one for real fields held as half spectra: d is the real-output z pass of a complex-to-real inverse as it is
// (real_input = 2, n the real length, lines of n/2+1 complex values through the in_* side), strided, no split, no half box
Variant *pick_prod_real(const offt_pass_desc *d) {
  if (!d || (d->precision != OFFT_PREC_F64 && d->precision != OFFT_PREC_F32)) return nullptr;
  if (d->in_contig || d->in_split || d->in_split_nfloor || d->real_input != 2 || d->half || d->tw4) return nullptr;
  return find_variant(VariantKey{d->n, d->precision, false, false, Role::ProdReal, false, 0});
}

int pointwise_prod_launch(const char *who, const void *x, const void *y, void *out, int precision, int n0, int n1, int n2, long long s0,
                          long long s1, long long s2, void *stream) {
  const bool real = (precision & OFFT_HIPK_PROD_REAL) != 0;
  const int prec = precision & ~OFFT_HIPK_PROD_REAL;
  if (prec != OFFT_PREC_F64 && prec != OFFT_PREC_F32) { snprintf(g_err, sizeof g_err, "%s: bad precision %d", who, precision); return -1; }
  if (!x || !out) { snprintf(g_err, sizeof g_err, "%s: a NULL array", who); return -1; }
  if (!y) y = x;
  if (n0 < 1 || n1 < 1 || n2 < 1) return 0;
  const PointRows r(n0, n1, n2, s0, s1, s2);
  const bool aligned = !((uintptr_t)x & 15) && !((uintptr_t)y & 15) && !((uintptr_t)out & 15);
  // scalars per lane: 16 B where the rows are unit-stride runs of whole 16-B words on the 16-B grid, else one element
  int w = real ? 1 : 2;
  if (real) {
    const int full = prec == OFFT_PREC_F64 ? 2 : 4;
    if (aligned && r.st[2] == 1 && !(r.n[2] % full) && !(r.st[1] % full) && !(r.st[0] % full)) w = full;
  } else if (aligned && r.pair_rows(prec)) w = 4;
  const int epl = real ? w : w / 2;
  const dim3 grid((unsigned)((r.n[2] / epl + 255) / 256), (unsigned)(r.rows < 65535 ? r.rows : 65535));
  hipStream_t sm = (hipStream_t)stream;
  (void)hipGetLastError();
#define PROD(T, REAL, W) \
  hipLaunchKernelGGL((pointwise_prod_k<T, REAL, W>), grid, dim3(256), 0, sm, (const T *)x, (const T *)y, (T *)out, r.n[1], r.n[2], r.st[0], r.st[1], r.st[2], r.rows)
  if (prec == OFFT_PREC_F64) {
    if (!real) PROD(double, false, 2);
    else if (w == 2) PROD(double, true, 2);
    else PROD(double, true, 1);
  } else {
    if (!real) { if (w == 4) PROD(float, false, 4); else PROD(float, false, 2); }
    else if (w == 4) PROD(float, true, 4);
    else PROD(float, true, 1);
  }
#undef PROD
  HIPK_CHECK(hipGetLastError());
  return 0;
}

// ---- offt_hipk_spectrum_shells: the geometry of a call, worked out on the host ----
struct ShellGeom {
  ShellArgs sa;      // all but n2l and step, which depend on the elements per lane (shells_grid)
  int waves;         // waves per workgroup: as many of 4, 2, 1 as have their tables in 64 KiB of LDS
  size_t lds;        // ... and those tables' bytes
  long long rows;
};

// the host's copy of shell_of (the same clamp, the same integer decision)
int shell_of_host(unsigned long long k2) {
  const unsigned c = k2 < (1ull << 27) ? (unsigned)k2 : (1u << 27);
  const unsigned four = 4u * c;
  unsigned s = (unsigned)(std::sqrt((double)c) + 0.5);
  while ((2u * s + 1u) * (2u * s + 1u) <= four) ++s;
  while (s > 0u && (2u * s - 1u) * (2u * s - 1u) > four) --s;
  return (int)s;
}

// false with g_err set: arguments the sweep cannot take.  start may be NULL (zeros), kmul may be NULL (ones).
bool shells_geom(const char *who, int precision, int r2c, const int n[3], const long long st[3], const int start[3], const int N[3],
                 const int kmul[3], int nbins, ShellGeom &g) {
  if (precision != OFFT_PREC_F64 && precision != OFFT_PREC_F32) { snprintf(g_err, sizeof g_err, "%s: bad precision %d", who, precision); return false; }
  if (nbins < 1 || nbins > OFFT_HIPK_SHELLS_MAX_BINS) {
    snprintf(g_err, sizeof g_err, "%s: nbins = %d (1 ... %d)", who, nbins, OFFT_HIPK_SHELLS_MAX_BINS);
    return false;
  }
  if (!n || !N) { snprintf(g_err, sizeof g_err, "%s: needs the box and the global extents (got NULL)", who); return false; }
  memset(&g, 0, sizeof g);
  int order[3] = {0, 1, 2};   // by falling stride, PointRows' sort
  if (st)
    for (int a = 0; a < 2; a++)
      for (int b = 0; b < 2 - a; b++)
        if (st[order[b]] < st[order[b + 1]]) std::swap(order[b], order[b + 1]);
  ShellArgs &sa = g.sa;
  sa.zaxis = -1;
  unsigned long long k2max = 0;
  for (int i = 0; i < 3; i++) {
    const int ax = order[i], km = kmul ? kmul[ax] : 1, s0 = start ? start[ax] : 0;
    const bool halved = r2c && ax == 2;
    if (km < 1) { snprintf(g_err, sizeof g_err, "%s: kmul[%d] = %d (multipliers are >= 1)", who, ax, km); return false; }
    if (N[ax] < 1 || n[ax] < 0 || s0 < 0 || (long long)s0 + n[ax] > (halved ? N[ax] / 2 + 1 : N[ax])) {
      snprintf(g_err, sizeof g_err, "%s: axis %d: block %d + %d outside the spectrum of %d points", who, ax, s0, n[ax], N[ax]);
      return false;
    }
    const long long q = (long long)km * (N[ax] / 2);
    if (q > (1ll << 30)) { snprintf(g_err, sizeof g_err, "%s: kmul[%d] * N/2 = %lld is above 2^30", who, ax, q); return false; }
    k2max += (unsigned long long)(q * q);
    sa.n[i] = n[ax]; sa.st[i] = st ? st[ax] : 0; sa.g0[i] = s0; sa.N[i] = N[ax]; sa.km[i] = km;
    if (halved) { sa.zaxis = i; sa.Nz = N[ax]; }
  }
  g.rows = (long long)sa.n[0] * sa.n[1];
  if (g.rows >= (1ll << 30)) { snprintf(g_err, sizeof g_err, "%s: %lld rows (below 2^30)", who, g.rows); return false; }
  const int top = shell_of_host(k2max) + 1;
  sa.nb = nbins < top ? nbins : top;
  g.waves = (size_t)sa.nb * 36 <= 65536 ? 4 : (size_t)sa.nb * 20 <= 65536 ? 2 : 1;
  g.lds = (size_t)sa.nb * (8 * (size_t)g.waves + 4);
  return true;
}

// workgroups of the sweep with `epl` elements per lane (0 for an empty box); fills sa.n2l and sa.step.  Enough workgroups
// to fill the device, no more partials than 32 MiB (256 workgroups whatever they take).
int shells_grid(ShellGeom &g, int epl) {
  ShellArgs &sa = g.sa;
  if (g.rows < 1 || sa.n[2] < 1) return 0;
  sa.n2l = sa.n[2] / epl;
  const long long chunks = (g.rows * sa.n2l + 63) / 64, want = (chunks + g.waves - 1) / g.waves;
  long long cap = (32ll << 20) / ((long long)sa.nb * 12);
  if (cap < 256) cap = 256;
  if (cap > 8192 / g.waves) cap = 8192 / g.waves;
  const int nwg = (int)(want < cap ? want : cap);
  const long long stride = (long long)nwg * g.waves * 64, r = stride / sa.n2l;
  sa.step[2] = (int)(stride % sa.n2l); sa.step[1] = (int)(r % sa.n[1]); sa.step[0] = (int)(r / sa.n[1]);
  return nwg;
}
}  // namespace

long long offt_hipk_spectrum_shells_partials(int precision, const int n[3], const int N[3], const int kmul[3], int nbins) {
  ShellGeom g;
  if (!shells_geom("offt_hipk_spectrum_shells_partials", precision, 0, n, nullptr, nullptr, N, kmul, nbins, g)) return 0;
  return (long long)shells_grid(g, 1) * g.sa.nb * 12;   // one element per lane: the larger grid of the two
}

int offt_hipk_spectrum_shells(const void *a, const void *b, int precision, int r2c, const int n[3], const long long stride[3], const int start[3],
                              const int N[3], const int kmul[3], int nbins, double *sums, long long *counts, void *partials,
                              long long partials_bytes, void *stream) {
  const char *who = "offt_hipk_spectrum_shells";
  ShellGeom g;
  if (!stride) { snprintf(g_err, sizeof g_err, "%s: needs the strides (got NULL)", who); return -1; }
  if (!shells_geom(who, precision, r2c, n, stride, start, N, kmul, nbins, g)) return -1;
  if (!sums) { snprintf(g_err, sizeof g_err, "%s: sums is NULL", who); return -1; }
  ShellArgs &sa = g.sa;
  const bool empty = g.rows < 1 || sa.n[2] < 1;
  if (!empty && !a) { snprintf(g_err, sizeof g_err, "%s: the spectrum is NULL", who); return -1; }
  const PointRows pr(sa.n[0], sa.n[1], sa.n[2], sa.st[0], sa.st[1], sa.st[2]);
  const bool pair = !empty && pr.pair_rows(precision) && !((uintptr_t)a & 15) && !((uintptr_t)b & 15);
  const int nwg = shells_grid(g, pair ? 2 : 1);
  const long long need = (long long)nwg * sa.nb * 12;
  if (need > partials_bytes || (need && !partials)) {
    snprintf(g_err, sizeof g_err, "%s: %lld bytes of partials, %lld needed (offt_hipk_spectrum_shells_partials)", who, partials ? partials_bytes : 0ll, need);
    return -1;
  }
  sa.with_counts = counts != nullptr;
  double *psum = (double *)partials;
  unsigned *pcnt = (unsigned *)(psum + (size_t)nwg * sa.nb);
  hipStream_t sm = (hipStream_t)stream;
  (void)hipGetLastError();
  if (nwg) {
#define SWEEP(T, CROSS, EPL) \
  hipLaunchKernelGGL((shells_sweep_k<T, CROSS, EPL>), dim3((unsigned)nwg), dim3(64 * g.waves), g.lds, sm, sa, (const typename vec2<T>::type *)a, (const typename vec2<T>::type *)b, psum, pcnt)
    const bool cross = b != nullptr && b != a;
    if (pair) { if (cross) SWEEP(float, true, 2); else SWEEP(float, false, 2); }
    else if (cross) FOR_PREC(precision, SWEEP(T, true, 1));
    else FOR_PREC(precision, SWEEP(T, false, 1));
#undef SWEEP
    HIPK_CHECK(hipGetLastError());
  }
  hipLaunchKernelGGL(shells_combine_k, dim3((unsigned)((nbins + 7) / 8)), dim3(256), 0, sm, psum, pcnt, nwg, sa.nb, nbins, sums, counts);
  HIPK_CHECK(hipGetLastError());
  return 0;
}

int offt_hipk_conv_has_fused(const offt_pass_desc *fwd, const offt_filter_desc *f) { return pick_conv(fwd, f, false) != nullptr; }
const char *offt_hipk_conv_kernel_name(const offt_pass_desc *fwd, const offt_filter_desc *f) { return conv_kernel_name(pick_conv(fwd, f, false)); }
int offt_hipk_conv_pass(const offt_pass_desc *d, const offt_filter_desc *f, const void *filter, void *data, void *stream) {
  return conv_launch("offt_hipk_conv_pass", d, f, filter, data, data, false, stream);
}

int offt_hipk_conv_has_fused_oop(const offt_pass_desc *fwd, const offt_filter_desc *f) { return pick_conv(fwd, f, false, true) != nullptr; }
const char *offt_hipk_conv_oop_kernel_name(const offt_pass_desc *fwd, const offt_filter_desc *f) {
  return conv_kernel_name(pick_conv(fwd, f, false, true));
}
int offt_hipk_conv_pass_oop(const offt_pass_desc *d, const offt_filter_desc *f, const void *filter, const void *src, void *dst, void *stream) {
  if (!src || !dst || src == dst) {
    snprintf(g_err, sizeof g_err, "offt_hipk_conv_pass_oop: needs two different arrays (src == dst is offt_hipk_conv_pass)");
    return -1;
  }
  return conv_launch("offt_hipk_conv_pass_oop", d, f, filter, src, dst, true, stream);
}

int offt_hipk_pointwise(void *data, const void *filter, int precision, int kind, int n0, int n1, int n2, long long s0, long long s1,
                        long long s2, void *stream) {
  return pointwise_launch("offt_hipk_pointwise", data, data, false, filter, precision, kind, n0, n1, n2, s0, s1, s2, stream);
}

int offt_hipk_pointwise_oop(const void *in, void *out, const void *filter, int precision, int kind, int n0, int n1, int n2, long long s0,
                            long long s1, long long s2, void *stream) {
  return pointwise_launch("offt_hipk_pointwise_oop", in, out, true, filter, precision, kind, n0, n1, n2, s0, s1, s2, stream);
}

// ---- filtered forward and filtered inverse (offt_hipk.h) ----
int offt_hipk_filt_has_fused(const offt_pass_desc *d, const offt_filter_desc *f) {
  return pick_filt(d, f, false, false) != nullptr && pick_filt(d, f, false, true) != nullptr;
}
const char *offt_hipk_filt_fwd_kernel_name(const offt_pass_desc *d, const offt_filter_desc *f) { return conv_kernel_name(pick_filt(d, f, false, false)); }
const char *offt_hipk_filt_inv_kernel_name(const offt_pass_desc *d, const offt_filter_desc *f) { return conv_kernel_name(pick_filt(d, f, false, true)); }
int offt_hipk_filt_pass_fwd(const offt_pass_desc *d, const offt_filter_desc *f, const void *filter, void *data, void *stream) {
  return filt_launch("offt_hipk_filt_pass_fwd", d, f, filter, data, data, false, stream);
}
int offt_hipk_filt_pass_inv(const offt_pass_desc *d, const offt_filter_desc *f, const void *filter, const void *src, void *dst, void *stream) {
  return filt_launch("offt_hipk_filt_pass_inv", d, f, filter, src, dst, true, stream);
}

// ---- multi-input convolution (offt_hipk.h) ----
int offt_hipk_conv_has_fused_sum(const offt_pass_desc *fwd, const offt_filter_desc *f) { return pick_conv_sum(fwd, f, false) != nullptr; }
const char *offt_hipk_conv_sum_kernel_name(const offt_pass_desc *fwd, const offt_filter_desc *f) {
  return conv_kernel_name(pick_conv_sum(fwd, f, false));
}
int offt_hipk_conv_pass_sum(const offt_pass_desc *d, const offt_filter_desc *f, int nin, const void *const *filters, const void *const *srcs,
                            void *dst, void *stream) {
  const char *who = "offt_hipk_conv_pass_sum";
  SumArgs sa;
  if (!fill_sum_args(who, sa, nin, srcs, filters)) return -1;
  if (!dst) { snprintf(g_err, sizeof g_err, "%s: dst is NULL", who); return -1; }
  Variant *v = pick_conv_sum(d, f, d && d->out_keep);
  if (!v && d && d->out_keep) v = pick_conv_sum(d, f, false);
  if (!v) {
    snprintf(g_err, sizeof g_err, "%s: no multi-input fused convolution kernel for this descriptor (n=%d)", who, d ? d->n : 0);
    return -1;
  }
  void *mid[2] = {(void *)&sa, (void *)&dst};
  return line_launch(who, v, d, f, mid, 2, stream);
}

int offt_hipk_pointwise_sum(int nin, const void *const *ins, const void *const *filters, void *out, int precision, int kind, int n0, int n1,
                            int n2, long long s0, long long s1, long long s2, void *stream) {
  return pointwise_sum_launch("offt_hipk_pointwise_sum", nin, ins, filters, out, precision, kind, n0, n1, n2, s0, s1, s2, stream);
}

// ---- pseudo-spectral product (offt_hipk.h) ----
int offt_hipk_prod_has_fused(const offt_pass_desc *d) { return pick_prod(d) != nullptr; }
const char *offt_hipk_prod_kernel_name(const offt_pass_desc *d) { return conv_kernel_name(pick_prod(d)); }
int offt_hipk_prod_pass(const offt_pass_desc *d, const void *src0, const void *src1, void *dst, void *stream) {
  const char *who = "offt_hipk_prod_pass";
  if (!src0 || !dst) { snprintf(g_err, sizeof g_err, "%s: a NULL array", who); return -1; }
  Variant *v = pick_prod(d);
  if (!v) { snprintf(g_err, sizeof g_err, "%s: no fused product kernel for this descriptor (n=%d)", who, d ? d->n : 0); return -1; }
  if (src1 == src0) src1 = nullptr;  // the square: one load, one inverse
  if (d->ncols < 1 || d->nb1 < 1 || d->nb2 < 1) return 0;
  Tables tb;
  if (get_tables(d->n, d->precision, tb, false)) return -1;
  PassArgs a = pass_args(d, v->cols, true);  // loads and stores through the in_* side, no split
  void *args[] = {(void *)&a, (void *)&src0, (void *)&src1, (void *)&dst, (void *)&tb.full};
  return launch(who, v->fn, nullptr, &v->attr_set, v->lds, v->lds, v->threads, (long long)a.ncp * d->nb1 * d->nb2, &a.xcd_lim, &a.xcd_gshift,
                args, (hipStream_t)stream);
}

int offt_hipk_prod_real_has_fused(const offt_pass_desc *d) { return pick_prod_real(d) != nullptr; }
const char *offt_hipk_prod_real_kernel_name(const offt_pass_desc *d) { return conv_kernel_name(pick_prod_real(d)); }
int offt_hipk_prod_real_pass(const offt_pass_desc *d, const void *src0, const void *src1, void *dst, void *stream) {
  const char *who = "offt_hipk_prod_real_pass";
  if (!src0 || !dst) { snprintf(g_err, sizeof g_err, "%s: a NULL array", who); return -1; }
  Variant *v = pick_prod_real(d);
  if (!v) { snprintf(g_err, sizeof g_err, "%s: no fused real product kernel for this descriptor (n=%d)", who, d ? d->n : 0); return -1; }
  if (src1 == src0) src1 = nullptr;  // the square: one load, one inverse
  if (d->ncols < 1 || d->nb1 < 1 || d->nb2 < 1) return 0;
  Tables tb;
  if (get_tables(d->n, d->precision, tb, false)) return -1;
  PassArgs a = pass_args(d, v->cols, true);  // loads and stores through the in_* side, no split
  void *args[] = {(void *)&a, (void *)&src0, (void *)&src1, (void *)&dst, (void *)&tb.full};
  return launch(who, v->fn, nullptr, &v->attr_set, v->lds, v->lds, v->threads, (long long)a.ncp * d->nb1 * d->nb2, &a.xcd_lim, &a.xcd_gshift,
                args, (hipStream_t)stream);
}

int offt_hipk_pointwise_prod(const void *x, const void *y, void *out, int precision, int n0, int n1, int n2, long long s0, long long s1,
                             long long s2, void *stream) {
  return pointwise_prod_launch("offt_hipk_pointwise_prod", x, y, out, precision, n0, n1, n2, s0, s1, s2, stream);
}

int offt_hipk_zero_outside(void *buf, int precision, int n0, int n1, int n2, int k0, int k1, int k2, long long s0, long long s1,
                           long long s2, void *stream) {
  const bool real = (precision & OFFT_HIPK_ZERO_REAL) != 0;
  const int prec = precision & ~OFFT_HIPK_ZERO_REAL;
  if (prec != OFFT_PREC_F64 && prec != OFFT_PREC_F32) { snprintf(g_err, sizeof g_err, "offt_hipk_zero_outside: bad precision %d", precision); return -1; }
  if (n0 < 1 || n1 < 1 || n2 < 1) return 0;
  if (k0 < 0 || k1 < 0 || k2 < 0 || k0 > n0 || k1 > n1 || k2 > n2) { snprintf(g_err, sizeof g_err, "offt_hipk_zero_outside: kept box outside the block"); return -1; }
  if (k0 == n0 && k1 == n1 && k2 == n2) return 0;
  const size_t ssz = prec == OFFT_PREC_F64 ? 8 : 4;
  const int spe = real ? 1 : 2;                      // scalars per element
  const int w = 16 / (int)ssz;                       // scalars per 16-B store
  // 16 B per lane: unit-stride rows that start on the 16-B grid (every row: base and the two outer strides)
  const bool vec = s2 == 1 && !((uintptr_t)buf & 15) && !((s0 * spe) % w) && !((s1 * spe) % w);
  const long long rows = (long long)n0 * n1;
  const long long per_row = vec ? ((long long)n2 * spe + w - 1) / w : n2;
  const unsigned gx = (unsigned)((per_row + 255) / 256);
  const unsigned gy = (unsigned)(rows < 65535 ? rows : 65535);
  hipStream_t sm = (hipStream_t)stream;
  (void)hipGetLastError();
#define ZERO_OUT(S, SPE, VEC) \
  hipLaunchKernelGGL((zero_outside_k<S, SPE, VEC>), dim3(gx, gy), dim3(256), 0, sm, (S *)buf, n1, n2, k0, k1, k2, s0, s1, s2, rows)
  if (prec == OFFT_PREC_F64) {
    if (real) { if (vec) ZERO_OUT(double, 1, true); else ZERO_OUT(double, 1, false); }
    else { if (vec) ZERO_OUT(double, 2, true); else ZERO_OUT(double, 2, false); }
  } else {
    if (real) { if (vec) ZERO_OUT(float, 1, true); else ZERO_OUT(float, 1, false); }
    else { if (vec) ZERO_OUT(float, 2, true); else ZERO_OUT(float, 2, false); }
  }
#undef ZERO_OUT
  HIPK_CHECK(hipGetLastError());
  return 0;
}

int offt_hipk_copy3d(const void *in, void *out, int precision, int n0, int n1, int n2, long long is0,
                     long long is1, long long is2, long long os0, long long os1, long long os2, void *stream) {
  long long total = (long long)n0 * n1 * n2;
  if (total <= 0) return 0;
  long long nb = (total + 255) / 256;
  if (nb > 256 * 64) nb = 256 * 64;
  FOR_PREC(precision, hipLaunchKernelGGL(copy3d_k<V2>, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, (const V2 *)in, (V2 *)out, n0, n1, n2,
                                         is0, is1, is2, os0, os1, os2));
  HIPK_CHECK(hipGetLastError());
  return 0;
}

int offt_hipk_fill(void *buf, int precision, int kind, int n0, int n1, int n2, int s0, int s1, int s2,
                   long long st0, long long st1, long long st2, void *stream) {
  long long total = (long long)n0 * n1 * n2;
  if (total <= 0) return 0;
  long long nb = (total + 255) / 256;
  if (nb > 256 * 64) nb = 256 * 64;
  if (precision & 0x100)  // real-valued field (r2c input), strides in scalars
    FOR_PREC(precision & 0xff, hipLaunchKernelGGL(fill_real_k<T>, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, (T *)buf, kind, n0, n1, n2,
                                                  s0, s1, s2, st0, st1, st2));
  else
    FOR_PREC(precision, hipLaunchKernelGGL(fill_k<V2>, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, (V2 *)buf, kind, n0, n1, n2,
                                           s0, s1, s2, st0, st1, st2));
  HIPK_CHECK(hipGetLastError());
  return 0;
}

}  // extern "C"
