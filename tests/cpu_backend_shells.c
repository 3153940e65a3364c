/*
 * cpu_backend_shells.c -- TEST INFRASTRUCTURE ONLY.
 *
 * The CPU backend chain up to cpu_backend_spec.c (whose logging entries stay in place) with the spectrum_shells entry
 * filled: plain loops over the strided box, the integer shell rule of include/offt_hip.h decided without any square root,
 * sequential double sums.  Every call of the entry is counted, so that the tests can tell a refusal (nothing launched)
 * from a run.  `partials` is ignored: there are no workgroups here.
 * Built into tests/libcpubackend_shells.so (tests/test_spectrum_shells.py), never into the library.
 */
#include <string.h>
#include "offt_backend.h"

const offt_backend *cpu_backend_spec_table(void);

static offt_backend g_shells;
static long g_calls = 0;

/* the s with (2s-1)^2 <= 4 k2 < (2s+1)^2; shells from `limit` on are all the same to the caller */
static int shell_of(unsigned long long k2, int limit) {
  int s = 0;
  while (s < limit && (2ull * s + 1) * (2ull * s + 1) <= 4 * k2) s++;
  return s;
}

static long long signed_k(int g, int N) { return 2 * g <= N ? g : g - N; }

static int shells(const void *a, const void *b, int precision, int r2c, const int n[3], const long long stride[3], const int start[3],
                  const int N[3], const int kmul[3], int nbins, double *sums, long long *counts, void *partials, long long partials_bytes,
                  void *stream) {
  (void)partials; (void)partials_bytes; (void)stream;
  g_calls++;
  if (!sums || nbins < 1) return -1;
  const int f32 = precision == OFFT_PREC_F32;
  if (!b) b = a;
  for (int s = 0; s < nbins; s++) { sums[s] = 0.0; if (counts) counts[s] = 0; }
  for (int i0 = 0; i0 < n[0]; i0++)
    for (int i1 = 0; i1 < n[1]; i1++)
      for (int i2 = 0; i2 < n[2]; i2++) {
        const int g[3] = {i0 + (start ? start[0] : 0), i1 + (start ? start[1] : 0), i2 + (start ? start[2] : 0)};
        unsigned long long k2 = 0;
        for (int d = 0; d < 3; d++) {
          const long long q = (kmul ? kmul[d] : 1) * signed_k(g[d], N[d]);
          k2 += (unsigned long long)(q * q);
        }
        const int s = shell_of(k2, nbins);
        if (s >= nbins) continue;
        const long long o = i0 * stride[0] + i1 * stride[1] + i2 * stride[2];
        double ar, ai, br, bi;
        if (f32) { ar = ((const float *)a)[2 * o]; ai = ((const float *)a)[2 * o + 1]; br = ((const float *)b)[2 * o]; bi = ((const float *)b)[2 * o + 1]; }
        else { ar = ((const double *)a)[2 * o]; ai = ((const double *)a)[2 * o + 1]; br = ((const double *)b)[2 * o]; bi = ((const double *)b)[2 * o + 1]; }
        const int w = r2c && g[2] > 0 && 2 * g[2] != N[2] ? 2 : 1;
        sums[s] += (double)w * (ar * br + ai * bi);
        if (counts) counts[s] += w;
      }
  return 0;
}

const offt_backend *cpu_backend_shells_table(void) {
  g_shells = *cpu_backend_spec_table();
  g_shells.spectrum_shells = shells;
  return &g_shells;
}
long cpu_backend_shells_calls(void) { return g_calls; }
