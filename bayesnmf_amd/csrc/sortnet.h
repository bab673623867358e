// bayesnmf_amd/csrc/sortnet.h — the workgroup's sort of doubles in the LDS and the two searches of a sorted run, shared by the rank
// transform of bnmf_coactivity (coactivity.h) and the order statistics of bnmf_summary (summary.h).
#pragma once
#include "dmath.h"

namespace bnmf {

// bitonic sort of key[0 .. n2) ascending, n2 a power of two, by the whole workgroup.  The compare-exchange network touches fixed places
// whatever the keys hold (a NaN only leaves the order undefined; its factor is flagged and its ranks are not used).
template <int NT>
BNMF_DEV void coa_bitonic(double* key, int n2, int tid) {
  for (int k = 2; k <= n2; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < (n2 >> 1); t += NT) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
        const bool up = (i & k) == 0;
        const double p = key[i], q = key[i + j];
        if ((p > q) == up) { key[i] = q; key[i + j] = p; }
      }
      __syncthreads();
    }
}
// #(key < x) and #(key <= x) of the ascending key[0 .. n): every probe lies inside [0, n)
BNMF_DEV int coa_lower(const double* key, int n, double x) {
  int lo = 0;
  while (n > 0) { const int h = n >> 1; if (key[lo + h] < x) { lo += h + 1; n -= h + 1; } else n = h; }
  return lo;
}
BNMF_DEV int coa_upper(const double* key, int n, double x) {
  int lo = 0;
  while (n > 0) { const int h = n >> 1; if (key[lo + h] <= x) { lo += h + 1; n -= h + 1; } else n = h; }
  return lo;
}
BNMF_DEV bool coa_finite(double x) { return dabs(x) < BNMF_INF; }   // false for NaN

}  // namespace bnmf
