// bayesnmf_amd/csrc/mixing.h — mixing diagnostics of a recorded range: for every element of the renormalised P and E, over the used
// samples of the record_sample rings, the mean and variance, Geyer's effective sample size, the Monte-Carlo standard error of the mean,
// split R-hat and the per-half moments from which a between-chain R-hat is combined on the host (bnmf_mixing / bnmf_mixing_at;
// DESIGN.md §13).  Reads the rings after the fact, as k_map_quant does; no sweep kernel is involved.
//
// Per element, over the used samples s = 0 .. S-1, oldest first (a lag counts used samples; a gapped used[] is one contiguous series).
// canon(v_0 .. v_{m-1}) is the canonical W = 64 sum: accumulator l adds v_l, v_{l+64}, ... ascending from +0.0, then wave_tree64.
//   x_s    = P_s[k,n] / cs_s[n]  (SIDE 0)   or   E_s[n,g] * cs_s[n]  (SIDE 1),  cs = k_map_colsum: the expressions of k_map_stats
//   mu     = canon(x) / S,  d_s = x_s - mu,  q0 = canon(d_s * d_s),  var = q0 / (S - 1),  gamma0 = q0 / S
//   h = S / 2; half a = samples 0 .. h-1, half b = samples S-h .. S-1:  mean_a = canon(x_a) / h,  var_a = canon((x - mean_a)^2) / (h - 1)
//   W = (var_a + var_b) * 0.5,  mb = (mean_a + mean_b) * 0.5,  Bn = (mean_a - mb)^2 + (mean_b - mb)^2,
//   vp = W * ((double)(h - 1) / (double)h) + Bn,  rhat = dsqrt(vp / W), NaN if !(W > 0)
//   degenerate: !(gamma0 > 0) (a NaN, an underflow), or every x_s == x_0 (a constant series: canon(x) / S need not round back to x_0, so
//     gamma0 alone would let rounding noise through):  ess = mcse = rhat = NaN, pairs = 0, exit = 0; mean, var and the half moments are written
//   rho_t  = (canon_{s = 0 .. S-1-t}(d_s * d_{s+t}) / S) / gamma0
//   Gamma_0 = rho_0 + rho_1, sum = Gamma_0;  for m = 1, 2, ... while 2m + 1 <= S - 2:  Gamma_m = rho_{2m} + rho_{2m+1};
//     !(Gamma_m > 0): stop, exit = 0;  else Gamma_m = min(Gamma_m, Gamma_{m-1}), sum = sum + Gamma_m;  out of lags: exit = 1
//   tau = 2 * sum - 1,  tau = tau < tau_min ? tau_min : tau  (tau_min = 1 / log10(S), from the host),  ess = S / tau,  mcse = dsqrt(var / ess)
// Only + - * / and dsqrt, associated as written: the bits depend on this alone, not on the tiling below.
//
// Tiling.  An element's series is a stride-len gather in the ring, so a workgroup takes MX_E (8, 4, 2 or 1: as many as fit the LDS at
// this S) consecutive elements — at 8 one 64-byte line per sample — with the slot list in the LDS, renormalises them and lays them out
// [element][S] there.  A wavefront then owns one element: lane l holds the canonical accumulator l of every sum, so for a lag the two
// streams d[s] and d[s + t] are stride-1 across the lanes (no bank conflict), and every stop decision is taken on a value all lanes hold
// (no divergence inside a wave).  No atomics, no waits.  A series that does not fit the LDS alone is refused by the host
// (mixing_max_samples), never truncated.
#pragma once
#include "kernels.h"

namespace bnmf {

constexpr int MX_EMAX = 8;           // elements of a workgroup at most: one wavefront each
constexpr int MX_NROW = 11;          // rows of the per-element output (BNMF_NMIX)
constexpr size_t MX_LDS = 160 * 1024;
inline size_t mixing_lds_bytes(int epw, int S) { return (size_t)epw * (size_t)S * sizeof(double) + (size_t)S * sizeof(int); }
inline int mixing_max_samples() { return (int)(MX_LDS / (sizeof(double) + sizeof(int))); }
inline int mixing_elements_per_group(int S) {   // 8, 4, 2, 1: the most whose series fit the LDS; 0: not even one
  for (int e = MX_EMAX; e >= 1; e >>= 1) if (mixing_lds_bytes(e, S) <= MX_LDS) return e;
  return 0;
}

// lane l's accumulator of canon_{s = 0 .. m-1}(a[s] * b[s])
BNMF_DEV double mx_dot_lane(const double* a, const double* b, int m, int lane) {
  double acc = 0.0;
#pragma unroll 4
  for (int s = lane; s < m; s += 64) acc = acc + a[s] * b[s];
  return acc;
}
// lane l's accumulators of canon(a[0 .. m-1]) and, given c, of canon((a - c)^2)
BNMF_DEV double mx_sum_lane(const double* a, int m, int lane) {
  double acc = 0.0;
#pragma unroll 4
  for (int s = lane; s < m; s += 64) acc = acc + a[s];
  return acc;
}
BNMF_DEV double mx_sq_lane(const double* a, double c, int m, int lane) {
  double acc = 0.0;
#pragma unroll 4
  for (int s = lane; s < m; s += 64) { const double d = a[s] - c; acc = acc + d * d; }
  return acc;
}
BNMF_DEV double mx_all(double lane_acc) { return wave_bcast0(wave_tree64(lane_acc)); }   // the canonical sum, in every lane

template <int SIDE>
__global__ __launch_bounds__(64 * MX_EMAX) void k_mixing(const double* ring, size_t len, int K, int N, const int* slots, int S, const double* cs,
                                                          double tau_min, int epw, double* out /* [MX_NROW][len] */) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  double* tile = (double*)smem;                            // [epw][S]
  int* sl = (int*)(tile + (size_t)epw * S);                // [S] ring slots of the samples
  const int tid = (int)threadIdx.x, nt = 64 * epw, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const size_t e0 = (size_t)blockIdx.x * (size_t)epw;
  for (int s = tid; s < S; s += nt) sl[s] = slots[s];
  __syncthreads();
  {
    const int j = tid % epw, sb = tid / epw;               // element j, samples sb, sb + 64, ...
    const size_t ec = min(e0 + (size_t)j, len - 1);        // (a wave past the end stages the last element and writes nothing)
    const int n = SIDE ? (int)(ec % (size_t)N) : (int)(ec / (size_t)K);
    constexpr int B = 8;
    for (int s0 = sb; s0 < S; s0 += 64 * B) {
      double v[B], c[B];
#pragma unroll
      for (int b = 0; b < B; ++b) {                        // every load is made (no branch around it): 8 lines in flight
        const int sc = min(s0 + 64 * b, S - 1);
        v[b] = ring[(size_t)sl[sc] * len + ec];
        c[b] = cs[(size_t)sc * N + n];
      }
#pragma unroll
      for (int b = 0; b < B; ++b) {
        const int s = s0 + 64 * b;
        if (s < S) tile[(size_t)j * S + s] = SIDE ? v[b] * c[b] : v[b] / c[b];
      }
    }
  }
  __syncthreads();
  const size_t e = e0 + (size_t)wave;
  if (e >= len) return;                                    // wave-uniform; no barrier follows
  double* x = tile + (size_t)wave * S;
  const double dS = (double)S, NaN = __builtin_nan("");
  const int h = S / 2;
  const double dh = (double)h, dh1 = (double)(h - 1);
  // the moments of the series and of its halves, while x is intact
  const double mu = mx_all(mx_sum_lane(x, S, lane)) / dS;
  const double mean_a = mx_all(mx_sum_lane(x, h, lane)) / dh, mean_b = mx_all(mx_sum_lane(x + (S - h), h, lane)) / dh;
  const double var_a = mx_all(mx_sq_lane(x, mean_a, h, lane)) / dh1, var_b = mx_all(mx_sq_lane(x + (S - h), mean_b, h, lane)) / dh1;
  int same = 1;                                            // a constant series: every sample equal to the first (false for a NaN)
  { const double x0 = x[0]; for (int s = lane; s < S; s += 64) same &= x[s] == x0 ? 1 : 0; }
  const int constant = __all(same);
  wave_lds_fence();                                        // half b is read at another lane offset: those reads come first
  double acc = 0.0;
  for (int s = lane; s < S; s += 64) { const double d = x[s] - mu; x[s] = d; acc = acc + d * d; }
  const double q0 = mx_all(acc);
  const double var = q0 / (double)(S - 1), gamma0 = q0 / dS;
  wave_lds_fence();                                        // d[] of every lane is visible to the wave
  double ess = NaN, mcse = NaN, rhat = NaN, pairs = 0.0, ex = 0.0;
  if (__builtin_amdgcn_readfirstlane(gamma0 > 0.0 && !constant ? 1 : 0)) {   // (the same value in every lane)
    const double Wv = (var_a + var_b) * 0.5, mb = (mean_a + mean_b) * 0.5;
    const double Bn = (mean_a - mb) * (mean_a - mb) + (mean_b - mb) * (mean_b - mb);
    const double vp = Wv * (dh1 / dh) + Bn;
    if (Wv > 0.0) rhat = dsqrt(vp / Wv);
    const double rho0 = (q0 / dS) / gamma0;
    const double rho1 = (mx_all(mx_dot_lane(x, x + 1, S - 1, lane)) / dS) / gamma0;
    double Gp = rho0 + rho1, sum = Gp;
    int np = 1, ran_out = 1;
    for (int m = 1; 2 * m + 1 <= S - 2; ++m) {
      const int t = 2 * m;
      const double a0 = mx_dot_lane(x, x + t, S - t, lane), a1 = mx_dot_lane(x, x + t + 1, S - t - 1, lane);
      const double r0 = (mx_all(a0) / dS) / gamma0, r1 = (mx_all(a1) / dS) / gamma0;
      double Gm = r0 + r1;
      if (!__builtin_amdgcn_readfirstlane(Gm > 0.0 ? 1 : 0)) { ran_out = 0; break; }
      Gm = Gm < Gp ? Gm : Gp;
      sum = sum + Gm;
      Gp = Gm; ++np;
    }
    double tau = 2.0 * sum - 1.0;
    tau = tau < tau_min ? tau_min : tau;
    ess = dS / tau;
    mcse = dsqrt(var / ess);
    pairs = (double)np; ex = (double)ran_out;
  }
  if (lane == 0) {
    const double r[MX_NROW] = {mu, var, ess, mcse, rhat, pairs, ex, mean_a, var_a, mean_b, var_b};
#pragma unroll
    for (int q = 0; q < MX_NROW; ++q) out[(size_t)q * len + e] = r[q];
  }
}

}  // namespace bnmf
