// bayesnmf_amd/csrc/contrast.h — group contrasts of exposures over a recorded range: for every used sample of the record_sample rings
// and every group of tumours the group's mean load, mean share and prevalence per factor, on the device (bnmf_contrast /
// bnmf_contrast_at).  Reads the rings after the fact, as k_attr and k_mixing do; no sweep kernel is involved and none of
// the chain's streams is consumed.
//
// Per used sample s (oldest first), tumour g and factor n, with cs_s[n] the bits of k_map_colsum:
//   x[n,g] = A_s[n] != 0 ? E_s[n,g] * cs_s[n] : +0.0       bnmf_map's renormalised exposure; an excluded factor is +0.0 in every sum
//   t = sum_n x[n,g]    n ascending from +0.0;   u = t > 0 ? 1 / t : 0.0;   r = x * u;   b = (x >= min_load)
// Per group c with members g_0 < g_1 < ... (m_c of them) and factor n, in the canonical W = 64 order over the members (accumulator l
// adds members l, l + 64, ... ascending from +0.0, then wave_tree64):
//   v0 = canon64_i(x[n,g_i]) / m_c     v1 = canon64_i(r) / m_c     v2 = #(b) / m_c     out[q][s][n + N c] = v_q
// The statistics over s and the pairs are the host's (posterior.h).
//
// Tiling: one wavefront per (group, sample): lane l IS accumulator l and walks members l, l + 64, ... of the group's member list (built
// on the host), so the order of step 4 is the order of the loop.  A member's column E_s[., g] is N contiguous doubles; adjacent tumours
// are adjacent in memory, so a wave of adjacent members reads one contiguous run.  A lane's accumulator is one sequential chain of
// additions: splitting a group's members over waves would re-associate it and change the bits, so a long group is one wave's work and
// the parallelism is over the S C (group, sample) units and, in the tiled form, the factor tiles.
//   REG form  (N <= TN, TN = 8, 16, 24, 32): the column is loaded once, x and the 3 N accumulators stay in registers.
//   tiled form (any N; BNMF_CON_FORM=1 forces it): blockIdx.z is a tile of CT_TN = 8 factors; t is summed over all N from the column, the
//   tile's x are read again (the line is in the L1).  The same operations on the same values in the same order: the same bits.
#pragma once
#include "dmath.h"

namespace bnmf {

constexpr int CT_TN = 8;          // factors of a tile of the tiled form
constexpr int CT_MAX_REG = 32;    // most factors of the REG form
constexpr int CT_NSTAT = 3;       // statistics: load, share, prevalence
struct ConArgs {
  const double *ringE, *ringA;    // record_sample rings: [slot][N*G], [slot][N]
  const double* cs;               // [S][N]: k_map_colsum
  const int* slots;               // ring slots of the used samples, oldest first
  const int* members;             // the tumours of group 0, then of group 1, ...: ascending inside a group
  const int* goff;                // [C + 1]: group c is members[goff[c] .. goff[c + 1])
  double* out;                    // [3][S][N*C]
  size_t lenE; int N, C, S; double min_load;
};

template <int TN, bool REG>
__global__ __launch_bounds__(64) void k_contrast(ConArgs a) {
  const int lane = (int)threadIdx.x, c = (int)blockIdx.x, s = (int)blockIdx.y, N = a.N;
  const int n0 = REG ? 0 : (int)blockIdx.z * TN;
  const double* Es = a.ringE + (size_t)a.slots[s] * a.lenE;
  const double* As = a.ringA + (size_t)a.slots[s] * (size_t)N;
  const double* cs = a.cs + (size_t)s * N;
  const int m0 = a.goff[c], m1 = a.goff[c + 1];
  double f[TN];                                    // the tile's factors: cs where the sample includes the factor; 0 with inc false
  bool inc[TN];
#pragma unroll
  for (int t = 0; t < TN; ++t) { const int n = min(n0 + t, N - 1); inc[t] = As[n] != 0.0; f[t] = cs[n]; }
  double ax[TN], ar[TN]; int ab[TN];
#pragma unroll
  for (int t = 0; t < TN; ++t) { ax[t] = 0.0; ar[t] = 0.0; ab[t] = 0; }
  for (int i = m0 + lane; i < m1; i += 64) {
    const double* col = Es + (size_t)N * (size_t)a.members[i];
    double x[TN], tot = 0.0;
    if constexpr (REG) {
#pragma unroll
      for (int t = 0; t < TN; ++t) x[t] = inc[t] ? col[min(t, N - 1)] * f[t] : 0.0;
#pragma unroll
      for (int t = 0; t < TN; ++t) if (t < N) tot = tot + x[t];
    } else {
      for (int n = 0; n < N; ++n) tot = tot + (As[n] != 0.0 ? col[n] * cs[n] : 0.0);
#pragma unroll
      for (int t = 0; t < TN; ++t) x[t] = inc[t] ? col[min(n0 + t, N - 1)] * f[t] : 0.0;
    }
    const double u = tot > 0.0 ? 1.0 / tot : 0.0;
#pragma unroll
    for (int t = 0; t < TN; ++t) {
      ax[t] = ax[t] + x[t];
      ar[t] = ar[t] + x[t] * u;
      ab[t] += x[t] >= a.min_load ? 1 : 0;
    }
  }
  const double dm = (double)(m1 - m0);
  const size_t SNC = (size_t)a.S * N * a.C;
  double* o = a.out + (size_t)s * N * a.C + (size_t)N * c;
#pragma unroll
  for (int t = 0; t < TN; ++t) {
    if (n0 + t >= N) continue;                     // wave-uniform
    const double v0 = wave_tree64(ax[t]), v1 = wave_tree64(ar[t]), v2 = wave_tree64((double)ab[t]);   // the count: whole numbers, exact
    if (lane == 0) { o[n0 + t] = v0 / dm; o[SNC + n0 + t] = v1 / dm; o[2 * SNC + n0 + t] = v2 / dm; }
  }
}

}  // namespace bnmf
