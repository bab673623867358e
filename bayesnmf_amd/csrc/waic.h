// bayesnmf_amd/csrc/waic.h — WAIC of a recorded range: the pointwise predictive density of every cell (k, g) of the data over the
// used samples of the record_sample rings, on the device (bnmf_waic / bnmf_waic_at).  Reads the rings after the fact,
// as k_map_fit does; no sweep kernel is involved.
//
// Per cell, over the used samples s = 1..S, oldest first:
//   c_s   = sum_n (P_s[k,n] * A_s[n]) * E_s[n,g]            n ascending from +0.0, associated as written (k_map_fit's c)
//   l_s   = ((double)m * dlog(mh) - mh) - lgfact[m], mh = max(c_s, 1e-6)           Poisson (the cell term of colterms.h)
//         = (-log(sqrt(2 pi)) - dlog(sd)) - 0.5 * (z * z), sd = dsqrt(sigmasq_s[g]), z = (m - c_s) / sd    Normal (dnorm_log_sd)
//   running maximum a (from -inf) and r (from 0):  l_s > a ? (r = r * dexp(a - l_s) + 1, a = l_s) : (r = r + dexp(l_s - a))
//   Welford:  d = l_s - mu;  mu = mu + d * (1 / s);  M2 = M2 + d * (l_s - mu)
//   lppd = a + dlog(r / S),  p = M2 / (S - 1),  mean = mu,  elpd = lppd - p
// Per column, the sums over k of lppd, p, mean, elpd, elpd^2 and of (p > 0.4) in the canonical W = 64 order: accumulator l adds
// rows l, l + 64, ... from +0.0, then wave_tree64.  The bits depend on nothing else: not on the tiling below.
//
// Tiling.  A workgroup is 4 wavefronts and owns WA_GC = 8 adjacent columns, 2 per wavefront; lane = row.  The rows go in chunks of
// WA_CH = 128 (two 64-row passes: 4 statistics x 2 passes x 2 columns stay in registers); for every chunk the workgroup loops over the
// samples once, so a column's E_s[, g] is read once per chunk: once per call up to K = 128.  The lane's six column accumulators run
// across the chunks (rows ascending), which keeps the canonical order for any K.  Per sample the workgroup stages the chunk of
// P_s diag(A_s) ([n][row], conflict-free for lane = row) and its 8 columns of E_s (contiguous in the ring) in the LDS; every E value
// is then an LDS broadcast read.  Where the stage does not fit the LDS (160 KB: N > 150) the lanes read P, A and E through the caches instead:
// the same operations on the same values.  All samples of a cell are visited by one lane in order: no atomics, no split.
#pragma once
#include "dmath.h"

namespace bnmf {

constexpr int WA_T = 256, WA_CW = 2, WA_RP = 2, WA_CH = 64 * WA_RP, WA_GC = (WA_T / 64) * WA_CW;
constexpr int WA_NCOL = 6;   // per-column outputs: lppd, p, mean, elpd, elpd^2, cells with p > 0.4
struct WaicArgs {
  const double *ringP, *ringE, *ringA, *ringS;   // record_sample rings: [slot][K*N], [slot][N*G], [slot][N], [slot][G] (Normal)
  const int32_t* M; const double* Mf;            // the data: counts (Poisson) or fp64 (Normal), column-major K x G
  const double* lgfact; const int* slots;        // lgamma(m + 1) table; ring slots of the used samples, oldest first
  double *col /* [WA_NCOL][G] */, *cell /* [2][K*G]: lppd, p; may be null */;
  size_t lenP, lenE; int K, N, G, S, maxM, stage;
};
inline size_t waic_lds_bytes(int N) { return ((size_t)N * WA_CH + (size_t)N * WA_GC) * sizeof(double); }

template <bool NORMAL>
__global__ __launch_bounds__(WA_T) void k_waic(WaicArgs a) {
  extern __shared__ double wa_lds[];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int K = a.K, N = a.N, G = a.G, S = a.S;
  const int gb = (int)blockIdx.x * WA_GC;
  const int ncw = min(WA_GC, G - gb);              // columns of this workgroup that exist (>= 1 by the grid)
  double* pa = wa_lds;                             // [N][WA_CH]  P_s diag(A_s), rows of the chunk
  double* es = wa_lds + (size_t)N * WA_CH;         // [ncw][N]    E_s[, gb ..]
  int jl[WA_CW], gc[WA_CW]; bool gok[WA_CW];
#pragma unroll
  for (int j = 0; j < WA_CW; ++j) { const int q = wave * WA_CW + j; gok[j] = q < ncw; jl[j] = gok[j] ? q : ncw - 1; gc[j] = gb + jl[j]; }
  double acc[WA_CW][WA_NCOL];
#pragma unroll
  for (int j = 0; j < WA_CW; ++j)
#pragma unroll
    for (int q = 0; q < WA_NCOL; ++q) acc[j][q] = 0.0;
  const double dS = (double)S, dS1 = (double)(S - 1);

  for (int k0 = 0; k0 < K; k0 += WA_CH) {
    double md[WA_CW][WA_RP], lgf[WA_CW][WA_RP];
    double sa[WA_CW][WA_RP], sr[WA_CW][WA_RP], mu[WA_CW][WA_RP], m2[WA_CW][WA_RP];
#pragma unroll
    for (int j = 0; j < WA_CW; ++j)
#pragma unroll
      for (int p = 0; p < WA_RP; ++p) {
        const int k = min(k0 + p * 64 + lane, K - 1);
        const size_t at = (size_t)k + (size_t)K * (size_t)gc[j];
        if constexpr (NORMAL) { md[j][p] = a.Mf[at]; lgf[j][p] = 0.0; }
        else { const int m = a.M[at]; md[j][p] = (double)m; lgf[j][p] = a.lgfact[m < 0 ? 0 : (m > a.maxM ? a.maxM : m)]; }
        sa[j][p] = -BNMF_INF; sr[j][p] = 0.0; mu[j][p] = 0.0; m2[j][p] = 0.0;
      }
    for (int s = 0; s < S; ++s) {
      const size_t slot = (size_t)a.slots[s];
      const double* Ps = a.ringP + slot * a.lenP;
      const double* Es = a.ringE + slot * a.lenE;
      const double* As = a.ringA + slot * (size_t)N;
      if (a.stage) {
        __syncthreads();                           // the previous sample's reads of the stage are done
        for (int e = tid; e < N * WA_CH; e += WA_T) {
          const int r = e & (WA_CH - 1), n = e / WA_CH, k = k0 + r;
          pa[e] = k < K ? Ps[(size_t)k + (size_t)K * n] * As[n] : 0.0;
        }
        for (int e = tid; e < ncw * N; e += WA_T) es[e] = Es[(size_t)N * gb + e];
        __syncthreads();
      }
      const double rs = 1.0 / (double)(s + 1);
#pragma unroll
      for (int j = 0; j < WA_CW; ++j) {
        double sd = 1.0, lsd = 0.0;
        if constexpr (NORMAL) { sd = dsqrt(a.ringS[slot * (size_t)G + gc[j]]); lsd = dlog(sd); }
#pragma unroll
        for (int p = 0; p < WA_RP; ++p) {
          double c = 0.0;
          if (a.stage) {
            const double* pr = pa + p * 64 + lane;
            const double* er = es + (size_t)jl[j] * N;
            for (int n = 0; n < N; ++n) c = c + pr[(size_t)n * WA_CH] * er[n];
          } else {
            const int k = min(k0 + p * 64 + lane, K - 1);
            const double* er = Es + (size_t)N * gc[j];
            for (int n = 0; n < N; ++n) c = c + (Ps[(size_t)k + (size_t)K * n] * As[n]) * er[n];
          }
          double l;
          if constexpr (NORMAL) {
            const double z = (md[j][p] - c) / sd;
            l = (-0.91893853320467274178 - lsd) - 0.5 * (z * z);
          } else {
            const double mh = c < 1e-6 ? 1e-6 : c;
            l = (md[j][p] * dlog(mh) - mh) - lgf[j][p];
          }
          const bool up = l > sa[j][p];
          const double ex = dexp(up ? sa[j][p] - l : l - sa[j][p]);
          sr[j][p] = up ? sr[j][p] * ex + 1.0 : sr[j][p] + ex;
          sa[j][p] = up ? l : sa[j][p];
          const double d = l - mu[j][p];
          mu[j][p] = mu[j][p] + d * rs;
          m2[j][p] = m2[j][p] + d * (l - mu[j][p]);
        }
      }
    }
#pragma unroll
    for (int p = 0; p < WA_RP; ++p) {
      const int k = k0 + p * 64 + lane;
      if (k < K) {
#pragma unroll
        for (int j = 0; j < WA_CW; ++j) {
          const double lppd = sa[j][p] + dlog(sr[j][p] / dS);
          const double pk = m2[j][p] / dS1;
          const double elpd = lppd - pk;
          acc[j][0] = acc[j][0] + lppd; acc[j][1] = acc[j][1] + pk; acc[j][2] = acc[j][2] + mu[j][p];
          acc[j][3] = acc[j][3] + elpd; acc[j][4] = acc[j][4] + elpd * elpd; acc[j][5] = acc[j][5] + (pk > 0.4 ? 1.0 : 0.0);
          if (a.cell && gok[j]) {
            const size_t at = (size_t)k + (size_t)K * (size_t)gc[j];
            a.cell[at] = lppd; a.cell[(size_t)K * (size_t)G + at] = pk;
          }
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < WA_CW; ++j)
#pragma unroll
    for (int q = 0; q < WA_NCOL; ++q) {
      const double r = wave_tree64(acc[j][q]);
      if (lane == 0 && gok[j]) a.col[(size_t)q * G + gc[j]] = r;
    }
}

}  // namespace bnmf
