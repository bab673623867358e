// bayesnmf_amd/csrc/attribution.h — signature attribution of a recorded range: for every used sample of the record_sample rings the
// expected allocation of every cell of the data to the factors, summed per tumour and factor and averaged per cell, on the device
// (bnmf_attribution / bnmf_attribution_at).  Reads the rings after the fact, as k_waic and k_ppc do; no sweep kernel is
// involved and none of the chain's streams is consumed.
//
// Per cell (k, g) and factor n, over the used samples s = 1..S, oldest first:
//   f_n   = (P_s[k,n] * A_s[n]) * E_s[n,g]
//   c     = sum_n f_n                                      n ascending from +0.0 (waic.h's c_s, the same bits)
//   q     = c > 0 ? 1 / c : 0.0;   r_n = f_n * q           the share of factor n in the cell: one division per cell and sample, no clip
//   x_n   = m * r_n                                        Poisson: E[Z_kng | M, P_s, E_s], the multinomial mean (m the count as a double)
//         = f_n                                            Normal: the component of the fit (real-valued data are not allocated)
//   prob[k + K (n + N g)] = (sum_s r_n) / S                s ascending from +0.0, then one division
// Per tumour g, factor n and sample s:
//   a_s[n,g] = sum_k x_n   rows in chunks of 128; inside a chunk the canonical W = 64 order (accumulator l adds rows l, l + 64 of the
//              chunk from +0.0, then wave_tree64); the first chunk's sum, then + the next chunk's, ascending (ppc.h's order)
//   t = sum_n a_s[n,g]     n ascending from +0.0;   u = t > 0 ? 1 / t : 0.0;   share = a_s[n,g] * u
// Over s ascending, per (n, g):  Welford  d = a - mu; mu = mu + d * (1 / s); M2 = M2 + d * (a - mu);  sum of share from +0.0;  the count
// of a >= min_load.  load rows: 0 mu, 1 M2 / (S - 1), 2 sum share / S, 3 count / S (the probability that the signature is present).
// series[s][n] = canon(a_s[n, .], W = 1024) over g (block_tree<1024>'s order).  The bits depend on nothing else: not on the tiling, not on
// the batch size below.
//
// The identity of factor n over the samples is the assumption bnmf_map makes too (it averages P and E element-wise): on a chain whose
// labels switch inside the range the per-factor rows mix signatures, as the MAP does.
//
// Tiling: k_waic's.  A workgroup is 4 wavefronts and owns AT_GC = 8 adjacent columns, 2 per wavefront; lane = row; row chunks of
// AT_CH = 128 (two 64-row passes).  Per sample the workgroup stages the chunk of P_s diag(A_s) and its 8 columns of E_s in the LDS between
// two barriers; beyond 160 KB (N > 150) the lanes read P, A and E through the caches: the same operations on the same values.  With prob
// asked for, the sums of r_n stay in registers for a tile of AT_TN factors, the factor tiles loop outside the sample loop and c is
// recomputed in full for every tile; without it no per-cell state exists and one pass over the samples serves every factor.  One
// wave_tree64 per (sample, column, factor) leaves a_s[n,g] in the scratch: chunk 0 writes, a later chunk adds to what the same lane
// wrote.  The samples go in batches so that the scratch stays under a cap; k_attr_share then gives u per (s, g), and k_attr_stats
// continues the per-(n, g) statistics from the previous batch in sample order and reduces the series.
#pragma once
#include "dmath.h"

namespace bnmf {

constexpr int AT_T = 256, AT_CW = 2, AT_RP = 2, AT_CH = 64 * AT_RP, AT_GC = (AT_T / 64) * AT_CW;
constexpr int AT_TN = 8;         // factors whose sums of r_n stay in registers (prob asked for)
constexpr int AT_TT = 1024;      // threads of k_attr_stats: the W of the sums over g
constexpr int AT_NLOAD = 4;      // load rows: mean, variance, mean share, probability of presence
struct AttrArgs {
  const double *ringP, *ringE, *ringA;           // record_sample rings: [slot][K*N], [slot][N*G], [slot][N]
  const int32_t* M;                              // the counts (Poisson), column-major K x G
  const int* slots;                              // ring slots of the batch's samples, oldest first
  double *scr /* [Sb][N][G]: a_s */, *prob /* [K*N*G]: running sums of r_n, the mean after the last batch */;
  size_t lenP, lenE; int K, N, G, S /* all used samples */, Sb /* samples of the batch */, first /* the batch starts the range */,
      last /* ... ends it */, stage;
};
inline size_t attr_lds_bytes(int N) { return ((size_t)N * AT_CH + (size_t)N * AT_GC) * sizeof(double); }

template <bool NORMAL, bool PROB>
__global__ __launch_bounds__(AT_T) void k_attr(AttrArgs a) {
  extern __shared__ double at_lds[];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int K = a.K, N = a.N, G = a.G, Sb = a.Sb;
  const int gb = (int)blockIdx.x * AT_GC;
  const int ncw = min(AT_GC, G - gb);              // columns of this workgroup that exist (>= 1 by the grid)
  double* pa = at_lds;                             // [N][AT_CH]  P_s diag(A_s), rows of the chunk
  double* es = at_lds + (size_t)N * AT_CH;         // [ncw][N]    E_s[, gb ..]
  int jl[AT_CW], gc[AT_CW]; bool gok[AT_CW];
#pragma unroll
  for (int j = 0; j < AT_CW; ++j) { const int q = wave * AT_CW + j; gok[j] = q < ncw; jl[j] = gok[j] ? q : ncw - 1; gc[j] = gb + jl[j]; }
  const double dS = (double)a.S;
  const int TN = PROB ? AT_TN : N;                 // without prob one tile holds every factor

  for (int k0 = 0; k0 < K; k0 += AT_CH) {
    double md[AT_CW][AT_RP];
    bool kok[AT_RP];
    int kr[AT_RP];
#pragma unroll
    for (int p = 0; p < AT_RP; ++p) { kok[p] = k0 + p * 64 + lane < K; kr[p] = min(k0 + p * 64 + lane, K - 1); }
#pragma unroll
    for (int j = 0; j < AT_CW; ++j)
#pragma unroll
      for (int p = 0; p < AT_RP; ++p) {
        if constexpr (NORMAL) md[j][p] = 1.0;
        else md[j][p] = (double)a.M[(size_t)kr[p] + (size_t)K * (size_t)gc[j]];
      }
    for (int n0 = 0; n0 < N; n0 += TN) {
      double acc[AT_CW][AT_RP][PROB ? AT_TN : 1];
      if constexpr (PROB) {
#pragma unroll
        for (int j = 0; j < AT_CW; ++j)
#pragma unroll
          for (int p = 0; p < AT_RP; ++p)
#pragma unroll
            for (int t = 0; t < AT_TN; ++t) {
              const int n = min(n0 + t, N - 1);
              acc[j][p][t] = a.first ? 0.0 : a.prob[(size_t)kr[p] + (size_t)K * ((size_t)n + (size_t)N * (size_t)gc[j])];
            }
      }
      for (int s = 0; s < Sb; ++s) {
        const size_t slot = (size_t)a.slots[s];
        const double* Ps = a.ringP + slot * a.lenP;
        const double* Es = a.ringE + slot * a.lenE;
        const double* As = a.ringA + slot * (size_t)N;
        if (a.stage) {
          __syncthreads();                         // the previous sample's reads of the stage are done
          for (int e = tid; e < N * AT_CH; e += AT_T) {
            const int r = e & (AT_CH - 1), n = e / AT_CH, k = k0 + r;
            pa[e] = k < K ? Ps[(size_t)k + (size_t)K * n] * As[n] : 0.0;
          }
          for (int e = tid; e < ncw * N; e += AT_T) es[e] = Es[(size_t)N * gb + e];
          __syncthreads();
        }
#pragma unroll
        for (int j = 0; j < AT_CW; ++j) {
          if (!gok[j]) continue;                   // wave-uniform: the wave has no such column
          const double* er = a.stage ? es + (size_t)jl[j] * N : Es + (size_t)N * gc[j];
          double q[AT_RP];
#pragma unroll
          for (int p = 0; p < AT_RP; ++p) {
            double c = 0.0;
            if (a.stage) {
              const double* pr = pa + p * 64 + lane;
              for (int n = 0; n < N; ++n) c = c + pr[(size_t)n * AT_CH] * er[n];
            } else {
              for (int n = 0; n < N; ++n) c = c + (Ps[(size_t)kr[p] + (size_t)K * n] * As[n]) * er[n];
            }
            q[p] = c > 0.0 ? 1.0 / c : 0.0;
          }
          double* ap = a.scr + ((size_t)s * (size_t)N) * (size_t)G + (size_t)gc[j];
          auto factor = [&](int n, int t) {        // t: the factor's place in the tile (prob only)
            double xs = 0.0;
#pragma unroll
            for (int p = 0; p < AT_RP; ++p) {
              const double f = a.stage ? pa[(size_t)n * AT_CH + p * 64 + lane] * er[n] : (Ps[(size_t)kr[p] + (size_t)K * n] * As[n]) * er[n];
              const double r = f * q[p];
              if constexpr (PROB) acc[j][p][t] = acc[j][p][t] + r;
              const double x = NORMAL ? f : md[j][p] * r;
              if (kok[p]) xs = xs + x;
            }
            const double v = wave_tree64(xs);
            if (lane == 0) {
              double* o = ap + (size_t)n * (size_t)G;
              if (k0 == 0) *o = v; else *o = *o + v;
            }
          };
          if constexpr (PROB) {
#pragma unroll
            for (int t = 0; t < AT_TN; ++t) if (n0 + t < N) factor(n0 + t, t);
          } else {
            for (int n = 0; n < N; ++n) factor(n, 0);
          }
        }
      }
      if constexpr (PROB) {
#pragma unroll
        for (int j = 0; j < AT_CW; ++j)
#pragma unroll
          for (int p = 0; p < AT_RP; ++p)
#pragma unroll
            for (int t = 0; t < AT_TN; ++t)
              if (gok[j] && kok[p] && n0 + t < N)
                a.prob[(size_t)kr[p] + (size_t)K * ((size_t)(n0 + t) + (size_t)N * (size_t)gc[j])] = a.last ? acc[j][p][t] / dS : acc[j][p][t];
      }
    }
  }
}

// u[s][g] = 1 / sum_n a_s[n,g] (0.0 where the sum is not positive): a thread per (s, g) of the batch
__global__ __launch_bounds__(256) void k_attr_share(const double* scr, int Sb, int N, int G, double* u /* [Sb][G] */) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)Sb * (size_t)G) return;
  const size_t s = i / (size_t)G, g = i % (size_t)G;
  const double* x = scr + s * (size_t)N * (size_t)G + g;
  double t = 0.0;
  for (int n = 0; n < N; ++n) t = t + x[(size_t)n * G];
  u[i] = t > 0.0 ? 1.0 / t : 0.0;
}

// Blocks 0 .. Sb N - 1: block s N + n reduces a_s[n, .] over g (series[s0 + s][n]).  The blocks after them: a thread per (n, g) continues
// the statistics st[4][N*G] (mu, M2, sum of share, count; indexed g + G n as the scratch) over the batch's samples; the last batch also
// writes the load rows, laid out as E.
__global__ __launch_bounds__(AT_TT) void k_attr_stats(const double* scr, const double* u, int Sb, int N, int G, int S, int s0, int last,
                                                      double min_load, double* st, double* series /* [S][N] */, double* load /* [4][N*G] */) {
  __shared__ double buf[AT_TT];
  const int tid = (int)threadIdx.x, b = (int)blockIdx.x;
  if (b < Sb * N) {                                // block-uniform
    const double* x = scr + (size_t)b * (size_t)G;
    double acc = 0.0;
    for (int g = tid; g < G; g += AT_TT) acc = acc + x[g];
    const double r = block_tree<AT_TT>(acc, buf, tid);
    if (tid == 0) series[(size_t)s0 * N + b] = r;
    return;
  }
  const size_t NG = (size_t)N * (size_t)G, e = (size_t)(b - Sb * N) * AT_TT + tid;
  if (e >= NG) return;
  const size_t n = e / (size_t)G, g = e % (size_t)G;
  double mu = 0.0, m2 = 0.0, sh = 0.0, cnt = 0.0;
  if (s0 > 0) { mu = st[e]; m2 = st[NG + e]; sh = st[2 * NG + e]; cnt = st[3 * NG + e]; }
  for (int s = 0; s < Sb; ++s) {
    const double av = scr[(size_t)s * NG + e];
    const double rs = 1.0 / (double)(s0 + s + 1);
    const double d = av - mu;
    mu = mu + d * rs;
    m2 = m2 + d * (av - mu);
    sh = sh + av * u[(size_t)s * G + g];
    cnt = cnt + (av >= min_load ? 1.0 : 0.0);      // a whole number below 2^53: exact
  }
  st[e] = mu; st[NG + e] = m2; st[2 * NG + e] = sh; st[3 * NG + e] = cnt;
  if (last) {
    const double dS = (double)S, dS1 = (double)(S - 1);
    const size_t o = n + (size_t)N * g;
    load[o] = mu; load[NG + o] = m2 / dS1; load[2 * NG + o] = sh / dS; load[3 * NG + o] = cnt / dS;
  }
}

}  // namespace bnmf
