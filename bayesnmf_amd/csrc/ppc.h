// bayesnmf_amd/csrc/ppc.h — posterior predictive checks of a recorded range: for every used sample of the record_sample rings a
// replicate of the data is drawn from the sample's own fit and compared with the data, per cell, per column and over the whole
// matrix, on the device (bnmf_ppc / bnmf_ppc_at).  Reads the rings after the fact, as k_waic does; no sweep kernel
// is involved and none of the chain's own streams is consumed.
//
// Per cell (k, g), over the used samples s = 1..S, oldest first (t_s = the iteration of sample s):
//   c_s   = sum_n (P_s[k,n] * A_s[n]) * E_s[n,g]            n ascending from +0.0, associated as written (waic.h's c)
//   y_s   = rpois(lam), lam = c_s < 1e-6 ? 1e-6 : c_s                                 Poisson
//         = c_s + sd * rnorm_std, sd = dsqrt(sigmasq_s[g])                            Normal
//           both on stream (BNMF_V_YREP, element k + K g, iteration t_s) under the handle's key
//   Welford:  d = y_s - mu;  mu = mu + d * (1 / s);  M2 = M2 + d * (y_s - mu);   counts  n_less += (y_s < m), n_equal += (y_s == m)
//   mean = mu, var = M2 / (S - 1), p_less = n_less / S, p_equal = n_equal / S;  a tail cell: p_less + 0.5 p_equal outside [0.025, 0.975]
// Per column g and sample s, on the data x = m and on the replicate x = y_s, against the same fit:
//   Poisson: T1 = sum_k t * t, t = dsqrt(x) - dsqrt(lam);   T2 = sum_k (x == 0 ? 1 : 0)
//   Normal : T1 = sum_k z * z, z = (x - c_s) / sd;          T2 = max_k |z|   (from 0.0)
// The sums over k: rows in chunks of 128; inside a chunk the canonical W = 64 order (accumulator l adds rows l, l + 64 of the chunk
// from +0.0, then wave_tree64); the column's value is the first chunk's sum, then + the next chunk's, ascending (K <= 128: one chunk,
// the plain canonical sum).  k_ppc leaves them in T[4][S][G] (T1 data, T1 replicate, T2 data, T2 replicate).
// k_ppc_totals then gives, per column, over s ascending from +0.0: the sums of T data and T replicate, each / S, and
// #(T replicate >= T data) / S, for T1 (rows 0-2 of col) and T2 (rows 3-5); and per (T, s) the whole-matrix value: canon(T[.][s][g], W = 1024)
// over g, a plain maximum for the Normal T2.  The bits depend on nothing else: not on the tiling below.
//
// Tiling: k_waic's.  A workgroup is 4 wavefronts and owns PP_GC = 8 adjacent columns, 2 per wavefront; lane = row; row chunks of
// PP_CH = 128 (two 64-row passes), the sample loop inside the chunk loop, so the statistics of a cell stay in its lane's registers.
// Per sample the workgroup stages the chunk of P_s diag(A_s) and its 8 columns of E_s in the LDS between two barriers; the draws and
// their rejection loops, which diverge per lane, come after the second barrier and hold none.  Where the stage exceeds 160 KB
// (N > 150) the lanes read P, A and E through the caches: the same operations on the same values.
#pragma once
#include "dsamplers.h"

namespace bnmf {

constexpr int PP_T = 256, PP_CW = 2, PP_RP = 2, PP_CH = 64 * PP_RP, PP_GC = (PP_T / 64) * PP_CW;
constexpr int PP_TT = 1024;      // threads of k_ppc_totals: the W of the sums over g
constexpr int PP_NCOL = 6;       // per-column outputs: mean T1 data, mean T1 replicate, p1, mean T2 data, mean T2 replicate, p2
constexpr uint32_t PP_VAR = 19;  // BNMF_V_YREP
struct PpcArgs {
  const double *ringP, *ringE, *ringA, *ringS;   // record_sample rings: [slot][K*N], [slot][N*G], [slot][N], [slot][G] (Normal)
  const int32_t* M; const double* Mf;            // the data: counts (Poisson) or fp64 (Normal), column-major K x G
  const int *slots, *iters;                      // ring slot and iteration number of the used samples, oldest first
  double *T /* [4][S][G] */, *tail /* [G]: tail cells per column */, *cell /* [4][K*G]: mean, var, p_less, p_equal; may be null */;
  size_t lenP, lenE; int K, N, G, S, stage; uint32_t k0, k1;
};
inline size_t ppc_lds_bytes(int N) { return ((size_t)N * PP_CH + (size_t)N * PP_GC) * sizeof(double); }

BNMF_DEV double wave_max64(double v) {   // every lane gets the maximum over the wave (no NaN among the values)
#pragma unroll
  for (int h = 32; h >= 1; h >>= 1) { const double o = __shfl_xor(v, h); v = o > v ? o : v; }
  return v;
}

template <bool NORMAL>
__global__ __launch_bounds__(PP_T) void k_ppc(PpcArgs a) {
  extern __shared__ double pp_lds[];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int K = a.K, N = a.N, G = a.G, S = a.S;
  const int gb = (int)blockIdx.x * PP_GC;
  const int ncw = min(PP_GC, G - gb);              // columns of this workgroup that exist (>= 1 by the grid)
  double* pa = pp_lds;                             // [N][PP_CH]  P_s diag(A_s), rows of the chunk
  double* es = pp_lds + (size_t)N * PP_CH;         // [ncw][N]    E_s[, gb ..]
  int jl[PP_CW], gc[PP_CW]; bool gok[PP_CW];
#pragma unroll
  for (int j = 0; j < PP_CW; ++j) { const int q = wave * PP_CW + j; gok[j] = q < ncw; jl[j] = gok[j] ? q : ncw - 1; gc[j] = gb + jl[j]; }
  double tail[PP_CW];
#pragma unroll
  for (int j = 0; j < PP_CW; ++j) tail[j] = 0.0;
  const double dS = (double)S, dS1 = (double)(S - 1);
  const size_t SG = (size_t)S * (size_t)G;

  for (int k0 = 0; k0 < K; k0 += PP_CH) {
    double md[PP_CW][PP_RP], sm[PP_CW][PP_RP], mu[PP_CW][PP_RP], m2[PP_CW][PP_RP];
    int nl[PP_CW][PP_RP], ne[PP_CW][PP_RP];
    bool kok[PP_RP];
#pragma unroll
    for (int p = 0; p < PP_RP; ++p) kok[p] = k0 + p * 64 + lane < K;
#pragma unroll
    for (int j = 0; j < PP_CW; ++j)
#pragma unroll
      for (int p = 0; p < PP_RP; ++p) {
        const int k = min(k0 + p * 64 + lane, K - 1);
        const size_t at = (size_t)k + (size_t)K * (size_t)gc[j];
        if constexpr (NORMAL) { md[j][p] = a.Mf[at]; sm[j][p] = 0.0; }
        else { md[j][p] = (double)a.M[at]; sm[j][p] = dsqrt(md[j][p]); }
        mu[j][p] = 0.0; m2[j][p] = 0.0; nl[j][p] = 0; ne[j][p] = 0;
      }
    for (int s = 0; s < S; ++s) {
      const size_t slot = (size_t)a.slots[s];
      const uint32_t iter = (uint32_t)a.iters[s];
      const double* Ps = a.ringP + slot * a.lenP;
      const double* Es = a.ringE + slot * a.lenE;
      const double* As = a.ringA + slot * (size_t)N;
      if (a.stage) {
        __syncthreads();                           // the previous sample's reads of the stage are done
        for (int e = tid; e < N * PP_CH; e += PP_T) {
          const int r = e & (PP_CH - 1), n = e / PP_CH, k = k0 + r;
          pa[e] = k < K ? Ps[(size_t)k + (size_t)K * n] * As[n] : 0.0;
        }
        for (int e = tid; e < ncw * N; e += PP_T) es[e] = Es[(size_t)N * gb + e];
        __syncthreads();
      }
      const double rs = 1.0 / (double)(s + 1);
#pragma unroll
      for (int j = 0; j < PP_CW; ++j) {
        if (!gok[j]) continue;                     // wave-uniform: the wave has no such column
        double sd = 1.0;
        if constexpr (NORMAL) sd = dsqrt(a.ringS[slot * (size_t)G + gc[j]]);
        double t1o = 0.0, t1r = 0.0, t2o = 0.0, t2r = 0.0;
#pragma unroll
        for (int p = 0; p < PP_RP; ++p) {
          double c = 0.0;
          if (a.stage) {
            const double* pr = pa + p * 64 + lane;
            const double* er = es + (size_t)jl[j] * N;
            for (int n = 0; n < N; ++n) c = c + pr[(size_t)n * PP_CH] * er[n];
          } else {
            const int k = min(k0 + p * 64 + lane, K - 1);
            const double* er = Es + (size_t)N * gc[j];
            for (int n = 0; n < N; ++n) c = c + (Ps[(size_t)k + (size_t)K * n] * As[n]) * er[n];
          }
          if (kok[p]) {                            // the draw diverges per lane; no barrier inside
            const int k = k0 + p * 64 + lane;
            Stream st(a.k0, a.k1, PP_VAR, (uint32_t)((size_t)k + (size_t)K * (size_t)gc[j]), iter);
            const double m = md[j][p];
            double y;
            if constexpr (NORMAL) {
              y = c + sd * rnorm_std(st);
              const double zo = (m - c) / sd, zr = (y - c) / sd;
              t1o = t1o + zo * zo; t1r = t1r + zr * zr;
              const double ao = dabs(zo), ar = dabs(zr);
              t2o = ao > t2o ? ao : t2o; t2r = ar > t2r ? ar : t2r;
            } else {
              const double lam = c < 1e-6 ? 1e-6 : c;
              y = rpois(st, lam);
              const double sl = dsqrt(lam);
              const double d0 = sm[j][p] - sl, d1 = dsqrt(y) - sl;
              t1o = t1o + d0 * d0; t1r = t1r + d1 * d1;
              t2o = t2o + (m == 0.0 ? 1.0 : 0.0); t2r = t2r + (y == 0.0 ? 1.0 : 0.0);
            }
            nl[j][p] += y < m ? 1 : 0; ne[j][p] += y == m ? 1 : 0;
            const double d = y - mu[j][p];
            mu[j][p] = mu[j][p] + d * rs;
            m2[j][p] = m2[j][p] + d * (y - mu[j][p]);
          }
        }
        const double r0 = wave_tree64(t1o), r1 = wave_tree64(t1r);
        const double r2 = NORMAL ? wave_max64(t2o) : wave_tree64(t2o), r3 = NORMAL ? wave_max64(t2r) : wave_tree64(t2r);
        if (lane == 0) {
          double* Tp = a.T + (size_t)s * (size_t)G + (size_t)gc[j];
          if (k0 == 0) { Tp[0] = r0; Tp[SG] = r1; Tp[2 * SG] = r2; Tp[3 * SG] = r3; }
          else {
            Tp[0] = Tp[0] + r0; Tp[SG] = Tp[SG] + r1;
            if constexpr (NORMAL) { const double o2 = Tp[2 * SG], o3 = Tp[3 * SG]; Tp[2 * SG] = r2 > o2 ? r2 : o2; Tp[3 * SG] = r3 > o3 ? r3 : o3; }
            else { Tp[2 * SG] = Tp[2 * SG] + r2; Tp[3 * SG] = Tp[3 * SG] + r3; }
          }
        }
      }
    }
#pragma unroll
    for (int p = 0; p < PP_RP; ++p) {
      const int k = k0 + p * 64 + lane;
      if (k < K) {
#pragma unroll
        for (int j = 0; j < PP_CW; ++j) {
          if (!gok[j]) continue;
          const double var = m2[j][p] / dS1;
          const double pl = (double)nl[j][p] / dS, pe = (double)ne[j][p] / dS;
          const double pit = pl + 0.5 * pe;
          tail[j] = tail[j] + ((pit < 0.025 || pit > 0.975) ? 1.0 : 0.0);
          if (a.cell) {
            const size_t KG = (size_t)K * (size_t)G, at = (size_t)k + (size_t)K * (size_t)gc[j];
            a.cell[at] = mu[j][p]; a.cell[KG + at] = var; a.cell[2 * KG + at] = pl; a.cell[3 * KG + at] = pe;
          }
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < PP_CW; ++j) {
    const double r = wave_tree64(tail[j]);         // whole numbers: exact in any order
    if (lane == 0 && gok[j]) a.tail[gc[j]] = r;
  }
}

// Blocks 0 .. 4S-1: block q S + s reduces T[q][s][.] over g (series[q][s]).  The blocks after them: a thread per column, over s.
template <bool NORMAL>
__global__ __launch_bounds__(PP_TT) void k_ppc_totals(const double* T, int S, int G, double* series /* [4][S] */, double* col /* [PP_NCOL][G] */) {
  __shared__ double buf[PP_TT];
  const int tid = (int)threadIdx.x, b = (int)blockIdx.x;
  if (b < 4 * S) {                                 // block-uniform
    const double* x = T + (size_t)b * (size_t)G;
    const bool mx = NORMAL && b >= 2 * S;
    double acc = 0.0;
    for (int g = tid; g < G; g += PP_TT) { const double v = x[g]; acc = mx ? (v > acc ? v : acc) : acc + v; }
    double r;
    if (mx) {
      buf[tid] = acc;
      __syncthreads();
      for (int h = PP_TT / 2; h >= 1; h >>= 1) {
        if (tid < h) { const double o = buf[tid + h]; if (o > buf[tid]) buf[tid] = o; }
        __syncthreads();
      }
      r = buf[0];
    } else r = block_tree<PP_TT>(acc, buf, tid);
    if (tid == 0) series[b] = r;
    return;
  }
  const int g = (b - 4 * S) * PP_TT + tid;
  if (g >= G) return;
  const size_t SG = (size_t)S * (size_t)G;
  const double dS = (double)S;
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const double* To = T + (size_t)(2 * t) * SG + g;
    const double* Tr = To + SG;
    double so = 0.0, sr = 0.0; int n = 0;
    for (int s = 0; s < S; ++s) {
      const double o = To[(size_t)s * G], r = Tr[(size_t)s * G];
      so = so + o; sr = sr + r; n += r >= o ? 1 : 0;
    }
    col[(size_t)(3 * t) * G + g] = so / dS; col[(size_t)(3 * t + 1) * G + g] = sr / dS; col[(size_t)(3 * t + 2) * G + g] = (double)n / dS;
  }
}

}  // namespace bnmf
