// bayesnmf_amd/csrc/tradeoff.h — trade-offs between signatures within a tumour over a recorded range: for every included tumour the
// N x N covariance of its aligned renormalised exposures over the used, matched samples of the record_sample rings, its correlations and
// what follows from them, on the device (bnmf_tradeoff / bnmf_tradeoff_at).  Reads the E and A rings and k_map_colsum's
// column sums of P after the fact; no sweep kernel is involved, no random number is drawn and none of the chain's streams is consumed.
//
// Per matched used sample t = 1 .. S' (oldest first) and member i (the included tumours g_0 < g_1 < ..., m of them), cs_t[n] the bits of
// k_map_colsum:
//   x[n] = A_t[n] != 0 ? E_t[n,g_i] * cs_t[n] : +0.0          contrast.h's x, the same bits;      q_t[perm_t[n]] = x[n]
//   mu[j]    = (sum_t q_t[j], t ascending from +0.0) / S'
//   cov[j,l] = (sum_t (q_t[j] - mu[j]) * (q_t[l] - mu[l]), t ascending from +0.0, the product rounded before it is added) / (S' - 1)
//              for l <= j, mirrored: bitwise symmetric
//   r[j,l]   = cov[j,j] * cov[l,l] > 0 and finite ? cov[j,l] / dsqrt(cov[j,j] * cov[l,l]) : NaN      (trd_r, the one place that forms it)
// The bits depend on the samples, used[], the member list, perm, sets, query and min_corr only: not on the tile, the form or the band of
// members whose covariances pass through the scratch.
//
//   k_trd_prep      one lane per (t, n): the sample's tables by aligned place j = perm_t[n]: the offset of factor n in the E ring, cs_t[n]
//                   and A_t[n] != 0, so that the two passes read a place with one dependent load.
//   k_trd_mean      one lane per (member, j): the sum over t in a register, mu [m][N].  Adjacent lanes read adjacent doubles of a column
//                   E_t[., g] (N contiguous doubles; perm only shuffles them within the column).
//   k_trd_comoment  the co-moment pass.  A lane owns (member, j, a tile of TL values of l <= j) with its TL sums in registers; the lanes
//                   of a member number trd_items(N): 24 for N = 20, TL = 16.  A workgroup of TD_T lanes takes TD_T / items members (one
//                   member and TD_T items of it where a member has more: blockIdx.y).  Per sample the d = q - mu of the workgroup's
//                   members are staged once in the LDS by the first members x N lanes, one value each, the next sample's value loaded
//                   before the barrier; two buffers in turn, so one barrier per sample.  A member's row in the LDS is N | 1 doubles
//                   long: an odd number of 8-byte words, so the rows of the up to 32 members that one half-wave touches start in
//                   different banks (a row of N = 20 doubles is 160 bytes: members 8 apart would meet in one bank).  A lane reads its
//                   d[j] and the TL values of its tile, which the other lanes of the member read as well (a broadcast).
//                   <16> is the form that runs, <8> the one BNMF_TRD_FORM=1 forces: every sum is one lane's, t ascending, in both.
//                   The covariances go to the scratch as [j * N + l][member of the band]: the kernels behind read them lane by member.
//   k_trd_finish    one lane per member of the band: row 0 - 2 of tumour, pair_at and setstat from the band's covariances.
//   k_trd_pair      one wave per pair j > l: lane a IS accumulator a of regress.h's canonB over the member positions (a position's
//                   accumulator is position % 64: RG_BLOCK is a multiple of 64) for (defined ? r : +0.0) and cov; a block's tree and the
//                   running sum of the blocks when the block's last position has passed.  Between bands the running sums stay in `run`
//                   and, where a band ends inside a block, the 64 accumulators in `carry`.  The counts are whole numbers.
//   k_trd_dense     the query tumours' matrices out of the band.
// No grid synchronisation, no atomics, no polling, no scratch memory, no MFMA.
#pragma once
#include "dmath.h"
#include "regress.h"

namespace bnmf {

constexpr int TD_T = 256;               // lanes of k_trd_comoment
constexpr int TD_MAX_N = 128;
constexpr int TD_MAX_C = 32;
constexpr int TD_NTUM = 3;              // smallest correlation, defined pairs, variance ratio of the total
constexpr int TD_NPAIR = 5;             // mean r, n_def, share r <= -min_corr, share r >= min_corr, mean covariance
constexpr int TD_NSET = 4;              // mean, variance of the sum, sum of the variances, their ratio
constexpr int TD_STAGE = 2 * TD_T;      // doubles of one staging buffer: members * (N | 1) <= TD_T + members

struct TrdArgs {
  const double* ringE;                  // record_sample ring: [slot][N*G]
  const long long* off;                 // [S][N]: by aligned place, the offset of the factor in ringE (slot and factor)
  const double* f;                      // [S][N]: by aligned place, cs_t of the factor
  const int* on;                        // [S][N]: by aligned place, A_t of the factor != 0
  const int* members;                   // [m]: the included tumours, ascending
  double* mu;                           // [m][N]
  double* cov;                          // [N*N][mb]: the band's covariances
  int N, S, m, i0, cnt, mb;             // the band: member positions i0 .. i0 + cnt - 1, mb the stride of cov
};

// the lanes of a member in the co-moment pass: factor j has j / TL + 1 tiles of TL values of l
static inline __host__ __device__ int trd_items(int N, int TL) {
  const int kf = N / TL;
  return TL * kf * (kf + 1) / 2 + (N % TL) * (kf + 1);
}
// item w of a member -> its factor j and the first l of its tile
BNMF_DEV void trd_item(int w, int TL, int& j, int& l0) {
  int k = 0;
  while (TL * (k + 1) * (k + 2) / 2 <= w) ++k;
  const int r = w - TL * k * (k + 1) / 2;
  j = k * TL + r / (k + 1); l0 = (r % (k + 1)) * TL;
}
BNMF_DEV double trd_q(const TrdArgs& a, int t, int j, int g) {
  const size_t e = (size_t)t * a.N + j;
  const double v = a.ringE[(size_t)a.off[e] + (size_t)a.N * (size_t)g];
  return a.on[e] ? v * a.f[e] : 0.0;
}
// the correlation of a pair; false and NaN where it is undefined
BNMF_DEV bool trd_r(double c, double vj, double vl, double& r) {
  const double pr = vj * vl;
  const bool def = pr > 0.0 && pr < BNMF_INF;
  r = def ? c / dsqrt(pr) : BNMF_NAN;
  return def;
}

// (the kernels are templates although one instance of most runs: template instances are emitted behind every kernel that exists, so the
// sweep's kernels keep their places in the code object)
template <int>
__global__ __launch_bounds__(256) void k_trd_prep(const double* ringA, const double* cs /* [S][N] */, const int* slots, const int* perm /* [S][N] */, int N, int S,
                                                  size_t lenE, long long* off, double* f, int* on) {
  const int e = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (e >= S * N) return;
  const int t = e / N, n = e % N, slot = slots[t];
  const size_t o = (size_t)t * N + perm[e];                     // (a permutation of 0 .. N-1: checked on the host)
  off[o] = (long long)((size_t)slot * lenE + n); f[o] = cs[e]; on[o] = ringA[(size_t)slot * N + n] != 0.0 ? 1 : 0;
}

template <int>
__global__ __launch_bounds__(256) void k_trd_mean(TrdArgs a) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (size_t)a.m * a.N) return;
  const int i = (int)(e / a.N), j = (int)(e % a.N), g = a.members[i];
  double acc = 0.0;
#pragma unroll 4
  for (int t = 0; t < a.S; ++t) acc = acc + trd_q(a, t, j, g);
  a.mu[e] = acc / (double)a.S;
}

template <int TL>
__global__ __launch_bounds__(TD_T) void k_trd_comoment(TrdArgs a) {
  __shared__ double ds[2][TD_STAGE];
  const int tid = (int)threadIdx.x, N = a.N, NS = N | 1, S = a.S;
  const int items = trd_items(N, TL), per = min(items, TD_T), MB = TD_T / per;
  const int ib0 = (int)blockIdx.x * MB, nmem = min(MB, a.cnt - ib0);        // the workgroup's members: positions i0 + ib0 ...
  // the lane that stages (member sm, place sj)
  const bool stage = tid < nmem * N;
  const int sm = stage ? tid / N : 0, sj = stage ? tid % N : 0;
  const int sg = a.members[a.i0 + ib0 + sm];
  const double smu = a.mu[(size_t)(a.i0 + ib0 + sm) * N + sj];
  // the lane that sums (member mi, factor j, l0 .. l0 + TL - 1)
  const int mi = tid / per, w = (int)blockIdx.y * TD_T + tid % per;
  const bool work = mi < nmem && w < items;
  int j = 0, l0 = 0;
  if (work) trd_item(w, TL, j, l0);
  double acc[TL];
#pragma unroll
  for (int k = 0; k < TL; ++k) acc[k] = 0.0;
  double qn = stage ? trd_q(a, 0, sj, sg) : 0.0;
  for (int t = 0; t < S; ++t) {                                              // workgroup-uniform
    double* buf = ds[t & 1];
    if (stage) buf[sm * NS + sj] = qn - smu;
    if (stage && t + 1 < S) qn = trd_q(a, t + 1, sj, sg);
    __syncthreads();                                                         // (the buffer written now was last read two samples ago)
    if (work) {
      const double* row = buf + mi * NS;
      const double dj = row[j];
#pragma unroll
      for (int k = 0; k < TL; ++k) acc[k] = acc[k] + dj * row[min(l0 + k, j)];
    }
  }
  if (!work) return;
  const size_t ib = (size_t)(ib0 + mi), mb = (size_t)a.mb;
#pragma unroll
  for (int k = 0; k < TL; ++k) {
    const int l = l0 + k;
    if (l > j) continue;
    const double c = acc[k] / (double)(S - 1);
    a.cov[((size_t)j * N + l) * mb + ib] = c;
    a.cov[((size_t)l * N + j) * mb + ib] = c;
  }
}

template <int NT>
__global__ __launch_bounds__(256) void k_trd_finish(TrdArgs a, const int* sets /* [N] or null */, int C, double* tum /* [NT][m] */, int32_t* pair_at /* [m] */,
                                                    double* setstat /* [TD_NSET][C][m] */) {
  const int ib = (int)blockIdx.x * 256 + (int)threadIdx.x, N = a.N;
  if (ib >= a.cnt) return;
  const size_t mb = (size_t)a.mb, m = (size_t)a.m, pos = (size_t)a.i0 + ib;
  const double* cv = a.cov + ib;
  double best = BNMF_NAN, vt = 0.0, sv = 0.0; int at = -1, ndef = 0;
  for (int j = 0; j < N; ++j) {
    const double vj = cv[((size_t)j * N + j) * mb];
    double inner = 0.0;
    for (int l = 0; l < N; ++l) {
      const double c = cv[((size_t)j * N + l) * mb];
      inner = inner + c;
      if (l < j) {
        double r;
        if (trd_r(c, vj, cv[((size_t)l * N + l) * mb], r)) {
          ++ndef;
          if (at < 0 || r < best) { best = r; at = j * N + l; }
        }
      }
    }
    vt = vt + inner; sv = sv + vj;
  }
  tum[pos] = best; tum[m + pos] = (double)ndef; tum[2 * m + pos] = (sv > 0.0 && sv < BNMF_INF) ? vt / sv : BNMF_NAN;
  pair_at[pos] = at;
  for (int c = 0; c < C; ++c) {                                              // uniform: sets[] is read through the scalar unit
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int j = 0; j < N; ++j) {
      if (sets[j] != c) continue;
      s0 = s0 + a.mu[pos * N + j];
      double inner = 0.0;
      for (int l = 0; l < N; ++l) if (sets[l] == c) inner = inner + cv[((size_t)j * N + l) * mb];
      s1 = s1 + inner; s2 = s2 + cv[((size_t)j * N + j) * mb];
    }
    double* o = setstat + (size_t)c * m + pos;
    const size_t row = (size_t)C * m;
    o[0] = s0; o[row] = s1; o[2 * row] = s2; o[3 * row] = (s2 > 0.0 && s2 < BNMF_INF) ? s1 / s2 : BNMF_NAN;
  }
}

template <int>
__global__ __launch_bounds__(64) void k_trd_pair(TrdArgs a, double min_corr, double* carry /* [N*N][2][64] or null */, double* run /* [N*N][2] */,
                                                 int32_t* cnts /* [N*N][3] */) {
  const int j = (int)blockIdx.x, l = (int)blockIdx.y, lane = (int)threadIdx.x, N = a.N;
  if (l >= j) return;                                                        // wave-uniform
  const size_t p = (size_t)j * N + l, mb = (size_t)a.mb;
  const double *cjl = a.cov + p * mb, *cjj = a.cov + ((size_t)j * N + j) * mb, *cll = a.cov + ((size_t)l * N + l) * mb;
  double ar = carry ? carry[(p * 2) * 64 + lane] : 0.0, ac = carry ? carry[(p * 2 + 1) * 64 + lane] : 0.0;
  double runr = run[p * 2], runc = run[p * 2 + 1];
  int nd = 0, nle = 0, nge = 0;
  const int pend = a.i0 + a.cnt;
  for (int b = a.i0 / RG_BLOCK; b * RG_BLOCK < pend; ++b) {
    const int lo = max(a.i0, b * RG_BLOCK), hi = min(pend, (b + 1) * RG_BLOCK);
    for (int i = lo + ((lane - lo) & 63); i < hi; i += 64) {                 // the positions of the band whose accumulator is `lane`
      const int ib = i - a.i0;
      const double c = cjl[ib];
      double r;
      const bool def = trd_r(c, cjj[ib], cll[ib], r);
      ar = ar + (def ? r : 0.0); ac = ac + c;
      nd += def ? 1 : 0; nle += (def && r <= -min_corr) ? 1 : 0; nge += (def && r >= min_corr) ? 1 : 0;
    }
    if (hi == min(a.m, (b + 1) * RG_BLOCK)) {                                // the block's last position has passed
      const double vr = wave_tree64(ar), vc = wave_tree64(ac);
      runr = runr + vr; runc = runc + vc; ar = 0.0; ac = 0.0;
    }
  }
  if (carry) { carry[(p * 2) * 64 + lane] = ar; carry[(p * 2 + 1) * 64 + lane] = ac; }
  for (int o = 32; o >= 1; o >>= 1) { nd += __shfl_xor(nd, o); nle += __shfl_xor(nle, o); nge += __shfl_xor(nge, o); }
  if (lane == 0) { run[p * 2] = runr; run[p * 2 + 1] = runc; cnts[p * 3] += nd; cnts[p * 3 + 1] += nle; cnts[p * 3 + 2] += nge; }
}

template <int>
__global__ __launch_bounds__(256) void k_trd_dense(TrdArgs a, const int* qplace /* [Q] member positions */, double* dense /* [Q][2][N*N] */) {
  const int q = (int)blockIdx.x, N = a.N, ib = qplace[q] - a.i0;
  if (ib < 0 || ib >= a.cnt) return;                                         // another band's
  const size_t mb = (size_t)a.mb, NN = (size_t)N * N;
  const double* cv = a.cov + ib;
  for (int e = (int)threadIdx.x; e < N * N; e += 256) {
    const int j = e / N, l = e % N;
    const double c = cv[(size_t)e * mb];
    double r;
    trd_r(c, cv[((size_t)j * N + j) * mb], cv[((size_t)l * N + l) * mb], r);
    dense[(size_t)q * 2 * NN + e] = c;
    dense[(size_t)q * 2 * NN + NN + e] = j == l ? BNMF_NAN : r;
  }
}

}  // namespace bnmf
