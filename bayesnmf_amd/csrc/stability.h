// bayesnmf_amd/csrc/stability.h — silhouette stability of the recorded signatures: the cosine distances between all recorded columns of P
// over a range (and further columns handed in), summed per point and cluster, on the device (bnmf_stability / bnmf_stability_at;
// DESIGN.md §22).  Reads the rings after the fact; no sweep kernel is involved and none of the chain's streams is consumed.
//
// Point (s, n) of used sample s has index s N + n, extra column x has index S N + x.  The members (posterior.h decides them from
// k_stab_norm's squared norms) are packed cluster by cluster in member-list order: position q of the packed order holds point src[q].
//   norms   k_stab_norm    per ring point ok = A_s[n] != 0 && nn finite && nn > 0, with nn = sum_k P_s[k,n]^2 (k ascending from +0.0)
//   gather  k_stab_gather  packed[k][q] = the column of point src[q] (row stride Mp, the members rounded up to ST_ROWS; the padding holds
//                          +0.0 with nn = 1) and nn[q] beside it, the same sum
//   pairs   k_stab_pairs   for every member i, cluster j and block b of canonB over j's member list the block partial of
//                          d(i, i') = 1 - dot(i, i') / dsqrt(nn_i nn_i'), dot summed over k ascending from +0.0, the self term +0.0
// The blocks are added in order by the host, and everything from D on is stability_reduce's (reduce_host.h).
//
// Tiling of k_stab_pairs.  A unit is one block of one cluster's member list (RG_BLOCK = 1,024 members at most: canonB of regress.h).  One
// wavefront takes a unit and ST_ROWS members i: lane l IS accumulator l of the canonical W = 64 sum and walks members l, l + 64, ... of
// the unit; per round it forms ST_ROWS dot products at once, its own column coming through one coalesced load per k (the packed layout is
// k-major, so the 64 lanes read 64 neighbouring doubles) and the ST_ROWS values p_i[k] being wave-uniform neighbours (scalar loads).  A
// workgroup is ST_WAVES such waves on the same unit with neighbouring rows, so that they stream the same columns through the CU's vector
// cache together.  The wave's tree closes a unit; the block partials land in part[i][unit] and the tiling never shows in the bits.
// Every kernel is a template (plain kernels move the sweep's kernels apart in the code object).
#pragma once
#include "dmath.h"
#include "regress.h"

namespace bnmf {

constexpr int ST_ROWS = 8;     // members i of a wave of k_stab_pairs
constexpr int ST_WAVES = 4;    // waves of its workgroup
struct StabArgs {
  const double *ringP, *ringA;           // record_sample rings: [slot][K*N], [slot][N]
  const int* slots;                      // ring slots of the used samples, oldest first
  const double* extra;                   // [X][K]: the further columns
  const int* src;                        // [Mp]: the point of packed position q; -1 in the padding
  const int *ustart, *uend;              // [U]: the packed positions [ustart, uend) of a unit
  int* ok;                               // [S*N]: k_stab_norm
  double* packed;                        // [K][Mp]
  double* nn;                            // [Mp]
  double* part;                          // [M][U]
  size_t lenP; int N, K, S, M, Mp, U;
};

template <int NS>
__global__ __launch_bounds__(64) void k_stab_norm(StabArgs a) {
  const int e = (int)blockIdx.x * 64 + (int)threadIdx.x;
  if (e >= a.S * a.N) return;
  const int s = e / a.N, n = e % a.N;
  const double* col = a.ringP + (size_t)a.slots[s] * a.lenP + (size_t)a.K * n;
  double nn = 0.0;
  for (int k = 0; k < a.K; ++k) { const double v = col[k]; nn = nn + v * v; }
  a.ok[e] = (a.ringA[(size_t)a.slots[s] * (size_t)a.N + n] != 0.0 && nn > 0.0 && nn < BNMF_INF) ? 1 : 0;
}

template <int NS>
__global__ __launch_bounds__(64) void k_stab_gather(StabArgs a) {
  const int q = (int)blockIdx.x * 64 + (int)threadIdx.x;
  if (q >= a.Mp) return;
  const int p = a.src[q], SN = a.S * a.N;
  if (p < 0) {                                     // padding: never a member, never stored from
    for (int k = 0; k < a.K; ++k) a.packed[(size_t)k * a.Mp + q] = 0.0;
    a.nn[q] = 1.0;
    return;
  }
  const double* col = p < SN ? a.ringP + (size_t)a.slots[p / a.N] * a.lenP + (size_t)a.K * (p % a.N) : a.extra + (size_t)a.K * (p - SN);
  double nn = 0.0;
  for (int k = 0; k < a.K; ++k) { const double v = col[k]; a.packed[(size_t)k * a.Mp + q] = v; nn = nn + v * v; }
  a.nn[q] = nn;
}

template <int R>
__global__ __launch_bounds__(64 * ST_WAVES) void k_stab_pairs(StabArgs a) {
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6, u = (int)blockIdx.x, K = a.K, M = a.M;
  const int i0 = ((int)blockIdx.y * ST_WAVES + __builtin_amdgcn_readfirstlane(wave)) * R;   // wave-uniform, and known to be: the rows come through scalar loads; i0 + R <= Mp when i0 < M
  if (i0 >= M) return;
  const size_t Mp = (size_t)a.Mp;
  const int j0 = a.ustart[u], j1 = a.uend[u];
  const double* __restrict__ pk = a.packed;
  const double* __restrict__ rows = pk + i0;
  double ni[R], acc[R];
#pragma unroll
  for (int r = 0; r < R; ++r) { ni[r] = a.nn[i0 + r]; acc[r] = 0.0; }
  for (int jb = j0; jb < j1; jb += 64) {
    const bool live = jb + lane < j1;
    const int j = live ? jb + lane : j1 - 1;
    const double* __restrict__ col = pk + j;
    double dot[R];
#pragma unroll
    for (int r = 0; r < R; ++r) dot[r] = 0.0;
#pragma unroll 2
    for (int k = 0; k < K; ++k) {
      const double x = col[(size_t)k * Mp];
#pragma unroll
      for (int r = 0; r < R; ++r) dot[r] = dot[r] + rows[(size_t)k * Mp + r] * x;
    }
    const double nj = a.nn[j];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      double d = 1.0 - dot[r] / dsqrt(ni[r] * nj);
      if (j == i0 + r) d = 0.0;
      if (live) acc[r] = acc[r] + d;
    }
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const double v = wave_tree64(acc[r]);
    if (lane == 0 && i0 + r < M) a.part[(size_t)(i0 + r) * a.U + u] = v;
  }
}

}  // namespace bnmf
