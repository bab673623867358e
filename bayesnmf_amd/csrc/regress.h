// bayesnmf_amd/csrc/regress.h — regression of exposures on tumour covariates over a recorded range: for every used sample of the
// record_sample rings and every factor the least-squares coefficients of the load, the share and the square root of the load on a design
// matrix, on the device (bnmf_regress / bnmf_regress_at).  Reads the rings after the fact, as k_contrast does; no sweep
// kernel is involved and none of the chain's streams is consumed.
//
// Per used sample s (oldest first), included tumour g_i (the member list, ascending) and factor n, with cs_s[n] the bits of k_map_colsum:
//   x = A_s[n] != 0 ? E_s[n,g] * cs_s[n] : +0.0;   t = sum_n x   n ascending from +0.0;   u = t > 0 ? 1 / t : 0.0
//   y0 = x    y1 = x * u    y2 = dsqrt(x)
// canonB, the blocked canonical sum over the m members: block b holds members RG_BLOCK b .. min(RG_BLOCK (b + 1), m) - 1; a block's sum is
// the canonical W = 64 sum of its members (accumulator l adds members l, l + 64, ... ascending from +0.0, then wave_tree64); the block sums
// are added with b ascending from +0.0.
//   totals  k_regress_total     t and u per (s, member)
//   pass 1  k_regress_moments   w[j] = canonB_i(y_i * D[i,j])  j < Q,   sy = canonB_i(y_i)                     the block partials
//   solve   k_regress_solve     the blocks added;  z_j = (w_j - sum_{t<j} L[j][t] z_t) / L[j][j];  beta_j = (z_j - sum_{t>j} L[t][j] beta_t) / L[j][j]
//                               (L the Cholesky factor of the Gram matrix, from the host; each sum t ascending, subtracted one by one);  ybar = sy / m
//   pass 2  k_regress_resid     yhat_i = sum_j D[i,j] * beta_j  j ascending from +0.0;  rss = canonB_i((y_i - yhat_i)^2),  tss = canonB_i((y_i - ybar)^2)
//   tail    k_regress_fit       the blocks added;  r2 = tss > 0 ? 1 - rss / tss : NaN;  sigma2 = rss / (m - Q)
// The statistics over s are the host's (posterior.h).
//
// Tiling.  k_regress_total: one wave per 64 members of a sample reads their columns E_s[., g] (N contiguous doubles each) together, sums t
// per member and leaves u.
// The two passes: one wavefront per (block, sample, tile): lane l IS accumulator l and walks members l, l + 64, ... of its block,
// RG_BLOCK / 64 = 16 rounds at most, so the chain of a block's sum is the loop, and a long cohort is many short waves where k_contrast had
// one long one per group.  The design is uploaded row-major in member order ([m][Q]): a wave's covariates are one contiguous run.  A tile
// is TN factors (and, in pass 1, TQ design columns; the column tile 0 also carries sy): a lane reads the tile's TN values of its member's
// column and u.  Every tiling is the same operations on the same values in the same order, hence the same bits: <4, 4> is the form
// that runs, <2, 2> the one BNMF_REG_FORM=1 forces (fewer registers, more waves).  The tiles of one block read the same cache lines of E:
// the units of a block are placed 8 apart in the grid (reg_unit), because workgroups are observed to be dealt round-robin over the 8 XCDs,
// so that they meet in one XCD's L2 — for speed only, nothing depends on it.
#pragma once
#include "dmath.h"

namespace bnmf {

constexpr int RG_BLOCK = 1024;    // members of a block of canonB: part of the spec
constexpr int RG_MAX_Q = 16;      // most design columns
constexpr int RG_NSTAT = 3;       // responses: load, share, sqrt(load)
struct RegArgs {
  const double *ringE, *ringA;    // record_sample rings: [slot][N*G], [slot][N]
  const double* cs;               // [S][N]: k_map_colsum
  const int* slots;               // ring slots of the used samples, oldest first
  const int* members;             // [m]: the included tumours, ascending
  const double* D;                // [m][Q]: the design, row-major in member order
  const double* L;                // [Q][Q] row-major: the Cholesky factor (lower triangle)
  double* part;                   // pass 1: [S][nb][3][N][Q + 1]  (w_0 .. w_{Q-1}, sy)
  double* part2;                  // pass 2: [S][nb][3][N][2]      (rss, tss)
  double* coef;                   // [3][S][N*Q], each n + N j: beta
  double* ybar;                   // [3][S][N]
  double* r2;                     // [3][S][N]
  double* sigma2;                 // [3][S][N]
  double* u;                      // [S][m]: 1 / t per member, 0 where t is not positive
  size_t lenE; int N, Q, S, m, nb;
};

// One wave per 64 members of a sample: t = sum_n x, n ascending from +0.0, and u.  The 64 columns are read RG_TC factors at a time by the
// whole wave, element e of the 64 x TC tile by lane e % 64 (adjacent members are adjacent in memory: one contiguous run), and x goes
// through the LDS to the lane that owns the member, which adds its row in order.
// (This kernel, k_regress_solve and k_regress_fit are templates although one instance of each runs: the compiler emits plain kernels in the
// order of the translation unit, in front of every template instance, and three plain kernels here moved k_zalloc_sort 8 KB away from
// k_draw in the code object — bench.py fell from 12,240 to 11,850 iterations/s with no sweep kernel changed.  Template instances are
// emitted behind everything that exists, so the sweep's kernels keep their distances: DESIGN.md §20.)
constexpr int RG_TC = 32;
template <int TC>
__global__ __launch_bounds__(64) void k_regress_total(RegArgs a) {
  __shared__ double xs[64][TC + 1];
  const int lane = (int)threadIdx.x, i0 = (int)blockIdx.x * 64, s = (int)blockIdx.y, N = a.N;
  const int cnt = min(64, a.m - i0);
  const double* Es = a.ringE + (size_t)a.slots[s] * a.lenE;
  const double* As = a.ringA + (size_t)a.slots[s] * (size_t)N;
  const double* cs = a.cs + (size_t)s * N;
  double tot = 0.0;
  for (int c0 = 0; c0 < N; c0 += TC) {
    const int w = min(TC, N - c0);
    for (int e = lane; e < cnt * w; e += 64) {
      const int r = e / w, n = c0 + e % w;
      xs[r][n - c0] = As[n] != 0.0 ? Es[(size_t)N * (size_t)a.members[i0 + r] + n] * cs[n] : 0.0;
    }
    __syncthreads();
    if (lane < cnt) for (int c = 0; c < w; ++c) tot = tot + xs[lane][c];
    __syncthreads();
  }
  if (lane < cnt) a.u[(size_t)s * a.m + i0 + lane] = tot > 0.0 ? 1.0 / tot : 0.0;
}

// unit `id` of a pass's grid -> its tile and block; false for the padding of the last 8 blocks
BNMF_DEV bool reg_unit(int id, int ntile, int nb, int& tile, int& b) {
  tile = (id >> 3) % ntile; b = (id & 7) + 8 * ((id >> 3) / ntile);
  return b < nb;
}
static inline unsigned reg_units(int ntile, int nb) { return (unsigned)ntile * 8u * (unsigned)((nb + 7) / 8); }

// the three responses of factor tile [n0, n0 + TN) of member i of sample s; x is a copy of factor N - 1 beyond N (never stored)
template <int TN>
BNMF_DEV void reg_responses(const RegArgs& a, const double* Es, const double (&f)[TN], const bool (&inc)[TN], int n0, int s, int i, double (&y)[RG_NSTAT][TN]) {
  const int N = a.N;
  const double* col = Es + (size_t)N * (size_t)a.members[i];
  double v[TN];
#pragma unroll
  for (int t = 0; t < TN; ++t) v[t] = col[min(n0 + t, N - 1)];
  const double u = a.u[(size_t)s * a.m + i];
#pragma unroll
  for (int t = 0; t < TN; ++t) {
    const double x = inc[t] ? v[t] * f[t] : 0.0;
    y[0][t] = x; y[1][t] = x * u; y[2][t] = dsqrt(x);
  }
}

template <int TN, int TQ>
__global__ __launch_bounds__(64) void k_regress_moments(RegArgs a) {
  const int lane = (int)threadIdx.x, s = (int)blockIdx.y, N = a.N, Q = a.Q;
  const int ntn = (N + TN - 1) / TN, ntq = (Q + TQ - 1) / TQ;
  int tile, b;
  if (!reg_unit((int)blockIdx.x, ntn * ntq, a.nb, tile, b)) return;   // wave-uniform
  const int n0 = (tile % ntn) * TN, j0 = (tile / ntn) * TQ;
  const double* Es = a.ringE + (size_t)a.slots[s] * a.lenE;
  const double* As = a.ringA + (size_t)a.slots[s] * (size_t)N;
  const double* cs = a.cs + (size_t)s * N;
  double f[TN]; bool inc[TN];
#pragma unroll
  for (int t = 0; t < TN; ++t) { const int n = min(n0 + t, N - 1); inc[t] = As[n] != 0.0; f[t] = cs[n]; }
  double aw[RG_NSTAT][TN][TQ], ay[RG_NSTAT][TN];
#pragma unroll
  for (int q = 0; q < RG_NSTAT; ++q)
#pragma unroll
    for (int t = 0; t < TN; ++t) {
      ay[q][t] = 0.0;
#pragma unroll
      for (int c = 0; c < TQ; ++c) aw[q][t][c] = 0.0;
    }
  const int i1 = min((b + 1) * RG_BLOCK, a.m);
  for (int i = b * RG_BLOCK + lane; i < i1; i += 64) {
    double y[RG_NSTAT][TN], d[TQ];
    reg_responses<TN>(a, Es, f, inc, n0, s, i, y);
#pragma unroll
    for (int c = 0; c < TQ; ++c) d[c] = a.D[(size_t)i * Q + min(j0 + c, Q - 1)];
#pragma unroll
    for (int q = 0; q < RG_NSTAT; ++q)
#pragma unroll
      for (int t = 0; t < TN; ++t) {
        ay[q][t] = ay[q][t] + y[q][t];
#pragma unroll
        for (int c = 0; c < TQ; ++c) aw[q][t][c] = aw[q][t][c] + y[q][t] * d[c];
      }
  }
  double* o = a.part + ((size_t)s * a.nb + b) * RG_NSTAT * N * (Q + 1);
#pragma unroll
  for (int q = 0; q < RG_NSTAT; ++q)
#pragma unroll
    for (int t = 0; t < TN; ++t) {
      if (n0 + t >= N) continue;                   // wave-uniform
      double* row = o + ((size_t)q * N + n0 + t) * (Q + 1);
#pragma unroll
      for (int c = 0; c < TQ; ++c) {
        if (j0 + c >= Q) continue;                 // wave-uniform
        const double v = wave_tree64(aw[q][t][c]);
        if (lane == 0) row[j0 + c] = v;
      }
      if (j0 == 0) { const double v = wave_tree64(ay[q][t]); if (lane == 0) row[Q] = v; }
    }
}

// one lane per (s, q, n): the blocks of pass 1 added, the two triangular solves in place in the lane's LDS column
template <int MQ>
__global__ __launch_bounds__(64) void k_regress_solve(RegArgs a) {
  __shared__ double zs[MQ][64];
  const int lane = (int)threadIdx.x, N = a.N, Q = a.Q, S = a.S;
  const size_t e = (size_t)blockIdx.x * 64 + lane, tot = (size_t)S * RG_NSTAT * N;
  if (e >= tot) return;
  const int n = (int)(e % N), q = (int)((e / N) % RG_NSTAT), s = (int)(e / ((size_t)N * RG_NSTAT));
  const size_t stride = (size_t)RG_NSTAT * N * (Q + 1);
  const double* p = a.part + (size_t)s * a.nb * stride + ((size_t)q * N + n) * (Q + 1);
  for (int j = 0; j <= Q; ++j) {
    double v = 0.0;
    for (int b = 0; b < a.nb; ++b) v = v + p[(size_t)b * stride + j];
    if (j < Q) zs[j][lane] = v;
    else a.ybar[((size_t)q * S + s) * N + n] = v / (double)a.m;
  }
  const double* L = a.L;
  for (int j = 0; j < Q; ++j) {
    double v = zs[j][lane];
    for (int t = 0; t < j; ++t) v = v - L[j * Q + t] * zs[t][lane];
    zs[j][lane] = v / L[j * Q + j];
  }
  double* o = a.coef + ((size_t)q * S + s) * N * Q + n;
  for (int j = Q - 1; j >= 0; --j) {
    double v = zs[j][lane];
    for (int t = j + 1; t < Q; ++t) v = v - L[t * Q + j] * zs[t][lane];
    v = v / L[j * Q + j];
    zs[j][lane] = v;
    o[(size_t)N * j] = v;
  }
}

template <int TN>
__global__ __launch_bounds__(64) void k_regress_resid(RegArgs a) {
  __shared__ double sb[RG_NSTAT][TN][RG_MAX_Q];    // the tile's coefficients
  const int lane = (int)threadIdx.x, s = (int)blockIdx.y, N = a.N, Q = a.Q, S = a.S;
  const int ntn = (N + TN - 1) / TN;
  int tile, b;
  if (!reg_unit((int)blockIdx.x, ntn, a.nb, tile, b)) return;         // uniform over the workgroup, before its barrier
  const int n0 = tile * TN;
  const double* Es = a.ringE + (size_t)a.slots[s] * a.lenE;
  const double* As = a.ringA + (size_t)a.slots[s] * (size_t)N;
  const double* cs = a.cs + (size_t)s * N;
  for (int e = lane; e < RG_NSTAT * TN * Q; e += 64) {
    const int j = e % Q, t = (e / Q) % TN, q = e / (Q * TN);
    sb[q][t][j] = a.coef[((size_t)q * S + s) * N * Q + min(n0 + t, N - 1) + (size_t)N * j];
  }
  __syncthreads();
  double f[TN], yb[RG_NSTAT][TN]; bool inc[TN];
#pragma unroll
  for (int t = 0; t < TN; ++t) {
    const int n = min(n0 + t, N - 1);
    inc[t] = As[n] != 0.0; f[t] = cs[n];
#pragma unroll
    for (int q = 0; q < RG_NSTAT; ++q) yb[q][t] = a.ybar[((size_t)q * S + s) * N + n];
  }
  double ar[RG_NSTAT][TN], at[RG_NSTAT][TN];
#pragma unroll
  for (int q = 0; q < RG_NSTAT; ++q)
#pragma unroll
    for (int t = 0; t < TN; ++t) { ar[q][t] = 0.0; at[q][t] = 0.0; }
  const int i1 = min((b + 1) * RG_BLOCK, a.m);
  for (int i = b * RG_BLOCK + lane; i < i1; i += 64) {
    double y[RG_NSTAT][TN], yh[RG_NSTAT][TN];
    reg_responses<TN>(a, Es, f, inc, n0, s, i, y);
#pragma unroll
    for (int q = 0; q < RG_NSTAT; ++q)
#pragma unroll
      for (int t = 0; t < TN; ++t) yh[q][t] = 0.0;
    for (int j = 0; j < Q; ++j) {
      const double d = a.D[(size_t)i * Q + j];
#pragma unroll
      for (int q = 0; q < RG_NSTAT; ++q)
#pragma unroll
        for (int t = 0; t < TN; ++t) yh[q][t] = yh[q][t] + d * sb[q][t][j];
    }
#pragma unroll
    for (int q = 0; q < RG_NSTAT; ++q)
#pragma unroll
      for (int t = 0; t < TN; ++t) {
        const double e = y[q][t] - yh[q][t], c = y[q][t] - yb[q][t];
        ar[q][t] = ar[q][t] + e * e;
        at[q][t] = at[q][t] + c * c;
      }
  }
  double* o = a.part2 + ((size_t)s * a.nb + b) * RG_NSTAT * N * 2;
#pragma unroll
  for (int q = 0; q < RG_NSTAT; ++q)
#pragma unroll
    for (int t = 0; t < TN; ++t) {
      if (n0 + t >= N) continue;                   // wave-uniform
      const double v0 = wave_tree64(ar[q][t]), v1 = wave_tree64(at[q][t]);
      if (lane == 0) { o[((size_t)q * N + n0 + t) * 2] = v0; o[((size_t)q * N + n0 + t) * 2 + 1] = v1; }
    }
}

// one lane per (s, q, n): the blocks of pass 2 added, r2 and sigma2
template <int NS>
__global__ __launch_bounds__(64) void k_regress_fit(RegArgs a) {
  const int N = a.N, S = a.S;
  const size_t e = (size_t)blockIdx.x * 64 + threadIdx.x, tot = (size_t)S * NS * N;
  if (e >= tot) return;
  const int n = (int)(e % N), q = (int)((e / N) % NS), s = (int)(e / ((size_t)N * NS));
  const size_t stride = (size_t)NS * N * 2;
  const double* p = a.part2 + (size_t)s * a.nb * stride + ((size_t)q * N + n) * 2;
  double rss = 0.0, tss = 0.0;
  for (int b = 0; b < a.nb; ++b) { rss = rss + p[(size_t)b * stride]; tss = tss + p[(size_t)b * stride + 1]; }
  const size_t at = ((size_t)q * S + s) * N + n;
  a.r2[at] = tss > 0.0 ? 1.0 - rss / tss : BNMF_NAN;
  a.sigma2[at] = rss / (double)(a.m - a.Q);
}

}  // namespace bnmf
