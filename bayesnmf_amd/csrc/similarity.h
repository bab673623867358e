// bayesnmf_amd/csrc/similarity.h — similarity of tumours over a recorded range: for every used sample of the record_sample rings the
// cosine between the renormalised exposure profiles of every pair of included tumours, and over the samples its mean, variance and the
// share of samples above a threshold, on the device (bnmf_similarity / bnmf_similarity_at).  Reads the E and A rings and
// k_map_colsum's column sums of P after the fact; no sweep kernel is involved, no random number is drawn and none of the chain's streams
// is consumed.
//
// Per used sample s (oldest first) and member i (the included tumours g_0 < g_1 < ..., m of them), cs_s[n] the bits of k_map_colsum:
//   x[n,i]   = A_s[n] != 0 ? E_s[n,g_i] * cs_s[n] : +0.0           contrast.h's x, the same bits
//   nn[i]    = sum_n x[n,i] * x[n,i]        dot(i,j) = sum_n x[n,i] * x[n,j]          n ascending from +0.0
//   c(i,j)   = nn[i] * nn[j] == 0 ? +0.0 : dot(i,j) / dsqrt(nn[i] * nn[j])            bitwise symmetric in (i, j)
// Per pair over s ascending, attribution.h's Welford and a whole-number count:
//   d = c - mu;  mu = mu + d * (1 / s);  M2 = M2 + d * (c - mu);  cnt += (c >= min_cosine)
//   mean = mu    var = M2 / (S - 1)    p = cnt / S
// The bits depend on the samples, used[], the member list and min_cosine only: not on the tile, the band or the chunk of factors.
//
//   k_sim_norm    a thread per (s, member): nn, n ascending.
//   k_sim_pairs   the hot one.  A workgroup of 256 lanes owns a tile of SM_TILE x SM_TILE pairs (rows: the band's row list, columns: the
//                 member list) and loops over s with the Welford state of its pairs in registers, so no m x m x S intermediate exists.
//                 Lane (ty, tx) owns the 4 x 4 pairs of rows ty + 16 a and columns tx + 16 b: a wave's column reads of the LDS are 16
//                 consecutive doubles (conflict-free), its row reads broadcasts, its stores 16 consecutive doubles.  Per sample the
//                 tile's 2 x 64 profiles are staged in the LDS in chunks of SM_NC factors ([n][place], row stride 65 doubles); the dot
//                 products run on through the chunks, so a chunk boundary changes no bit and any N takes the one form.  A place past
//                 the end repeats the last row / member and stores nothing.  The results of a band of rows go to res [3][nr][m].
//   k_sim_select  a wave per row of the band: the blocked canonical sum of the means over the member list (regress.h's canonB, the self
//                 term entered as +0.0; lane l IS accumulator l), the degree, and max(top_k, 1) rounds of an arg-max under the total
//                 order (mean descending, lower member first; a NaN is no candidate), each round restricted to what follows the previous
//                 pick.  Only comparisons: the order of the lanes cannot change the result.
// No atomics, no polling, no scratch memory, no MFMA.
#pragma once
#include "dmath.h"

namespace bnmf {

constexpr int SM_T = 256;               // threads of k_sim_pairs: 16 x 16 lanes
constexpr int SM_TILE = 64;             // rows and columns of a tile
constexpr int SM_R = 4;                 // a lane's rows and columns, 16 apart
constexpr int SM_NC = 32;               // factors of a staged chunk
constexpr int SM_LD = SM_TILE + 1;      // doubles between the rows of a staged chunk: the staging stores of a wave spread over the banks
constexpr int SM_NROW = 3;              // mean, variance, p_similar
constexpr int SM_MAX_K = 32;

struct SimArgs {
  const double *ringE, *ringA;          // record_sample rings: [slot][N*G], [slot][N]
  const double* cs;                     // [S][N]: k_map_colsum
  const double* nn;                     // [S][m]: k_sim_norm
  const int* slots;                     // ring slots of the used samples, oldest first
  const int* members;                   // [m]: the included tumours, ascending
  const int* rows;                      // [nr]: the member (its place in the member list) of every row of the band
  double* res;                          // [3][nr][m]
  size_t lenE; int N, S, m, nr; double min_cosine;
};

// (the kernels use no template parameter: they are templates only for their place in the code object, behind every kernel that exists,
// DESIGN.md 20)
template <int>
__global__ __launch_bounds__(256) void k_sim_norm(const double* ringE, const double* ringA, const double* cs, const int* slots, const int* members,
                                                  size_t lenE, int N, int S, int m, double* nn /* [S][m] */) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (size_t)S * (size_t)m) return;
  const int s = (int)(e / (size_t)m), i = (int)(e % (size_t)m);
  const double* col = ringE + (size_t)slots[s] * lenE + (size_t)N * (size_t)members[i];
  const double* As = ringA + (size_t)slots[s] * (size_t)N;
  const double* c = cs + (size_t)s * N;
  double a = 0.0;
  for (int n = 0; n < N; ++n) {
    const double x = As[n] != 0.0 ? col[n] * c[n] : 0.0;
    a = a + x * x;
  }
  nn[e] = a;
}

template <int>
__global__ __launch_bounds__(SM_T) void k_sim_pairs(SimArgs a) {
  __shared__ double xr[SM_NC * SM_LD], xc[SM_NC * SM_LD];
  const int tid = (int)threadIdx.x, tx = tid & 15, ty = tid >> 4, N = a.N, m = a.m;
  const int c0 = (int)blockIdx.x * SM_TILE, r0 = (int)blockIdx.y * SM_TILE;
  // staging: two lanes per place, the 64 rows then the 64 columns; lane `half` takes factors half, half + 2, ... of the chunk
  const int place = tid >> 1, half = tid & 1;
  const int sp = place < SM_TILE ? a.rows[min(r0 + place, a.nr - 1)] : min(c0 + place - SM_TILE, m - 1);   // the member staged here
  const size_t sg = (size_t)N * (size_t)a.members[sp];
  double* const sdst = (place < SM_TILE ? xr : xc) + (place & (SM_TILE - 1));
  int ri[SM_R], ci[SM_R];                                       // the members of the lane's rows and columns
#pragma unroll
  for (int q = 0; q < SM_R; ++q) { ri[q] = a.rows[min(r0 + ty + 16 * q, a.nr - 1)]; ci[q] = min(c0 + tx + 16 * q, m - 1); }
  double mu[SM_R][SM_R], m2[SM_R][SM_R]; int cnt[SM_R][SM_R];
#pragma unroll
  for (int p = 0; p < SM_R; ++p)
#pragma unroll
    for (int q = 0; q < SM_R; ++q) { mu[p][q] = 0.0; m2[p][q] = 0.0; cnt[p][q] = 0; }

  for (int s = 0; s < a.S; ++s) {
    const size_t slot = (size_t)a.slots[s];
    const double* Es = a.ringE + slot * a.lenE + sg;
    const double* As = a.ringA + slot * (size_t)N;
    const double* cs = a.cs + (size_t)s * N;
    const double* nn = a.nn + (size_t)s * (size_t)m;
    double nr[SM_R], nc[SM_R];
#pragma unroll
    for (int q = 0; q < SM_R; ++q) { nr[q] = nn[ri[q]]; nc[q] = nn[ci[q]]; }
    double dot[SM_R][SM_R];
#pragma unroll
    for (int p = 0; p < SM_R; ++p)
#pragma unroll
      for (int q = 0; q < SM_R; ++q) dot[p][q] = 0.0;
    for (int n0 = 0; n0 < N; n0 += SM_NC) {                     // workgroup-uniform
      const int nc_ = min(SM_NC, N - n0);
      if (s > 0 || n0 > 0) __syncthreads();                     // the previous chunk has been read
      for (int n = half; n < nc_; n += 2) sdst[n * SM_LD] = As[n0 + n] != 0.0 ? Es[n0 + n] * cs[n0 + n] : 0.0;
      __syncthreads();
      for (int n = 0; n < nc_; ++n) {
        double rv[SM_R], cv[SM_R];
#pragma unroll
        for (int q = 0; q < SM_R; ++q) { rv[q] = xr[n * SM_LD + ty + 16 * q]; cv[q] = xc[n * SM_LD + tx + 16 * q]; }
#pragma unroll
        for (int p = 0; p < SM_R; ++p)
#pragma unroll
          for (int q = 0; q < SM_R; ++q) dot[p][q] = dot[p][q] + rv[p] * cv[q];
      }
    }
    const double rs = 1.0 / (double)(s + 1);
#pragma unroll
    for (int p = 0; p < SM_R; ++p)
#pragma unroll
      for (int q = 0; q < SM_R; ++q) {
        const double pr = nr[p] * nc[q];
        const double c = pr == 0.0 ? 0.0 : dot[p][q] / dsqrt(pr);
        const double d = c - mu[p][q];
        mu[p][q] = mu[p][q] + d * rs;
        m2[p][q] = m2[p][q] + d * (c - mu[p][q]);
        cnt[p][q] += c >= a.min_cosine ? 1 : 0;
      }
  }
  const double dS = (double)a.S, dS1 = (double)(a.S - 1);
  const size_t plane = (size_t)a.nr * (size_t)m;
#pragma unroll
  for (int p = 0; p < SM_R; ++p) {
    const int r = r0 + ty + 16 * p;
    if (r >= a.nr) continue;
#pragma unroll
    for (int q = 0; q < SM_R; ++q) {
      const int c = c0 + tx + 16 * q;
      if (c >= m) continue;
      double* o = a.res + (size_t)r * (size_t)m + (size_t)c;
      o[0] = mu[p][q]; o[plane] = m2[p][q] / dS1; o[2 * plane] = (double)cnt[p][q] / dS;
    }
  }
}

// is candidate (v, j) ahead of (bv, bj) in the order mean descending, lower member first?  bj < 0: there is no (bv, bj) yet
__device__ __forceinline__ bool sim_ahead(double v, int j, double bv, int bj) { return bj < 0 || v > bv || (v == bv && j < bj); }

// One wave per row r of the band; `row0` is the band's first row in the whole row list (the outputs are indexed by row).
template <int>
__global__ __launch_bounds__(64) void k_sim_select(const double* res, const int* rows, int m, int nr, int row0, int k, int32_t* nat /* [rows][k] */,
                                                   double* nb /* [3][rows][k] */, size_t nbplane, double* tum /* [3][rows] */, size_t tumplane) {
  const int r = (int)blockIdx.x, lane = (int)threadIdx.x, self = rows[r];
  const size_t plane = (size_t)nr * (size_t)m, row = (size_t)(row0 + r);
  const double* mean = res + (size_t)r * (size_t)m;
  for (int t = lane; t < k; t += 64) {
    nat[row * k + t] = -1;
    nb[row * k + t] = BNMF_NAN; nb[nbplane + row * k + t] = BNMF_NAN; nb[2 * nbplane + row * k + t] = BNMF_NAN;
  }
  double tot = 0.0; int deg = 0;
  for (int j0 = 0; j0 < m; j0 += 1024) {                        // canonB: blocks of 1,024 members, each the canonical W = 64 sum
    const int j1 = min(j0 + 1024, m);
    double acc = 0.0;
    for (int j = j0 + lane; j < j1; j += 64) {
      acc = acc + (j == self ? 0.0 : mean[j]);
      deg += (j != self && mean[2 * plane + j] >= 0.5) ? 1 : 0;
    }
    tot = tot + wave_tree64(acc);                               // (lane 0's value is the sum)
  }
  for (int off = 32; off >= 1; off >>= 1) deg += __shfl_xor(deg, off);
  double pv = 0.0; int pj = -1;                                 // the previous pick
  double first = BNMF_NAN;
  const int rounds = k > 1 ? k : 1;
  for (int t = 0; t < rounds; ++t) {
    double bv = 0.0; int bj = -1;
    for (int j = lane; j < m; j += 64) {
      const double v = mean[j];
      if (j == self || v != v) continue;
      if (pj >= 0 && !(v < pv || (v == pv && j > pj))) continue;
      if (bj < 0 || v > bv) { bv = v; bj = j; }
    }
    for (int off = 32; off >= 1; off >>= 1) {
      const double ov = __shfl_xor(bv, off); const int oj = __shfl_xor(bj, off);
      if (oj >= 0 && sim_ahead(ov, oj, bv, bj)) { bv = ov; bj = oj; }
    }
    if (bj < 0) break;                                          // wave-uniform: every lane holds the same pick
    if (t == 0) first = bv;
    if (lane == 0 && t < k) {
      nat[row * k + t] = bj;
      nb[row * k + t] = bv; nb[nbplane + row * k + t] = mean[plane + bj]; nb[2 * nbplane + row * k + t] = mean[2 * plane + bj];
    }
    pv = bv; pj = bj;
  }
  if (lane == 0) { tum[row] = tot / (double)(m - 1); tum[tumplane + row] = first; tum[2 * tumplane + row] = (double)deg; }
}

}  // namespace bnmf
