// bayesnmf_amd/csrc/subtypes.h — subtypes of tumours over a recorded range: for every used sample of the record_sample rings a Lloyd
// iteration (k-means) of the included tumours' share profiles from one common start, and from the labels of all samples the membership
// counts and the consensus rows, on the device (bnmf_subtypes / bnmf_subtypes_at).  Reads the E and A rings and
// k_map_colsum's column sums of P after the fact; no sweep kernel is involved, no random number is drawn and none of the chain's streams
// is consumed.
//
// Per matched used sample s (oldest first) and member i (the included tumours g_0 < g_1 < ..., m of them), cs_s[n] the bits of k_map_colsum:
//   x[n]  = A_s[n] != 0 ? E_s[n,g_i] * cs_s[n] : +0.0         contrast.h's x, the same bits
//   t     = sum_n x[n]   n ascending from +0.0;   unassigned (label -1, dmin +0.0, no count) unless t > 0 && t < inf
//   u = 1 / t;   r[n] = x[n] * u;   q[perm_s[n]] = r[n]       the aligned share profile
// A Lloyd step, mu [N][C] column-major from centres0:
//   assign  d(i,c) = sum_j (q[j] - mu[j,c]) * (q[j] - mu[j,c])  j ascending from +0.0;  label = 0, dmin = d(i,0);  c = 1 .. C-1 replaces
//           them only if d(i,c) < dmin
//   update  n_c = #(label == c);  mu[j,c] = canonB_i(label_i == c ? q_i[j] : +0.0) / n_c  where n_c > 0      (regress.h's canonB over
//           the positions of the member list)
// repeated until a step changes no label (step 1 compares with all -1) or n_steps are run; then inertia = canonB_i(dmin_i).
// The bits depend on the samples, used[], the member list, perm and centres0 only: not on the form, the tile, the number of waves or the
// batch of samples that passes through the scratch.
//
//   k_subtypes   one workgroup of SB_T lanes owns one sample and runs all its steps; only workgroup barriers.  The centres, the factors'
//                cs / A / inverse perm and the block partials are in the LDS; labels, dmin and u in the scratch ([sample of the batch][m]).
//                assign: a lane per member, strided; the column E_s[., g] is read once for t and once per chunk of SB_DC clusters
//                (from the L1), with the chunk's distances in registers, j the outer loop: every d is summed j ascending.
//                update: wave w owns blocks w, w + SB_W, ... of RG_BLOCK member positions; lane l IS accumulator l of the block's
//                canonical sum and walks positions l, l + 64, ...; a tile is TJ factors x TC clusters of accumulators in registers
//                (a non-member of c adds +0.0, which leaves a non-negative accumulator's bits alone).  After every round of SB_W
//                blocks one lane per (j, c) of the tile adds the round's block sums in ascending order to its running sum.
//                <8, 4> with one tile (N <= 8, C <= 4) is the form for small N C; <4, 8> the tiled one for any N C <= 128 x 32, which
//                BNMF_SUB_FORM=1 forces.  The same operations on the same values in the same order: the same bits.
//   k_sub_count  whole numbers only: blockIdx.y = 0 a lane per member adds the batch's samples to cnt [C][m] and assigned [m];
//                blockIdx.y = 1 + q a lane per member adds to together [Q][m] and both [Q][m].  A lane owns its cells: no atomics.
//                The queries go in slices of SB_QSLICE launches' worth (the grid's y is 16 bits wide).
// No grid synchronisation, no atomics, no polling, no scratch memory, no MFMA.
#pragma once
#include "dmath.h"
#include "regress.h"

namespace bnmf {

constexpr int SB_T = 512;               // lanes of k_subtypes
constexpr int SB_W = SB_T / 64;         // its waves: the blocks of a round
constexpr int SB_MAX_N = 128;
constexpr int SB_MAX_C = 32;
constexpr int SB_DC = 8;                // clusters of a chunk of distances
constexpr int SB_MAX_TILE = 32;         // most accumulators of a tile
constexpr int SB_NCROW = 4;             // mean, variance, lower, upper
constexpr int SB_NTUM = 3;              // certainty, share of samples assigned, runner-up membership
constexpr int SB_NSER = 3;              // inertia, steps, assigned tumours
constexpr int SB_QSLICE = 65534;        // most queries of one launch of k_sub_count

struct SubArgs {
  const double *ringE, *ringA;          // record_sample rings: [slot][N*G], [slot][N]
  const double* cs;                     // [S][N]: k_map_colsum
  const int* slots;                     // ring slots of the matched used samples, oldest first
  const int* members;                   // [m]: the included tumours, ascending
  const int* perm;                      // [S][N]: the aligned place of factor n
  const double* centres0;               // [N][C] column-major
  int32_t* lab;                         // [batch][m]
  double *dmin, *u;                     // [batch][m]
  double* centre;                       // [S][N*C]
  int32_t* size;                        // [S][C]
  double* inertia;                      // [S]
  int32_t *steps, *assigned, *changed;  // [S]; changed: labels changed in the last step run
  size_t lenE; int N, C, m, n_steps, s0;   // s0: the first sample of the batch
};

template <int TJ, int TC>
__global__ __launch_bounds__(SB_T) void k_subtypes(SubArgs a) {
  static_assert(TJ * TC <= SB_MAX_TILE && TJ * TC <= SB_T, "the tile");
  __shared__ double mu[SB_MAX_N * SB_MAX_C];
  __shared__ double fcs[SB_MAX_N];
  __shared__ double part[SB_W][SB_MAX_TILE];
  __shared__ int cpart[SB_W][SB_MAX_TILE];
  __shared__ int finc[SB_MAX_N], inv[SB_MAX_N], cnt[SB_MAX_C];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, N = a.N, C = a.C, m = a.m;
  const int sb = (int)blockIdx.x, s = a.s0 + sb;
  const double* Es = a.ringE + (size_t)a.slots[s] * a.lenE;
  int32_t* lab = a.lab + (size_t)sb * (size_t)m;
  double* dmin = a.dmin + (size_t)sb * (size_t)m;
  double* us = a.u + (size_t)sb * (size_t)m;
  for (int n = tid; n < N; n += SB_T) {
    fcs[n] = a.cs[(size_t)s * N + n];
    finc[n] = a.ringA[(size_t)a.slots[s] * (size_t)N + n] != 0.0 ? 1 : 0;
    inv[a.perm[(size_t)s * N + n]] = n;                        // (a permutation of 0 .. N-1: checked on the host)
  }
  for (int e = tid; e < N * C; e += SB_T) mu[e] = a.centres0[e];
  for (int i = tid; i < m; i += SB_T) lab[i] = -1;
  __syncthreads();
  const int nb = (m + RG_BLOCK - 1) / RG_BLOCK;
  int steps = 0, changed = 0;
  for (int step = 0; step < a.n_steps; ++step) {               // workgroup-uniform
    // ---- assign ----
    int mine = 0;
    for (int i = tid; i < m; i += SB_T) {
      const double* col = Es + (size_t)N * (size_t)a.members[i];
      double t = 0.0;
      for (int n = 0; n < N; ++n) t = t + (finc[n] ? col[n] * fcs[n] : 0.0);
      int best = -1; double bd = 0.0, u = 0.0;
      if (t > 0.0 && t < BNMF_INF) {
        u = 1.0 / t;
        for (int c0 = 0; c0 < C; c0 += SB_DC) {
          double d[SB_DC];
#pragma unroll
          for (int k = 0; k < SB_DC; ++k) d[k] = 0.0;
          for (int j = 0; j < N; ++j) {
            const int n = inv[j];
            const double x = finc[n] ? col[n] * fcs[n] : 0.0;
            const double q = x * u;
#pragma unroll
            for (int k = 0; k < SB_DC; ++k) {
              const double df = q - mu[j + N * min(c0 + k, C - 1)];
              d[k] = d[k] + df * df;
            }
          }
#pragma unroll
          for (int k = 0; k < SB_DC; ++k) {
            if (c0 + k >= C) continue;
            if (c0 + k == 0) { best = 0; bd = d[0]; }
            else if (d[k] < bd) { best = c0 + k; bd = d[k]; }
          }
        }
      }
      mine |= lab[i] != best ? 1 : 0;
      lab[i] = best; dmin[i] = bd; us[i] = u;
    }
    changed = __syncthreads_or(mine);                          // the labels are written: the update reads them
    // ---- update ----
    for (int c0 = 0; c0 < C; c0 += TC)
      for (int j0 = 0; j0 < N; j0 += TJ) {
        double run = 0.0; int crun = 0;
        for (int b0 = 0; b0 < nb; b0 += SB_W) {
          const int b = b0 + wave;
          if (b < nb) {                                        // wave-uniform
            double acc[TJ][TC]; int ac[TC];
#pragma unroll
            for (int k = 0; k < TC; ++k) {
              ac[k] = 0;
#pragma unroll
              for (int t = 0; t < TJ; ++t) acc[t][k] = 0.0;
            }
            const int i1 = min((b + 1) * RG_BLOCK, m);
            for (int i = b * RG_BLOCK + lane; i < i1; i += 64) {
              const double* col = Es + (size_t)N * (size_t)a.members[i];
              const int l = lab[i];
              const double u = us[i];
              double q[TJ];
#pragma unroll
              for (int t = 0; t < TJ; ++t) {
                const int n = inv[min(j0 + t, N - 1)];
                const double x = finc[n] ? col[n] * fcs[n] : 0.0;
                q[t] = x * u;
              }
#pragma unroll
              for (int k = 0; k < TC; ++k) {
                const bool in = l == c0 + k;
                ac[k] += in ? 1 : 0;
#pragma unroll
                for (int t = 0; t < TJ; ++t) acc[t][k] = acc[t][k] + (in ? q[t] : 0.0);
              }
            }
#pragma unroll
            for (int k = 0; k < TC; ++k) {
#pragma unroll
              for (int t = 0; t < TJ; ++t) {
                const double v = wave_tree64(acc[t][k]);
                if (lane == 0) part[wave][t * TC + k] = v;
              }
              if (j0 == 0) {
                int v = ac[k];
                for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
                if (lane == 0) cpart[wave][k] = v;
              }
            }
          }
          __syncthreads();
          const int nw = min(SB_W, nb - b0);
          if (tid < TJ * TC) for (int w = 0; w < nw; ++w) run = run + part[w][tid];
          if (j0 == 0 && tid < TC) for (int w = 0; w < nw; ++w) crun += cpart[w][tid];
          __syncthreads();
        }
        if (j0 == 0) {
          if (tid < TC && c0 + tid < C) cnt[c0 + tid] = crun;
          __syncthreads();
        }
        if (tid < TJ * TC) {
          const int j = j0 + tid / TC, c = c0 + tid % TC;
          if (j < N && c < C && cnt[c] > 0) mu[j + N * c] = run / (double)cnt[c];
        }
      }
    __syncthreads();
    steps = step + 1;
    if (!changed) break;
  }
  // ---- the sample's results: the centres, the sizes, the inertia of the last assignment ----
  for (int e = tid; e < N * C; e += SB_T) a.centre[(size_t)s * N * C + e] = mu[e];
  for (int c = tid; c < C; c += SB_T) a.size[(size_t)s * C + c] = cnt[c];
  double run = 0.0; int crun = 0;
  for (int b0 = 0; b0 < nb; b0 += SB_W) {
    const int b = b0 + wave;
    if (b < nb) {
      double acc = 0.0; int ac = 0;
      const int i1 = min((b + 1) * RG_BLOCK, m);
      for (int i = b * RG_BLOCK + lane; i < i1; i += 64) { acc = acc + dmin[i]; ac += lab[i] >= 0 ? 1 : 0; }
      const double v = wave_tree64(acc);
      for (int off = 32; off >= 1; off >>= 1) ac += __shfl_xor(ac, off);
      if (lane == 0) { part[wave][0] = v; cpart[wave][0] = ac; }
    }
    __syncthreads();
    const int nw = min(SB_W, nb - b0);
    if (tid == 0) for (int w = 0; w < nw; ++w) { run = run + part[w][0]; crun += cpart[w][0]; }
    __syncthreads();
  }
  if (tid == 0) { a.inertia[s] = run; a.steps[s] = steps; a.assigned[s] = crun; a.changed[s] = changed ? 1 : 0; }
}

// (no template parameter is used: a template only for its place in the code object, behind every kernel that exists)
template <int>
__global__ __launch_bounds__(256) void k_sub_count(const int32_t* lab /* [ns][m] */, int ns, int m, int C, const int* qplace /* [Q] */, int32_t* cnt /* [C][m] */,
                                                   int32_t* assigned /* [m] */, int32_t* together /* [Q][m] */, int32_t* both /* [Q][m] */, int counts) {
  const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (i >= m) return;
  if (blockIdx.y == 0) {
    if (!counts) return;                                          // a further slice of queries: the batch's counts are taken
    int na = 0;
    for (int s = 0; s < ns; ++s) {
      const int l = lab[(size_t)s * m + i];
      if (l >= 0 && l < C) { ++na; cnt[(size_t)l * m + i] += 1; }
    }
    assigned[i] += na;
  } else {
    const int q = (int)blockIdx.y - 1, p = qplace[q];
    int nt = 0, nbo = 0;
    for (int s = 0; s < ns; ++s) {
      const int lq = lab[(size_t)s * m + p], l = lab[(size_t)s * m + i];
      nbo += (lq >= 0 && l >= 0) ? 1 : 0;
      nt += (lq >= 0 && lq == l) ? 1 : 0;
    }
    together[(size_t)q * m + i] += nt; both[(size_t)q * m + i] += nbo;
  }
}

}  // namespace bnmf
