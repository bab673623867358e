// bayesnmf_amd/csrc/residuals.h — residual structure of a recorded range: for every used sample of the record_sample rings the
// standardised residuals of every cell, their K x K second-moment matrix over the included tumours, its leading component by power
// iteration and every tumour's score on it, on the device (bnmf_residuals / bnmf_residuals_at).  Reads the P, E, A (and
// sigmasq) rings and the data after the fact; no sweep kernel is involved, no random number is drawn and none of the chain's streams is
// consumed.
//
// Per used sample s (oldest first), member i (tumour g_i of the member list, ascending, m of them) and mutation type k, M the data cell
// as a double:
//   c = pre_N of reconstruction.h: pre_0 = +0.0, pre_{n+1} = pre_n + (P_s[k,n] * A_s[n]) * E_s[n,g], n ascending (waic.h's c_s, the same bits)
//   Poisson: lam = c < 1e-6 ? 1e-6 : c;  z = (M - lam) / dsqrt(lam)          Normal: z = (M - c) / dsqrt(sigmasq_s[g])
//   chi_s[i] = (sum_k z z) / K                                               k ascending from +0.0
//   b_s[k]   = canonB_i(z[k,i]) / m                                          canonB: regress.h's blocked canonical sum over the positions i
//   C_s[k,k'] = canonB_i(z[k,i] * z[k',i]) / m  for k' <= k, mirrored        the product rounded, then added
//   q_s[k] = C_s[k,k];  tr_s = sum_k C_s[k,k]                                k ascending from +0.0
// The leading component of C_s (k_res_power; the host runs the same routine on the mean matrix, reduce_host.h):
//   k* the largest diagonal element, the first wins;  y = C[:,k*];  nn = sum_k y[k] y[k];  v = y / dsqrt(nn)
//   n_steps times:  y[k] = sum_k' C[k,k'] v[k']  (k' ascending from +0.0, multiply and add rounded separately);  nn and v as before
//   once more y = C v:  lambda = sum_k v[k] y[k];  nn = sum_k y[k] y[k];  move = max_k |y[k] / dsqrt(nn) - v[k]|  (from +0.0, d > mx ? d : mx)
//   v is flipped so that its element of largest magnitude (the first wins) is positive;  share = lambda / tr
//   flat: tr is not > 0 and finite, or one of the nn (the last included) is not: the sample enters nothing over the samples
//   t_s[i] = sum_k v[k] z[k,i]                                               k ascending from +0.0
// Over the samples that are not flat, numbered j = 0, 1, ... in order: gram = canon64_j(C_s) / S' (accumulator j & 63 of every element
// is continued batch after batch, then the halving tree).  Every other statistic over the samples is the host's (reduce_host.h).
//
// Tiling.  z passes through the scratch once per batch of samples, k-major ([k][i]: a wave's read of one row is contiguous), K m doubles
// per sample; the Gram pass reads it back through the caches (DESIGN.md §26 says why it is not rebuilt per tile).
//   k_res_z<NORMAL, NT>  a lane owns a member and its k loop is the order of chi; the rows x[k][.] = P_s[k,.] A_s of k_rec_x are
//                        wave-uniform.  NT > 0: the lane's column of E_s in registers, NT = ceil(N / 8) * 8 <= 32 is the row stride of x,
//                        the places N .. NT - 1 hold +0.0 twice (pre + 0.0 * 0.0 is pre: never -0.0, reconstruction.h).  NT = 0: any N,
//                        the column read through the caches.
//   k_res_gram<T>        one wave per (pair of tiles of T types, sample): lane l IS accumulator l and walks positions l, l + 64, ... of a
//                        block of RG_BLOCK; after each block the T T trees (wave_tree64) and lane t T + u adds the block sum of product
//                        (t, u) to its total, so the blocks are added ascending.  <8> is the form that runs, <4> the one BNMF_RES_FORM=1
//                        forces (with k_res_z<., 0>): the same operations on the same values in the same order, hence the same bits.
//   k_res_b              one wave per (k, sample), the same walk
//   k_res_power          a workgroup per sample, v and y in the LDS; thread k owns row k (read as column k: C_s is bitwise symmetric, and
//                        adjacent threads read adjacent places); the sums over k are thread 0's loops
//   k_res_score          a lane per member
//   k_res_accum, k_res_mean   a thread per element of the mean matrix
// No atomics, no polling, no scratch memory, no MFMA (its fused rounding is not the spec's).  Every kernel is a template.
#pragma once
#include "dmath.h"
#include "regress.h"
#include "coactivity.h"   // coa_tile_pair

namespace bnmf {

constexpr int RS_NTYPE = 5, RS_NCOMP = 4, RS_NTUM = 3, RS_NSER = 5;
constexpr int RS_MAX_K = 2048;     // most mutation types: v and y of k_res_power are 2 K doubles of LDS
constexpr int RS_MAX_NT = 32;      // factors whose column of E stays in registers
constexpr int RS_T = 256;          // threads of k_res_z, k_res_power and k_res_score
struct ResArgs {
  const double *ringE, *ringS;     // record_sample rings: [slot][N*G], [slot][G] (Normal; else null)
  const double* xg;                // [Sb][K][NS]: k_rec_x
  const double* Mt;                // [K][G]: k_rec_data
  const int* slots;                // ring slots of the used samples, oldest first
  const int* members;              // [m]: the included tumours, ascending
  double* z;                       // [Sb][K][m]
  double* chi;                     // [Sb][m]
  double* t;                       // [Sb][m]
  double* C;                       // [Sb][K][K]
  double *b, *q, *v;               // [S][K] each: the whole range
  double* ser;                     // [4][S]: tr, lambda, share, move
  int* flat;                       // [S]
  size_t lenE; int K, N, NS, G, m, S, s0, n_steps;
};

template <bool NORMAL, int NT>
__global__ __launch_bounds__(RS_T) void k_res_z(ResArgs a) {
  const int i = (int)blockIdx.x * RS_T + (int)threadIdx.x, sb = (int)blockIdx.y, K = a.K, N = a.N, m = a.m;
  if (i >= m) return;
  const size_t slot = (size_t)a.slots[a.s0 + sb], g = (size_t)a.members[i];
  const double* Es = a.ringE + slot * a.lenE + (size_t)N * g;
  const double* xs = a.xg + (size_t)sb * (size_t)K * (size_t)a.NS;
  const double* Mg = a.Mt + g;
  double* zo = a.z + (size_t)sb * (size_t)K * (size_t)m + (size_t)i;
  double sd = 1.0;
  if constexpr (NORMAL) sd = dsqrt(a.ringS[slot * (size_t)a.G + g]);
  double e[NT > 0 ? NT : 1];
  if constexpr (NT > 0) {
#pragma unroll
    for (int n = 0; n < NT; ++n) e[n] = n < N ? Es[n] : 0.0;
  }
  double chi = 0.0;
  for (int k = 0; k < K; ++k) {
    double p = 0.0;
    if constexpr (NT > 0) {
      const double* row = xs + (size_t)k * NT;
#pragma unroll
      for (int n = 0; n < NT; ++n) p = p + row[n] * e[n];
    } else {
      const double* row = xs + (size_t)k * (size_t)N;
      for (int n = 0; n < N; ++n) p = p + row[n] * Es[n];
    }
    const double M = Mg[(size_t)k * (size_t)a.G];
    double zz;
    if constexpr (NORMAL) zz = (M - p) / sd;
    else { const double lam = p < 1e-6 ? 1e-6 : p; zz = (M - lam) / dsqrt(lam); }
    zo[(size_t)k * (size_t)m] = zz;
    chi = chi + zz * zz;
  }
  a.chi[(size_t)sb * m + i] = chi / (double)K;
}

// one wave per (k, sample): b_s[k] = canonB_i(z[k,i]) / m
template <int>
__global__ __launch_bounds__(64) void k_res_b(ResArgs a) {
  const int lane = (int)threadIdx.x, k = (int)blockIdx.x, sb = (int)blockIdx.y, m = a.m;
  const double* zr = a.z + ((size_t)sb * a.K + k) * (size_t)m;
  double tot = 0.0;
  for (int i0 = 0; i0 < m; i0 += RG_BLOCK) {       // wave-uniform
    const int i1 = min(i0 + RG_BLOCK, m);
    double acc = 0.0;
    for (int i = i0 + lane; i < i1; i += 64) acc = acc + zr[i];
    tot = tot + wave_tree64(acc);                  // (lane 0's is the sum)
  }
  if (lane == 0) a.b[(size_t)(a.s0 + sb) * a.K + k] = tot / (double)m;
}

template <int T>
__global__ __launch_bounds__(64) void k_res_gram(ResArgs a) {
  static_assert(T * T <= 64, "lane t T + u holds the total of product (t, u)");
  const int lane = (int)threadIdx.x, sb = (int)blockIdx.y, K = a.K, m = a.m;
  const int nt = (K + T - 1) / T;
  int ta, tb;
  coa_tile_pair((int)blockIdx.x, nt, ta, tb);      // ta <= tb
  const int a0 = ta * T, b0 = tb * T;
  const double* zs = a.z + (size_t)sb * (size_t)K * (size_t)m;
  const double *ra[T], *rb[T];
#pragma unroll
  for (int t = 0; t < T; ++t) {                    // a copy of type K - 1 beyond K (never stored)
    ra[t] = zs + (size_t)min(a0 + t, K - 1) * (size_t)m;
    rb[t] = zs + (size_t)min(b0 + t, K - 1) * (size_t)m;
  }
  double tot = 0.0;                                // of product (lane / T, lane % T)
  for (int i0 = 0; i0 < m; i0 += RG_BLOCK) {       // wave-uniform
    const int i1 = min(i0 + RG_BLOCK, m);
    double acc[T][T];
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
      for (int u = 0; u < T; ++u) acc[t][u] = 0.0;
    for (int i = i0 + lane; i < i1; i += 64) {
      double za[T], zb[T];
#pragma unroll
      for (int t = 0; t < T; ++t) { za[t] = ra[t][i]; zb[t] = rb[t][i]; }
#pragma unroll
      for (int t = 0; t < T; ++t)
#pragma unroll
        for (int u = 0; u < T; ++u) acc[t][u] = acc[t][u] + za[t] * zb[u];
    }
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
      for (int u = 0; u < T; ++u) {
        if (a0 + t >= K || b0 + u >= K || a0 + t > b0 + u) continue;       // wave-uniform
        const double v = __shfl(wave_tree64(acc[t][u]), 0, 64);
        tot = lane == t * T + u ? tot + v : tot;
      }
  }
  const int t = lane / T, u = lane % T, ka = a0 + t, kb = b0 + u;
  if (lane >= T * T || ka >= K || kb >= K || ka > kb) return;
  double* Cs = a.C + (size_t)sb * (size_t)K * (size_t)K;
  const double c = tot / (double)m;
  Cs[(size_t)ka * K + kb] = c;
  Cs[(size_t)kb * K + ka] = c;
}

// A workgroup per sample.  sh: v [K], y [K].
template <int>
__global__ __launch_bounds__(RS_T) void k_res_power(ResArgs a) {
  extern __shared__ double rs_lds[];
  __shared__ double s_r, s_tr;
  __shared__ int s_ks, s_flat;
  const int tid = (int)threadIdx.x, sb = (int)blockIdx.x, s = a.s0 + sb, K = a.K;
  const double* Cs = a.C + (size_t)sb * (size_t)K * (size_t)K;
  double *v = rs_lds, *y = rs_lds + K;
  if (tid == 0) {
    double tr = 0.0, best = Cs[0];
    int at = 0;
    for (int k = 0; k < K; ++k) {
      const double d = Cs[(size_t)k * K + k];
      tr = tr + d;
      if (d > best) { best = d; at = k; }
    }
    s_tr = tr; s_ks = at; s_flat = (tr > 0.0 && tr < BNMF_INF) ? 0 : 1;
  }
  __syncthreads();
  for (int k = tid; k < K; k += RS_T) {
    y[k] = Cs[(size_t)s_ks * K + k];               // (column k* is row k*: bitwise symmetric)
    a.q[(size_t)s * K + k] = Cs[(size_t)k * K + k];
  }
  __syncthreads();
  double lambda = BNMF_NAN, move = BNMF_NAN;
  for (int step = 0; step <= a.n_steps + 1; ++step) {          // workgroup-uniform
    // y holds C v (step 0: the start column).  nn, and unless this is the further product, v = y / dsqrt(nn)
    const bool further = step == a.n_steps + 1;
    if (tid == 0) {
      double nn = 0.0;
      for (int k = 0; k < K; ++k) nn = nn + y[k] * y[k];
      if (!(nn > 0.0 && nn < BNMF_INF)) s_flat = 1;
      s_r = dsqrt(nn);
      if (further) {
        double l = 0.0, mx = 0.0;
        for (int k = 0; k < K; ++k) l = l + v[k] * y[k];
        for (int k = 0; k < K; ++k) { const double d = dabs(y[k] / s_r - v[k]); mx = d > mx ? d : mx; }
        lambda = l; move = mx;
      }
    }
    __syncthreads();
    if (s_flat || further) break;
    const double r = s_r;
    for (int k = tid; k < K; k += RS_T) v[k] = y[k] / r;
    __syncthreads();
    for (int k = tid; k < K; k += RS_T) {
      double acc = 0.0;
      for (int j = 0; j < K; ++j) acc = acc + Cs[(size_t)j * K + k] * v[j];
      y[k] = acc;
    }
    __syncthreads();
  }
  if (tid == 0) {
    int at = 0;
    double big = dabs(v[0]);
    for (int k = 1; k < K; ++k) { const double d = dabs(v[k]); if (d > big) { big = d; at = k; } }
    s_ks = v[at] < 0.0 ? 1 : 0;
    const bool fl = s_flat != 0;
    a.flat[s] = fl ? 1 : 0;
    a.ser[s] = fl ? BNMF_NAN : s_tr;
    a.ser[(size_t)a.S + s] = fl ? BNMF_NAN : lambda;
    a.ser[2 * (size_t)a.S + s] = fl ? BNMF_NAN : lambda / s_tr;
    a.ser[3 * (size_t)a.S + s] = fl ? BNMF_NAN : move;
  }
  __syncthreads();
  const bool flip = s_ks != 0, fl = s_flat != 0;
  for (int k = tid; k < K; k += RS_T) a.v[(size_t)s * K + k] = fl ? BNMF_NAN : (flip ? -v[k] : v[k]);
}

// a lane per (member, sample): t_s[i] = sum_k v_s[k] z[k,i]
template <int>
__global__ __launch_bounds__(RS_T) void k_res_score(ResArgs a) {
  const int i = (int)blockIdx.x * RS_T + (int)threadIdx.x, sb = (int)blockIdx.y, K = a.K, m = a.m;
  if (i >= m) return;
  const double* vs = a.v + (size_t)(a.s0 + sb) * K;
  const double* zc = a.z + (size_t)sb * (size_t)K * (size_t)m + (size_t)i;
  double t = 0.0;
  for (int k = 0; k < K; ++k) t = t + vs[k] * zc[(size_t)k * (size_t)m];
  a.t[(size_t)sb * m + i] = t;
}

// a thread per element e of the K K: the batch's samples that are not flat are added to the 64 accumulators acc [64][K K] of the
// canonical sum over the samples, sample j of them to accumulator j & 63 (zeroed by the host before the first batch)
template <int>
__global__ __launch_bounds__(256) void k_res_accum(const double* C, const int* flat, int s0, int nb, size_t KK, double* acc) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= KK) return;
  int j = 0;
  for (int s = 0; s < s0; ++s) j += flat[s] ? 0 : 1;
  for (int s = 0; s < nb; ++s) {
    if (flat[s0 + s]) continue;
    double* p = acc + (size_t)(j & 63) * KK + e;
    *p = *p + C[(size_t)s * KK + e];
    ++j;
  }
}
// the halving tree over the accumulators (in place), gram = . / S'
template <int>
__global__ __launch_bounds__(256) void k_res_mean(const int* flat, int S, size_t KK, double* acc, double* gram) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= KK) return;
  int Sp = 0;
  for (int s = 0; s < S; ++s) Sp += flat[s] ? 0 : 1;
  for (int h = 32; h >= 1; h >>= 1)
    for (int l = 0; l < h; ++l) acc[(size_t)l * KK + e] = acc[(size_t)l * KK + e] + acc[(size_t)(l + h) * KK + e];
  gram[e] = acc[e] / (double)Sp;
}

}  // namespace bnmf
