// bayesnmf_amd/csrc/coactivity.h — co-activity of signatures over a recorded range: for every used sample of the record_sample rings and
// every pair of factors a < b the Pearson and the Spearman correlation of their loads across the included tumours, the phi coefficient
// of their presence and the cosine of their two columns of P, on the device (bnmf_coactivity / bnmf_coactivity_at).
// Reads the rings after the fact, as k_regress_moments does; no sweep kernel is involved and none of the chain's streams is consumed.
//
// Per used sample s (oldest first), included tumour g_i (the member list, ascending, m of them) and factor n, with cs_s[n] the bits of
// k_map_colsum:   x[n,i] = A_s[n] != 0 ? E_s[n,g_i] * cs_s[n] : +0.0.   canonB is regress.h's blocked canonical sum over the members.
//   means   k_coa_mean     the block partials of canonB_i(x[n,i]);   k_coa_mu: the blocks added, mu_n = . / m
//   pairs   k_coa_pairs    d = x - mu;  the block partials of S_ab = canonB_i(d_a,i d_b,i)  (a <= b), and per block the whole-number
//                          counts n11 = #(x_a >= min_load and x_b >= min_load)  (a == b: the count of factor a alone)
//   ranks   k_coa_rank     per (s, n): the m loads gathered, their keys sorted in the LDS (bitonic, padded with +Inf to a power of two),
//                          less = #(x_j < x_i) and equal = #(x_j == x_i) by a lower- and an upper-bound search, c = 2 less + equal - m
//           k_coa_sort, k_coa_search: the same through sorted chunks in the scratch (a cohort larger than one chunk; BNMF_COA_FORM=1)
//   T       k_coa_rsum     T_ab = sum_i c_a,i c_b,i in int64 (a <= b): whole numbers, the order is free
//   tail    k_coa_tail     the blocks added in order; v0 = S_ab / dsqrt(S_aa S_bb), v1 = T_ab / dsqrt(T_aa T_bb), v2 = phi
//   cosine  k_coa_cosine   v3 from P_s[, a] and P_s[, b], k ascending from +0.0 (k_ref_cosine's operations)
// The statistics over s are the host's (reduce_host.h).
//
// Tiling.  k_coa_mean and k_coa_pairs follow k_regress_moments: one wavefront per (block, sample, tile), lane l IS accumulator l and
// walks members l, l + 64, ... of its block, units of a block 8 apart in the grid (reg_unit).  A tile of k_coa_pairs is T factors a by T
// factors b with tile(a) <= tile(b): 2 T columns read, T T products (and T T counts) kept.  <4> is the form that runs, <2> the one
// BNMF_COA_FORM=1 forces: the same operations on the same values in the same order, hence the same bits.
// Every kernel is a template (plain kernels move the sweep's kernels apart in the code object).
#pragma once
#include "dmath.h"
#include "regress.h"
#include "sortnet.h"

namespace bnmf {

constexpr int CO_NSTAT = 4;          // statistics: pearson, spearman, co-presence, cosine
constexpr int CO_MAX_CHUNK = 16384;  // most doubles of a sorted chunk: 128 KB of LDS
constexpr int CO_MIN_CHUNK = 64;
struct CoaArgs {
  const double *ringE, *ringA, *ringP;   // record_sample rings: [slot][N*G], [slot][N], [slot][K*N]
  const double* cs;                      // [S][N]: k_map_colsum
  const int* slots;                      // ring slots of the used samples, oldest first
  const int* members;                    // [m]: the included tumours, ascending
  double* partM;                         // [Sb][nb][N]     block sums of x
  double* mu;                            // [Sb][N]
  double* partS;                         // [Sb][nb][N][N]  block sums of d_a d_b, a <= b
  int* partC;                            // [Sb][nb][N][N]  block counts n11, a <= b
  int* c;                                // [Sb][N][m]      2 midrank - (m + 1)
  double* sorted;                        // [Sb][N][nchunk][chunk]: the sorted chunks of the general form
  int* flag;                             // [Sb][N]: a load of the factor is not finite
  long long* T;                          // [Sb][N][N], a <= b
  double* ser;                           // [4][S][NP]: the whole range
  size_t lenE, lenP; int N, K, S, s0, m, nb, chunk, nchunk; double min_load;
};

// pair p of the a < b of N (a ascending, then b) -> (a, b);  tile pair p of the ta <= tb of nt -> (ta, tb)
BNMF_DEV void coa_pair(int p, int N, int& a, int& b) { a = 0; while (p >= N - 1 - a) { p -= N - 1 - a; ++a; } b = a + 1 + p; }
BNMF_DEV void coa_tile_pair(int p, int nt, int& ta, int& tb) { ta = 0; while (p >= nt - ta) { p -= nt - ta; ++ta; } tb = ta + p; }

BNMF_DEV long long wave_sum_i64(long long v) {   // every lane gets the sum over the wave: whole numbers, any order
  for (int o = 32; o >= 1; o >>= 1) {
    const int lo = __shfl_xor((int)v, o, 64), hi = __shfl_xor((int)(v >> 32), o, 64);
    v += (long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo);
  }
  return v;
}

// the loads of factor tile [n0, n0 + T) of member i; a copy of factor N - 1 beyond N (never stored)
template <int T>
BNMF_DEV void coa_loads(const CoaArgs& a, const double* Es, const double (&f)[T], const bool (&inc)[T], int n0, int i, double (&x)[T]) {
  const double* col = Es + (size_t)a.N * (size_t)a.members[i];
  double v[T];
#pragma unroll
  for (int t = 0; t < T; ++t) v[t] = col[min(n0 + t, a.N - 1)];
#pragma unroll
  for (int t = 0; t < T; ++t) x[t] = inc[t] ? v[t] * f[t] : 0.0;
}

template <int T>
__global__ __launch_bounds__(64) void k_coa_mean(CoaArgs a) {
  const int lane = (int)threadIdx.x, sb = (int)blockIdx.y, s = a.s0 + sb, N = a.N;
  int tile, b;
  if (!reg_unit((int)blockIdx.x, (N + T - 1) / T, a.nb, tile, b)) return;   // wave-uniform
  const int n0 = tile * T;
  const double* Es = a.ringE + (size_t)a.slots[s] * a.lenE;
  const double* As = a.ringA + (size_t)a.slots[s] * (size_t)N;
  const double* cs = a.cs + (size_t)s * N;
  double f[T], ax[T]; bool inc[T];
#pragma unroll
  for (int t = 0; t < T; ++t) { const int n = min(n0 + t, N - 1); inc[t] = As[n] != 0.0; f[t] = cs[n]; ax[t] = 0.0; }
  const int i1 = min((b + 1) * RG_BLOCK, a.m);
  for (int i = b * RG_BLOCK + lane; i < i1; i += 64) {
    double x[T];
    coa_loads<T>(a, Es, f, inc, n0, i, x);
#pragma unroll
    for (int t = 0; t < T; ++t) ax[t] = ax[t] + x[t];
  }
  double* o = a.partM + ((size_t)sb * a.nb + b) * N;
#pragma unroll
  for (int t = 0; t < T; ++t) {
    if (n0 + t >= N) continue;                     // wave-uniform
    const double v = wave_tree64(ax[t]);
    if (lane == 0) o[n0 + t] = v;
  }
}

// one lane per (sample of the batch, n): the blocks added in order, mu = . / m
template <int NS>
__global__ __launch_bounds__(64) void k_coa_mu(CoaArgs a, int Sb) {
  const size_t e = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (e >= (size_t)Sb * a.N) return;
  const size_t sb = e / a.N, n = e % a.N;
  const double* p = a.partM + sb * a.nb * a.N + n;
  double v = 0.0;
  for (int b = 0; b < a.nb; ++b) v = v + p[(size_t)b * a.N];
  a.mu[e] = v / (double)a.m;
}

template <int T>
__global__ __launch_bounds__(64) void k_coa_pairs(CoaArgs a) {
  const int lane = (int)threadIdx.x, sb = (int)blockIdx.y, s = a.s0 + sb, N = a.N;
  const int nt = (N + T - 1) / T;
  int tile, b;
  if (!reg_unit((int)blockIdx.x, nt * (nt + 1) / 2, a.nb, tile, b)) return;   // wave-uniform
  int ta, tb;
  coa_tile_pair(tile, nt, ta, tb);
  const int a0 = ta * T, b0 = tb * T;
  const double* Es = a.ringE + (size_t)a.slots[s] * a.lenE;
  const double* As = a.ringA + (size_t)a.slots[s] * (size_t)N;
  const double* cs = a.cs + (size_t)s * N;
  const double* mu = a.mu + (size_t)sb * N;
  double fa[T], fb[T], ma[T], mb[T]; bool ia[T], ib[T];
#pragma unroll
  for (int t = 0; t < T; ++t) {
    const int na = min(a0 + t, N - 1), nb = min(b0 + t, N - 1);
    ia[t] = As[na] != 0.0; fa[t] = cs[na]; ma[t] = mu[na];
    ib[t] = As[nb] != 0.0; fb[t] = cs[nb]; mb[t] = mu[nb];
  }
  double acc[T][T]; int cnt[T][T];
#pragma unroll
  for (int t = 0; t < T; ++t)
#pragma unroll
    for (int u = 0; u < T; ++u) { acc[t][u] = 0.0; cnt[t][u] = 0; }
  const int i1 = min((b + 1) * RG_BLOCK, a.m);
  for (int i = b * RG_BLOCK + lane; i < i1; i += 64) {
    double xa[T], xb[T], da[T], db[T];
    coa_loads<T>(a, Es, fa, ia, a0, i, xa);
    coa_loads<T>(a, Es, fb, ib, b0, i, xb);
#pragma unroll
    for (int t = 0; t < T; ++t) { da[t] = xa[t] - ma[t]; db[t] = xb[t] - mb[t]; }
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
      for (int u = 0; u < T; ++u) {
        acc[t][u] = acc[t][u] + da[t] * db[u];
        cnt[t][u] += (xa[t] >= a.min_load && xb[u] >= a.min_load) ? 1 : 0;
      }
  }
  const size_t at = ((size_t)sb * a.nb + b) * N * N;
#pragma unroll
  for (int t = 0; t < T; ++t)
#pragma unroll
    for (int u = 0; u < T; ++u) {
      if (a0 + t >= N || b0 + u >= N || a0 + t > b0 + u) continue;     // wave-uniform
      const double v = wave_tree64(acc[t][u]), k = wave_tree64((double)cnt[t][u]);   // the count: whole numbers <= 1,024, exact
      if (lane == 0) { a.partS[at + (size_t)(a0 + t) * N + b0 + u] = v; a.partC[at + (size_t)(a0 + t) * N + b0 + u] = (int)k; }
    }
}

// ---- the rank transform ----
// (coa_bitonic, coa_lower, coa_upper and coa_finite: sortnet.h, shared with summary.h)

// One workgroup per (factor, sample), a cohort of at most one chunk: n2 = the power of two >= max(m, 64) keys in the LDS.
template <int NT>
__global__ __launch_bounds__(NT) void k_coa_rank(CoaArgs a, int n2) {
  extern __shared__ __attribute__((aligned(16))) unsigned char coa_smem[];
  double* key = (double*)coa_smem;
  const int tid = (int)threadIdx.x, n = (int)blockIdx.x, sb = (int)blockIdx.y, s = a.s0 + sb, N = a.N, m = a.m;
  const double* Es = a.ringE + (size_t)a.slots[s] * a.lenE + n;
  const bool inc = a.ringA[(size_t)a.slots[s] * (size_t)N + n] != 0.0;
  const double f = a.cs[(size_t)s * N + n];
  int* c = a.c + ((size_t)sb * N + n) * (size_t)m;
  if (!inc) {                                      // uniform over the workgroup: every load is +0.0, every c is 0
    for (int i = tid; i < m; i += NT) c[i] = 0;
    if (tid == 0) a.flag[(size_t)sb * N + n] = 0;
    return;
  }
  int bad = 0;
  for (int i = tid; i < n2; i += NT) {
    double x = BNMF_INF;
    if (i < m) { x = Es[(size_t)N * (size_t)a.members[i]] * f; bad |= coa_finite(x) ? 0 : 1; }
    key[i] = x;
  }
  bad = __syncthreads_or(bad);
  coa_bitonic<NT>(key, n2, tid);
  if (tid == 0) a.flag[(size_t)sb * N + n] = bad ? 1 : 0;
  for (int i = tid; i < m; i += NT) {
    const double x = Es[(size_t)N * (size_t)a.members[i]] * f;
    const int less = coa_lower(key, n2, x), le = coa_upper(key, n2, x);
    c[i] = 2 * less + (le - less) - m;
  }
}

// The general form, pass 1: one workgroup per (factor, chunk, sample) leaves its chunk sorted in the scratch (the last padded with +Inf).
template <int NT>
__global__ __launch_bounds__(NT) void k_coa_sort(CoaArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char coa_smem[];
  double* key = (double*)coa_smem;
  const int tid = (int)threadIdx.x, n = (int)blockIdx.x % a.N, ch = (int)blockIdx.x / a.N, sb = (int)blockIdx.y, s = a.s0 + sb, N = a.N, m = a.m;
  const double* Es = a.ringE + (size_t)a.slots[s] * a.lenE + n;
  const bool inc = a.ringA[(size_t)a.slots[s] * (size_t)N + n] != 0.0;
  const double f = a.cs[(size_t)s * N + n];
  int bad = 0;
  for (int j = tid; j < a.chunk; j += NT) {
    const int i = ch * a.chunk + j;
    double x = BNMF_INF;
    if (i < m) { x = inc ? Es[(size_t)N * (size_t)a.members[i]] * f : 0.0; bad |= coa_finite(x) ? 0 : 1; }
    key[j] = x;
  }
  bad = __syncthreads_or(bad);
  coa_bitonic<NT>(key, a.chunk, tid);
  if (bad && tid == 0) atomicOr(a.flag + (size_t)sb * N + n, 1);        // (zeroed by the host before the launch)
  double* o = a.sorted + (((size_t)sb * N + n) * a.nchunk + ch) * (size_t)a.chunk;
  for (int j = tid; j < a.chunk; j += NT) o[j] = key[j];
}
// pass 2: one thread per (member, factor, sample) searches every sorted chunk
template <int NT>
__global__ __launch_bounds__(NT) void k_coa_search(CoaArgs a) {
  const int i = (int)blockIdx.x * NT + (int)threadIdx.x, n = (int)blockIdx.y, sb = (int)blockIdx.z, s = a.s0 + sb, N = a.N, m = a.m;
  if (i >= m) return;
  const bool inc = a.ringA[(size_t)a.slots[s] * (size_t)N + n] != 0.0;
  const double x = inc ? a.ringE[(size_t)a.slots[s] * a.lenE + n + (size_t)N * (size_t)a.members[i]] * a.cs[(size_t)s * N + n] : 0.0;
  const double* key = a.sorted + ((size_t)sb * N + n) * a.nchunk * (size_t)a.chunk;
  int less = 0, le = 0;
  for (int ch = 0; ch < a.nchunk; ++ch) {
    less += coa_lower(key + (size_t)ch * a.chunk, a.chunk, x);
    le += coa_upper(key + (size_t)ch * a.chunk, a.chunk, x);
  }
  a.c[((size_t)sb * N + n) * (size_t)m + i] = 2 * less + (le - less) - m;
}

// One wave per (tile pair, sample): T_ab = sum_i c_a,i c_b,i, an int64 accumulator per lane and product, then the wave's sum.
template <int T>
__global__ __launch_bounds__(64) void k_coa_rsum(CoaArgs a) {
  const int lane = (int)threadIdx.x, sb = (int)blockIdx.y, N = a.N, m = a.m;
  const int nt = (N + T - 1) / T;
  int ta, tb;
  coa_tile_pair((int)blockIdx.x, nt, ta, tb);
  const int a0 = ta * T, b0 = tb * T;
  const int* c = a.c + (size_t)sb * N * (size_t)m;
  long long acc[T][T];
#pragma unroll
  for (int t = 0; t < T; ++t)
#pragma unroll
    for (int u = 0; u < T; ++u) acc[t][u] = 0;
  for (int i = lane; i < m; i += 64) {
    int ca[T], cb[T];
#pragma unroll
    for (int t = 0; t < T; ++t) { ca[t] = c[(size_t)min(a0 + t, N - 1) * m + i]; cb[t] = c[(size_t)min(b0 + t, N - 1) * m + i]; }
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
      for (int u = 0; u < T; ++u) acc[t][u] += (long long)ca[t] * (long long)cb[u];
  }
#pragma unroll
  for (int t = 0; t < T; ++t)
#pragma unroll
    for (int u = 0; u < T; ++u) {
      if (a0 + t >= N || b0 + u >= N || a0 + t > b0 + u) continue;     // wave-uniform
      const long long v = wave_sum_i64(acc[t][u]);
      if (lane == 0) a.T[((size_t)sb * N + a0 + t) * N + b0 + u] = v;
    }
}

// one lane per (sample of the batch, pair): the blocks added in order, then v0, v1 and v2
template <int NS>
__global__ __launch_bounds__(64) void k_coa_tail(CoaArgs a, int Sb) {
  const int N = a.N, NP = N * (N - 1) / 2;
  const size_t e = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (e >= (size_t)Sb * NP) return;
  const int sb = (int)(e / NP), p = (int)(e % NP);
  int fa, fb;
  coa_pair(p, N, fa, fb);
  const size_t NN = (size_t)N * N, iab = (size_t)fa * N + fb, iaa = (size_t)fa * N + fa, ibb = (size_t)fb * N + fb;
  const double* ps = a.partS + (size_t)sb * a.nb * NN;
  const int* pc = a.partC + (size_t)sb * a.nb * NN;
  double sab = 0.0, saa = 0.0, sbb = 0.0;
  long long n11 = 0, n1x = 0, nx1 = 0;
  for (int b = 0; b < a.nb; ++b) {
    sab = sab + ps[b * NN + iab]; saa = saa + ps[b * NN + iaa]; sbb = sbb + ps[b * NN + ibb];
    n11 += pc[b * NN + iab]; n1x += pc[b * NN + iaa]; nx1 += pc[b * NN + ibb];
  }
  const size_t SNP = (size_t)a.S * NP, o = (size_t)(a.s0 + sb) * NP + p;
  const double den0 = saa * sbb;
  a.ser[o] = den0 > 0.0 ? sab / dsqrt(den0) : BNMF_NAN;
  const long long* T = a.T + (size_t)sb * NN;
  const long long tab = T[iab], taa = T[iaa], tbb = T[ibb];
  const bool ok = taa > 0 && tbb > 0 && !a.flag[(size_t)sb * N + fa] && !a.flag[(size_t)sb * N + fb];
  a.ser[SNP + o] = ok ? (double)tab / dsqrt((double)taa * (double)tbb) : BNMF_NAN;
  const long long m = a.m, n10 = n1x - n11, n01 = nx1 - n11, n00 = m - n1x - nx1 + n11, n0x = m - n1x, nx0 = m - nx1;
  const bool margins = n1x > 0 && n0x > 0 && nx1 > 0 && nx0 > 0;
  const double num = (double)n11 * (double)n00 - (double)n10 * (double)n01;
  a.ser[2 * SNP + o] = margins ? num / dsqrt(((double)n1x * (double)n0x) * ((double)nx1 * (double)nx0)) : BNMF_NAN;
}

// one lane per (pair, sample): dot, nn_a and nn_b over k ascending from +0.0, v3 = dot / dsqrt(nn_a nn_b); NaN where A_s excludes a or b
template <int NS>
__global__ __launch_bounds__(64) void k_coa_cosine(CoaArgs a) {
  const int N = a.N, NP = N * (N - 1) / 2, K = a.K, sb = (int)blockIdx.y, s = a.s0 + sb;
  const int p = (int)blockIdx.x * 64 + (int)threadIdx.x;
  if (p >= NP) return;
  int fa, fb;
  coa_pair(p, N, fa, fb);
  const double* P = a.ringP + (size_t)a.slots[s] * a.lenP;
  const double* As = a.ringA + (size_t)a.slots[s] * (size_t)N;
  const double *Pa = P + (size_t)K * fa, *Pb = P + (size_t)K * fb;
  double dot = 0.0, na = 0.0, nb = 0.0;
  for (int k = 0; k < K; ++k) { const double u = Pa[k], v = Pb[k]; dot = dot + u * v; na = na + u * u; nb = nb + v * v; }
  const bool inc = As[fa] != 0.0 && As[fb] != 0.0;
  a.ser[3 * (size_t)a.S * NP + (size_t)s * NP + p] = inc ? dot / dsqrt(na * nb) : BNMF_NAN;
}

}  // namespace bnmf
