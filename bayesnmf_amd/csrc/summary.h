// bayesnmf_amd/csrc/summary.h — cohort summary of signatures over a recorded range: for every used sample of the record_sample rings and
// every factor how its load is distributed across the included tumours: prevalence, total, fraction of the cohort's load, mean among the
// carriers, and exact order statistics (type-7 quantiles at the levels probs[]) of all loads, of the carriers' loads and of the shares, on
// the device (bnmf_summary / bnmf_summary_at).  Reads the rings after the fact, as k_coa_rank does; no sweep kernel is
// involved and none of the chain's streams is consumed.
//
// Per aligned sample s (oldest first), included tumour g_i (the member list, ascending, m of them) and factor n, with cs_s[n] the bits of
// k_map_colsum:   x[n,i] = (A_s[n] != 0 ? E_s[n,g_i] * cs_s[n] : +0.0) + 0.0    (the + 0.0 turns a -0.0 into +0.0: ties carry one pattern)
//   totals  k_sum_total    t_i = sum_n x[n,i], n ascending from +0.0;  u_i = t_i > 0 ? 1 / t_i : 0.0        (one lane per member: the scratch)
//   scalars k_sum_scalar   the block partials of canonB_i(x) and canonB_i(x >= min_load ? x : +0.0) and the block counts #(x >= min_load)
//           k_sum_tail     the blocks added in order; prevalence, total, fraction, mean_present
//   order   k_sum_rank     per (s, n): the m loads gathered, sorted in the LDS (bitonic, padded with +Inf to a power of two), c = m - #(key <
//                          min_load), the quantiles of key[0, m) and of its suffix key[m - c, m); then the same LDS sorts the shares
//                          r_i = x[n,i] * u_i + 0.0 and gives theirs
//           k_sum_sort, k_sum_select: the same through sorted chunks in the scratch (a cohort larger than one chunk; BNMF_SUM_CHUNK): every
//                          wanted order statistic by bisection on the value, #(key <= v) summed over the chunks — exact, the same bits
// A value goes to the place of its label perm[s][n].  The statistics over s are the host's (reduce_host.h).
// The workgroup that sorts reads t through u (the first small kernel forms it), it does not recompute the sum over n per key.
// Every kernel is a template (plain kernels move the sweep's kernels apart in the code object).
#pragma once
#include "dmath.h"
#include "regress.h"
#include "sortnet.h"

namespace bnmf {

constexpr int SM_NSCAL = 4;          // scalar statistics: prevalence, total, fraction, mean_present
constexpr int SM_MAX_Q = 8;          // most levels
constexpr int SM_MAX_CHUNK = 16384;  // most doubles of a sorted chunk: 128 KB of LDS
constexpr int SM_MIN_CHUNK = 64;
constexpr int SM_WIDTH = 1024;       // threads of the sorting workgroup
struct SumArgs {
  const double *ringE, *ringA;           // record_sample rings: [slot][N*G], [slot][N]
  const double* cs;                      // [S][N]: k_map_colsum
  const int* slots;                      // ring slots of the aligned samples, oldest first
  const int* members;                    // [m]: the included tumours, ascending
  const int* perm;                       // [S][N]: the label of factor n in sample s
  double* u;                             // [Sb][m]       1 / t, or 0.0
  double* part;                          // [Sb][nb][N][2] block sums of x and of the carriers' x
  int* partC;                            // [Sb][nb][N]   block counts of the carriers
  double* sorted;                        // [2][Sb][N][nchunk][chunk]: the sorted chunks of the general form, loads then shares
  int* flag;                             // [S][N]: a load or a share of the factor is not finite
  double* ser;                           // [NSTAT][S][N]: the whole range
  const double* probs;                   // [L] the levels, ascending
  size_t lenE; int N, S, Sb, s0, m, nb, chunk, nchunk, L; double min_load;
};

BNMF_DEV double sum_x(bool inc, double e, double f) { return (inc ? e * f : 0.0) + 0.0; }
// map_interp on the ascending y[0 .. k), k >= 1, at level p in [0, 1]
BNMF_DEV void sum_level(int k, double p, int& j, int& j1, double& g) {
  const double h = (double)(k - 1) * p;
  j = (int)h;                                      // floor: h >= 0
  g = h - (double)j;
  j1 = min(j + 1, k - 1);
}
BNMF_DEV double sum_interp(double a, double b, double g) { return a == b ? a : (1.0 - g) * a + g * b; }
BNMF_DEV void sum_put(const SumArgs& a, int q, int sb, int n, double v) {
  const size_t s = (size_t)(a.s0 + sb);
  a.ser[((size_t)q * a.S + s) * a.N + a.perm[s * a.N + n]] = v;
}

// one lane per (member, sample of the batch)
template <int NT>
__global__ __launch_bounds__(NT) void k_sum_total(SumArgs a) {
  const int i = (int)blockIdx.x * NT + (int)threadIdx.x, sb = (int)blockIdx.y, s = a.s0 + sb, N = a.N;
  if (i >= a.m) return;
  const double* col = a.ringE + (size_t)a.slots[s] * a.lenE + (size_t)N * (size_t)a.members[i];
  const double* As = a.ringA + (size_t)a.slots[s] * (size_t)N;
  const double* cs = a.cs + (size_t)s * N;
  double t = 0.0;
  for (int n = 0; n < N; ++n) t = t + sum_x(As[n] != 0.0, col[n], cs[n]);
  a.u[(size_t)sb * a.m + i] = t > 0.0 ? 1.0 / t : 0.0;
}

// one wavefront per (block, sample, tile of T factors), as k_coa_mean: lane l IS accumulator l of canonB's block
template <int T>
__global__ __launch_bounds__(64) void k_sum_scalar(SumArgs a) {
  const int lane = (int)threadIdx.x, sb = (int)blockIdx.y, s = a.s0 + sb, N = a.N;
  int tile, b;
  if (!reg_unit((int)blockIdx.x, (N + T - 1) / T, a.nb, tile, b)) return;   // wave-uniform
  const int n0 = tile * T;
  const double* Es = a.ringE + (size_t)a.slots[s] * a.lenE;
  const double* As = a.ringA + (size_t)a.slots[s] * (size_t)N;
  const double* cs = a.cs + (size_t)s * N;
  double f[T], ax[T], ap[T]; bool inc[T]; int cnt[T];
#pragma unroll
  for (int t = 0; t < T; ++t) { const int n = min(n0 + t, N - 1); inc[t] = As[n] != 0.0; f[t] = cs[n]; ax[t] = 0.0; ap[t] = 0.0; cnt[t] = 0; }
  const int i1 = min((b + 1) * RG_BLOCK, a.m);
  for (int i = b * RG_BLOCK + lane; i < i1; i += 64) {
    const double* col = Es + (size_t)N * (size_t)a.members[i];
    double v[T];
#pragma unroll
    for (int t = 0; t < T; ++t) v[t] = col[min(n0 + t, N - 1)];
#pragma unroll
    for (int t = 0; t < T; ++t) {
      const double x = sum_x(inc[t], v[t], f[t]);
      const bool on = x >= a.min_load;
      ax[t] = ax[t] + x;
      ap[t] = ap[t] + (on ? x : 0.0);
      cnt[t] += on ? 1 : 0;
    }
  }
  const size_t at = ((size_t)sb * a.nb + b) * N;
#pragma unroll
  for (int t = 0; t < T; ++t) {
    if (n0 + t >= N) continue;                     // wave-uniform
    const double v0 = wave_tree64(ax[t]), v1 = wave_tree64(ap[t]), k = wave_tree64((double)cnt[t]);   // the count: whole numbers <= 1,024, exact
    if (lane == 0) { a.part[(at + n0 + t) * 2] = v0; a.part[(at + n0 + t) * 2 + 1] = v1; a.partC[at + n0 + t] = (int)k; }
  }
}

// one lane per sample of the batch: the blocks added in order; the fraction's denominator is the totals added with n ascending
template <int NS>
__global__ __launch_bounds__(64) void k_sum_tail(SumArgs a, int ns) {
  const int sb = (int)blockIdx.x * 64 + (int)threadIdx.x, N = a.N;
  if (sb >= ns) return;
  const double* p = a.part + (size_t)sb * a.nb * N * 2;
  const int* pc = a.partC + (size_t)sb * a.nb * N;
  double den = 0.0;
  for (int n = 0; n < N; ++n) {
    double tot = 0.0;
    for (int b = 0; b < a.nb; ++b) tot = tot + p[((size_t)b * N + n) * 2];
    den = den + tot;
  }
  for (int n = 0; n < N; ++n) {
    double tot = 0.0, pre = 0.0; int c = 0;
    for (int b = 0; b < a.nb; ++b) { tot = tot + p[((size_t)b * N + n) * 2]; pre = pre + p[((size_t)b * N + n) * 2 + 1]; c += pc[(size_t)b * N + n]; }
    sum_put(a, 0, sb, n, (double)c / (double)a.m);
    sum_put(a, 1, sb, n, tot);
    sum_put(a, 2, sb, n, den > 0.0 ? tot / den : BNMF_NAN);
    sum_put(a, 3, sb, n, c > 0 ? pre / (double)c : BNMF_NAN);
  }
}

// One workgroup per (factor, sample), a cohort of at most one chunk: n2 = the power of two >= max(m, 64) keys in the LDS, first the
// loads, then the shares.
template <int NT>
__global__ __launch_bounds__(NT) void k_sum_rank(SumArgs a, int n2) {
  extern __shared__ __attribute__((aligned(16))) unsigned char sum_smem[];
  double* key = (double*)sum_smem;
  const int tid = (int)threadIdx.x, n = (int)blockIdx.x, sb = (int)blockIdx.y, s = a.s0 + sb, N = a.N, m = a.m, L = a.L;
  const double* Es = a.ringE + (size_t)a.slots[s] * a.lenE + n;
  const bool inc = a.ringA[(size_t)a.slots[s] * (size_t)N + n] != 0.0;
  const double f = a.cs[(size_t)s * N + n];
  const double* u = a.u + (size_t)sb * m;
  int bad = 0;
  for (int i = tid; i < n2; i += NT) {
    double x = BNMF_INF;
    if (i < m) {
      x = sum_x(inc, Es[(size_t)N * (size_t)a.members[i]], f);
      const double r = x * u[i] + 0.0;
      bad |= (coa_finite(x) && coa_finite(r)) ? 0 : 1;
    }
    key[i] = x;
  }
  bad = __syncthreads_or(bad);
  coa_bitonic<NT>(key, n2, tid);
  if (tid == 0) a.flag[(size_t)s * N + n] = bad ? 1 : 0;
  if (tid < 2 * L) {                               // load_all[l], then load_present[l]
    const int l = tid % L, present = tid / L;
    const int c = m - coa_lower(key, m, a.min_load), k = present ? c : m, off = present ? m - c : 0;
    double v = BNMF_NAN;
    if (k > 0 && !bad) { int j, j1; double g; sum_level(k, a.probs[l], j, j1, g); v = sum_interp(key[off + j], key[off + j1], g); }
    sum_put(a, SM_NSCAL + present * L + l, sb, n, v);
  }
  __syncthreads();                                 // the loads are read: the keys become the shares
  for (int i = tid; i < n2; i += NT) {
    double r = BNMF_INF;
    if (i < m) r = sum_x(inc, Es[(size_t)N * (size_t)a.members[i]], f) * u[i] + 0.0;
    key[i] = r;
  }
  __syncthreads();
  coa_bitonic<NT>(key, n2, tid);
  if (tid < L) {
    double v = BNMF_NAN;
    if (!bad) { int j, j1; double g; sum_level(m, a.probs[tid], j, j1, g); v = sum_interp(key[j], key[j1], g); }
    sum_put(a, SM_NSCAL + 2 * L + tid, sb, n, v);
  }
}

// The general form, pass 1: one workgroup per (factor, chunk, sample, family) leaves its chunk sorted in the scratch (the last padded
// with +Inf).  blockIdx.z: 0 the loads, 1 the shares.
template <int NT>
__global__ __launch_bounds__(NT) void k_sum_sort(SumArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char sum_smem[];
  double* key = (double*)sum_smem;
  const int tid = (int)threadIdx.x, n = (int)blockIdx.x % a.N, ch = (int)blockIdx.x / a.N, sb = (int)blockIdx.y, fam = (int)blockIdx.z;
  const int s = a.s0 + sb, N = a.N, m = a.m;
  const double* Es = a.ringE + (size_t)a.slots[s] * a.lenE + n;
  const bool inc = a.ringA[(size_t)a.slots[s] * (size_t)N + n] != 0.0;
  const double f = a.cs[(size_t)s * N + n];
  const double* u = a.u + (size_t)sb * m;
  int bad = 0;
  for (int j = tid; j < a.chunk; j += NT) {
    const int i = ch * a.chunk + j;
    double v = BNMF_INF;
    if (i < m) {
      const double x = sum_x(inc, Es[(size_t)N * (size_t)a.members[i]], f), r = x * u[i] + 0.0;
      bad |= (coa_finite(x) && coa_finite(r)) ? 0 : 1;
      v = fam ? r : x;
    }
    key[j] = v;
  }
  bad = __syncthreads_or(bad);
  coa_bitonic<NT>(key, a.chunk, tid);
  if (bad && tid == 0) atomicOr(a.flag + (size_t)s * N + n, 1);          // (zeroed by the host before the launch)
  double* o = a.sorted + ((((size_t)fam * a.Sb + sb) * N + n) * a.nchunk + ch) * (size_t)a.chunk;
  for (int j = tid; j < a.chunk; j += NT) o[j] = key[j];
}

// doubles <-> unsigned keys of the same order (no NaN is mapped: the bisection stays inside [-Inf, +Inf])
BNMF_DEV unsigned long long sum_okey(double x) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(x);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
BNMF_DEV double sum_oval(unsigned long long k) {
  const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  return __longlong_as_double((long long)b);
}
// the order statistic of rank r (from 0) of the keys of nchunk sorted chunks: the smallest v with #(key <= v) > r, by bisection on the
// value.  Every rank asked for is below m and the pads are +Inf, so the answer is a key; a key is never -0.0, and -0.0 is the value below
// +0.0 in the order of the bisection, so + 0.0 returns the key's own bits.
BNMF_DEV double sum_select(const double* key, int nchunk, int chunk, int r) {
  unsigned long long lo = sum_okey(-BNMF_INF), hi = sum_okey(BNMF_INF);
  while (lo < hi) {
    const unsigned long long mid = lo + ((hi - lo) >> 1);
    const double v = sum_oval(mid);
    long long cnt = 0;
    for (int ch = 0; ch < nchunk; ++ch) cnt += coa_upper(key + (size_t)ch * chunk, chunk, v);
    if (cnt > (long long)r) hi = mid; else lo = mid + 1;
  }
  return sum_oval(lo) + 0.0;
}
// pass 2: one wave per (factor, sample); lane t < 3 L takes one family and level: load_all, load_present, share_all
template <int NT>
__global__ __launch_bounds__(NT) void k_sum_select(SumArgs a) {
  const int tid = (int)threadIdx.x, n = (int)blockIdx.x, sb = (int)blockIdx.y, s = a.s0 + sb, N = a.N, m = a.m, L = a.L;
  if (tid >= 3 * L) return;
  const int l = tid % L, fam = tid / L;            // 0 load_all, 1 load_present, 2 share_all
  const size_t run = (size_t)a.nchunk * (size_t)a.chunk;
  const double* key = a.sorted + ((((size_t)(fam == 2 ? 1 : 0)) * a.Sb + sb) * N + n) * run;
  int k = m, off = 0;
  if (fam == 1) {
    int less = 0;
    for (int ch = 0; ch < a.nchunk; ++ch) less += coa_lower(key + (size_t)ch * a.chunk, a.chunk, a.min_load);   // (the pads are +Inf: never below)
    k = m - less; off = less;
  }
  double v = BNMF_NAN;
  if (k > 0 && !a.flag[(size_t)s * N + n]) {
    int j, j1; double g;
    sum_level(k, a.probs[l], j, j1, g);
    const double ya = sum_select(key, a.nchunk, a.chunk, off + j), yb = j1 == j ? ya : sum_select(key, a.nchunk, a.chunk, off + j1);
    v = sum_interp(ya, yb, g);
  }
  sum_put(a, SM_NSCAL + fam * L + l, sb, n, v);
}

}  // namespace bnmf
