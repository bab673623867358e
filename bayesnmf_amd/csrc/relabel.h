// bayesnmf_amd/csrc/relabel.h — label-switching correction of a recorded range: every used sample of the record_sample rings is aligned to
// a pivot by the permutation of its factors that maximises the total cosine, the pivot is iterated to the aligned mean, and the aligned
// mean and variance of the renormalised P and E are left with the permutations (bnmf_relabel / bnmf_relabel_at).  Reads
// the rings after the fact, as k_mixing and k_attr do; no sweep kernel is involved and none of the chain's streams is consumed.
//
// Over the used samples s = 0 .. S-1, oldest first, and ALL N factors, included or not (as bnmf_label_switching takes them).  pivot is
// K x N; round 1's is the caller's (or the newest used sample's P), round r + 1's the aligned mean of the renormalised P of round r.
//   refnorm2[j] = sum_k pivot[k,j] * pivot[k,j]                       k ascending from +0.0
//   C_s[n][j]   = dot / dsqrt(nn * refnorm2[j]),  dot = sum_k P_s[k,n] * pivot[k,j],  nn = sum_k P_s[k,n] * P_s[k,n]   (k_ref_cosine's
//                 operations on the raw P_s, k ascending from +0.0)
//   perm_s      = hungarian_wave(C_s, N, N): the assignment n -> j that maximises sum_n C_s[n][perm_s(n)], the lowest column among equals;
//                 cosine[s][n] = C_s[n][perm_s(n)];  inv_s(perm_s(n)) = n.  No assignment (a cosine is not finite): the sample is unmatched,
//                 perm = -1, cosine = NaN, it enters nothing below.  The aligned samples a = 0 .. S'-1 are the others, in order.
//   changed     = the aligned samples whose perm_s differs from the round before (round 1: from the identity).  A round with changed == 0,
//                 or round max_rounds, is the last.
//   cs_s[n]     = k_map_colsum;  x_s[k,n] = P_s[k,n] / cs_s[n],  e_s[n,g] = E_s[n,g] * cs_s[n]   (bnmf_map's renormalisation)
//   aligned series of element (k, j) of P: x_s[k, inv_s(j)];  of element (j, g) of E: e_s[inv_s(j), g];  over a = 0 .. S'-1
//   mu = canon(series) / S',  var = canon((series - mu)^2) / (S' - 1)   canon: accumulator l adds terms l, l + 64, ... ascending from +0.0,
//                 then wave_tree64 (mixing.h's expressions)
// Only + - * /, dsqrt and comparisons, associated as written: the bits depend on this alone, not on the tiling below.
//
// Tiling.  k_rl_match: one wave per sample, k_label_switch's shape; the N x N cosines and the solver's scratch in the LDS; it writes perm
// (over the previous round's, after comparing), inv, the cosines and a flag word per sample.  Past 160 KiB (N >= 141) the host runs
// k_ref_cosine + k_hungarian over chunks of samples and k_rl_finish writes the same words.  k_rl_compact (one wave) turns the flags into
// the list of aligned samples and two counts by ballots: the counts are all the host reads between rounds.  k_rl_accum: a wave owns
// RL_E = 8 consecutive elements of the output and lane l the canonical accumulator l of each, so the 64 lanes read 64 different samples
// and a lane's 8 loads of a sample fall into one 64-byte line of P (a column is contiguous, the permutation moves whole columns) or into
// the N-entry column of E that the permutation shuffles; the table (slot, sample, inv) of the aligned samples sits in the LDS, shared by
// the 16 waves of the workgroup (read from memory when it does not fit).  The mean, then (the last round) the variance in a second pass
// over the same loads; wave_tree64 at the end; no atomics, no waits.  k_rl_gather writes the aligned samples themselves.
#pragma once
#include "kernels.h"

namespace bnmf {

constexpr int RL_E = 8;              // consecutive elements of a wave of k_rl_accum: one 64-byte line of a sample
constexpr int RL_AT = 1024;          // threads of k_rl_accum: 16 waves share the table
constexpr int RL_NROW = 2;           // rows of the output: mean, variance (BNMF_NREL)
constexpr size_t RL_LDS = 160 * 1024;
constexpr size_t RL_TAB_LDS = 128 * 1024;   // the table is staged up to this size
inline size_t relabel_hung_lds(int N) { return (size_t)(N + 1) * (16 + 12) + (size_t)(N + 1) * 8; }
inline size_t relabel_match_lds(int N) { return (size_t)N * N * sizeof(double) + relabel_hung_lds(N); }
inline size_t relabel_tab_bytes(int S, int N) { return (size_t)S * (size_t)(N + 2) * sizeof(int); }

// the pivot (K x N column-major) as k_ref_cosine reads a catalogue: row-major [k][j], and the squared norms of its columns
__global__ __launch_bounds__(64) void k_rl_pivot(const double* piv, int K, int N, double* refT, double* refnorm2) {
  const int j = (int)blockIdx.x * 64 + (int)threadIdx.x;
  if (j >= N) return;
  double n2 = 0.0;
  for (int k = 0; k < K; ++k) { const double v = piv[(size_t)k + (size_t)K * j]; refT[(size_t)k * N + j] = v; n2 = n2 + v * v; }
  refnorm2[j] = n2;
}

// flag word of a sample: bit 0 aligned, bit 1 its permutation differs from the previous round's
// one sample per workgroup (one wave).  LDS: relabel_match_lds(N).
__global__ __launch_bounds__(64) void k_rl_match(const double* ringP, int K, int N, const int* slots, const double* refT, const double* refnorm2,
                                                  int first_round, int32_t* perm, int32_t* inv, double* cosine, int32_t* flag) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int s = blockIdx.x, lane = threadIdx.x;
  double* c = (double*)smem;                               // [N][N]
  const double* P = ringP + (size_t)slots[s] * (size_t)K * N;
  for (int e = lane; e < N * N; e += 64) {
    const int n = e / N, j = e - n * N;
    const double* Pn = P + (size_t)K * n;
    double dot = 0.0, nn = 0.0;
    for (int k = 0; k < K; ++k) { const double p = Pn[k]; dot = dot + p * refT[(size_t)k * N + j]; nn = nn + p * p; }
    c[e] = dot / dsqrt(nn * refnorm2[j]);
  }
  wave_lds_fence();
  const int* p = hungarian_wave(c, N, N, 0, smem + (size_t)N * N * sizeof(double));
  int32_t* pm = perm + (size_t)s * N;
  int32_t* iv = inv + (size_t)s * N;
  double* cs = cosine + (size_t)s * N;
  if (!p) {
    for (int n = lane; n < N; n += 64) { pm[n] = -1; iv[n] = -1; cs[n] = __builtin_nan(""); }
    if (lane == 0) flag[s] = 0;
    return;
  }
  int changed = 0;
  for (int j = lane + 1; j <= N; j += 64) {                // rows and columns are N each: every column has its row
    const int f = p[j] - 1;
    changed |= (first_round ? f : pm[f]) != j - 1 ? 1 : 0;
    pm[f] = j - 1; iv[j - 1] = f; cs[f] = c[(size_t)f * N + (j - 1)];
  }
  const int any = __any(changed);
  if (lane == 0) flag[s] = 1 | (any ? 2 : 0);
}
// the same words from k_ref_cosine + k_hungarian over a chunk of ns samples (the cosine matrix does not fit the LDS): cosv [s][N][N],
// col [s][N] (the column of every row, -1 where k_hungarian found no assignment); one thread per sample
__global__ __launch_bounds__(64) void k_rl_finish(const double* cosv, const int32_t* col, int N, int ns, int first_round, int32_t* perm, int32_t* inv,
                                                   double* cosine, int32_t* flag) {
  const int s = blockIdx.x * 64 + threadIdx.x;
  if (s >= ns) return;
  const int32_t* a = col + (size_t)s * N;
  int32_t* pm = perm + (size_t)s * N;
  int32_t* iv = inv + (size_t)s * N;
  double* cs = cosine + (size_t)s * N;
  bool ok = true;
  for (int n = 0; n < N; ++n) ok = ok && a[n] >= 0 && a[n] < N;
  if (!ok) {
    for (int n = 0; n < N; ++n) { pm[n] = -1; iv[n] = -1; cs[n] = __builtin_nan(""); }
    flag[s] = 0;
    return;
  }
  int changed = 0;
  for (int n = 0; n < N; ++n) {
    const int j = a[n];
    changed |= (first_round ? n : pm[n]) != j ? 1 : 0;
    pm[n] = j; iv[j] = n; cs[n] = cosv[((size_t)s * N + n) * N + j];
  }
  flag[s] = 1 | (changed ? 2 : 0);
}

// one wave: alist[a] = the a-th aligned sample, cnt[0] = S', cnt[1] = the aligned samples whose permutation changed.  Whole numbers,
// counted by ballots: no atomics.
__global__ __launch_bounds__(64) void k_rl_compact(const int32_t* flag, int S, int* alist, int* cnt) {
  const int lane = threadIdx.x;
  int na = 0, nc = 0;                                      // (the same value in every lane)
  for (int s0 = 0; s0 < S; s0 += 64) {
    const int s = s0 + lane;
    const int f = s < S ? flag[s] : 0;
    const unsigned long long ma = __ballot(f & 1), mc = __ballot((f & 3) == 3);
    if (f & 1) alist[na + __popcll(ma & ((1ull << lane) - 1ull))] = s;
    na += __popcll(ma); nc += __popcll(mc);
  }
  if (lane == 0) { cnt[0] = na; cnt[1] = nc; }
}

// The aligned mean (row 0 of out) and, with want_var, the aligned variance (row 1) of the renormalised P (SIDE 0) or E (SIDE 1).
// STAGE: the table [S'][N + 2] (ring slot, sample, inv) in the LDS.
template <int SIDE, bool STAGE>
__global__ __launch_bounds__(RL_AT) void k_rl_accum(const double* ring, size_t len, int K, int N, const int* slots, const int* alist, const int* cnt,
                                                     const int32_t* inv, const double* cs, int want_var, double* out /* [RL_NROW][len] */) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int Sa = cnt[0], W1 = N + 2;
  if constexpr (STAGE) {
    int* tab = (int*)smem;
    for (int e = tid; e < Sa * W1; e += RL_AT) {
      const int a = e / W1, q = e - a * W1, s = alist[a];
      tab[e] = q == 0 ? slots[s] : q == 1 ? s : inv[(size_t)s * N + (q - 2)];
    }
    __syncthreads();
  }
  const size_t e0 = ((size_t)blockIdx.x * (RL_AT / 64) + (size_t)wave) * RL_E;
  if (e0 >= len) return;                                   // wave-uniform; no barrier follows
  int nq[RL_E]; size_t off[RL_E];                          // the element's factor, and its offset apart from the factor
#pragma unroll
  for (int q = 0; q < RL_E; ++q) {                         // (a wave past the end repeats the last element and writes it once)
    const size_t ec = min(e0 + (size_t)q, len - 1);
    nq[q] = SIDE ? (int)(ec % (size_t)N) : (int)(ec / (size_t)K);
    off[q] = SIDE ? ec - (size_t)nq[q] : ec - (size_t)K * (size_t)nq[q];
  }
  const double dS = (double)Sa, dS1 = (double)(Sa - 1);
  double mu[RL_E];
  for (int pass = 0; pass < (want_var ? 2 : 1); ++pass) {
    double acc[RL_E];
#pragma unroll
    for (int q = 0; q < RL_E; ++q) acc[q] = 0.0;
    for (int a = lane; a < Sa; a += 64) {
      int slot, s, ns[RL_E];
      if constexpr (STAGE) {
        const int* row = (const int*)smem + (size_t)a * W1;
        slot = row[0]; s = row[1];
#pragma unroll
        for (int q = 0; q < RL_E; ++q) ns[q] = row[2 + nq[q]];
      } else {
        s = alist[a]; slot = slots[s];
#pragma unroll
        for (int q = 0; q < RL_E; ++q) ns[q] = inv[(size_t)s * N + nq[q]];
      }
      const double* Rs = ring + (size_t)slot * len;
      const double* cr = cs + (size_t)s * N;
      double v[RL_E], c[RL_E];
#pragma unroll
      for (int q = 0; q < RL_E; ++q) {                     // every load is made before the first use: 16 in flight per lane
        v[q] = Rs[off[q] + (SIDE ? (size_t)ns[q] : (size_t)K * (size_t)ns[q])];
        c[q] = cr[ns[q]];
      }
#pragma unroll
      for (int q = 0; q < RL_E; ++q) {
        const double x = SIDE ? v[q] * c[q] : v[q] / c[q];
        if (pass == 0) acc[q] = acc[q] + x;
        else { const double d = x - mu[q]; acc[q] = acc[q] + d * d; }
      }
    }
#pragma unroll
    for (int q = 0; q < RL_E; ++q) {
      const double r = wave_bcast0(wave_tree64(acc[q]));
      const double o = pass == 0 ? r / dS : r / dS1;
      if (pass == 0) mu[q] = o;
      if (lane == 0 && e0 + (size_t)q < len) out[(size_t)pass * len + e0 + (size_t)q] = o;
    }
  }
}

// the aligned samples themselves, for the used samples s0 .. s0 + nb - 1 of the range: out[s - s0][element]; an unmatched sample's row is NaN
template <int SIDE>
__global__ __launch_bounds__(256) void k_rl_gather(const double* ring, size_t len, int K, int N, const int* slots, const int32_t* inv, const int32_t* flag,
                                                    const double* cs, int s0, double* out) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= len) return;
  const int s = s0 + (int)blockIdx.y;
  double x = __builtin_nan("");
  if (flag[s] & 1) {
    const int n = SIDE ? (int)(e % (size_t)N) : (int)(e / (size_t)K);
    const int ns = inv[(size_t)s * N + n];
    const size_t src = SIDE ? e - (size_t)n + (size_t)ns : e - (size_t)K * (size_t)n + (size_t)K * (size_t)ns;
    const double v = ring[(size_t)slots[s] * len + src], c = cs[(size_t)s * N + ns];
    x = SIDE ? v * c : v / c;
  }
  out[(size_t)blockIdx.y * len + e] = x;
}

}  // namespace bnmf
