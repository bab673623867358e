// bayesnmf_amd/csrc/decompose.h — decomposition of the recorded signatures into a reference catalogue: for every used sample of the
// record_sample rings the KL (EM / multiplicative-update) refit of every renormalised column of P to the K x R catalogue, pruned to the
// references that carry a share, on the device (bnmf_decompose / bnmf_decompose_at).  The mirror of project.h: there the
// dictionary varies per sample and the data are fixed, here the data (the columns of P_s) vary per sample and the dictionary is fixed
// for the whole call.  Reads the P and A rings after the fact; no sweep kernel is involved and no random number is drawn.
//
// Host, once: rs[r] = sum_k ref[k,r] (k ascending from +0.0), z[k,r] = ref[k,r] / rs[r].
// Per used sample s (oldest first) and factor n:
//   cs[n]  = k_map_colsum's column sum of P_s[, n];  the factor takes part iff keep[n] != 0, A_s[n] != 0 and cs[n] > 0; one that does not
//            has every weight +0.0, a NaN cosine, 0.0 for the other fit values and nactive = 0, and its column is never read
//   y[k]   = P_s[k,n] / cs[n];   t = sum_k y[k]                       k ascending from +0.0
//   stage 1: w_r = t / (double)R, then n_steps times
//              for k ascending:  c = sum_r z[k,r] * w_r (r ascending from +0.0);  q = c > 0 ? y[k] / c : 0.0;
//                                g_r = g_r + z[k,r] * q (each g_r from +0.0)
//              then w_r = w_r * g_r;   d = max_r |w_r(new) - w_r(old)| (from +0.0, v > d ? v : d)
//   pruning (skipped when min_share == 0.0: every reference is active and the call ends after stage 1):
//            r is active iff w_r >= min_share * t; if none is, the one with the largest w_r (from r = 0, v > best: the first wins a
//            tie); every inactive reference gets w_r = +0.0 for good
//   stage 2: n_steps more updates from the weights as they stand; w_r of an inactive reference is re-selected to +0.0 at every update,
//            whatever g_r became: z is finite and c is never -0.0, so z * (+0.0) leaves c bit for bit and the references are carried
//            under a mask, not skipped
//   change = d / t                                                    d of the last step performed
//   with c_k of the final w:  dot = sum_k y c, yy = sum_k y y, cc = sum_k c c, l1 = sum_k |y - c|   (k ascending from +0.0)
//   cosine = dot / dsqrt(yy * cc);   rel_l1 = l1 / t;   nactive = the number of active references
//   w_s[r,n] in the scratch [Sb][R][N]: attribution.h's k_attr_share and k_attr_stats (N := R, G := N, min_load := min_share) make the
//   four weight rows of it, project.h's k_proj_fit (J := N) the three fit rows, k_proj_exposures (N := R, J := N) every sample's weights.
// The bits depend on the samples, used[], keep[], the catalogue, n_steps and min_share only: not on the batch size or the form of the kernel.
//
// Tiling: a lane owns one problem (s, n) of the batch, p = s N + n; adjacent lanes own adjacent n, so the stores to the scratch are
// contiguous and z is wave-uniform.  k_dec_y leaves the flags and y k-major ([k][p], +0.0 for a factor that takes no part: a wave's reads of
// one row are contiguous).  k_decompose<RT, STAGE> is k_project's update (project.h's kl_row) with the roles of x and X exchanged:
//   RT > 0: w and g in registers, RT = ceil(R / 8) * 8 <= 32 of each, the row stride of z is RT; the places R .. RT - 1 hold z = +0.0
//           and are never active.  256 threads per workgroup.
//   RT = 0: w and g in lane-private LDS columns [R][64] (a lane reads its own 8 bytes of a row of 512: no bank conflict), R up to
//           DC_MAX_R.  64 threads per workgroup.
//   STAGE:  the workgroup copies z to the LDS once and the lanes read it as broadcasts; else every lane reads z through the caches at
//           wave-uniform addresses (scalar loads): the same values.  Measured at the headline shape the staged catalogue
//           beside the columns leaves one wave per CU and takes 1.8 times as long, so the host stages only when BNMF_DEC_STAGE = 1 asks.
// The active set is a lane's own: a bit per reference in two 64-bit words.
#pragma once
#include "project.h"

namespace bnmf {

constexpr int DC_MAX_R = PJ_MAX_N;   // references at all; DC_MAX_R <= 128: two words of mask
constexpr int DC_NFIT = PJ_NFIT;     // fit rows: mean cosine, mean relative L1 error, largest last-step change

// A thread per (k, p) of the batch, p = s N + n: part[p] and yt[k][p] = P_s[k,n] / cs[n], +0.0 where the factor takes no part (its column
// is not read).
__global__ __launch_bounds__(256) void k_dec_y(const double* ringP, const double* ringA, size_t lenP, int K, int N, int Pn, const int* slots,
                                               const double* cs /* [Sb][N] */, const int* keep /* [N] */, double* yt /* [K][Pn] */,
                                               int* part /* [Pn] */) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (size_t)K * (size_t)Pn) return;
  const int k = (int)(e / (size_t)Pn), p = (int)(e % (size_t)Pn), s = p / N, n = p - s * N;
  const size_t slot = (size_t)slots[s];
  const double c = cs[p];
  const bool in = keep[n] != 0 && ringA[slot * (size_t)N + n] != 0.0 && c > 0.0;
  yt[e] = in ? ringP[slot * lenP + (size_t)k + (size_t)K * n] / c : 0.0;
  if (k == 0) part[p] = in ? 1 : 0;
}

template <int RT, bool STAGE>
__global__ __launch_bounds__(RT > 0 ? PJ_T : PJ_TL) void k_decompose(const double* __restrict__ zg /* [K][RS] */, const double* __restrict__ yt /* [K][Pn] */,
                                                                      const int* __restrict__ part /* [Pn] */, int K, int R, int N, int Pn, int n_steps,
                                                                      double min_share, double* __restrict__ scr /* [Sb][R][N] */,
                                                                      double* __restrict__ fitscr /* [Sb][3][N] */, int* __restrict__ nact /* [Pn] */) {
  constexpr bool REG = RT > 0;
  constexpr int T = REG ? PJ_T : PJ_TL;
  extern __shared__ double dc_lds[];
  const int tid = (int)threadIdx.x;
  const int p = (int)blockIdx.x * T + tid;
  const bool ok = p < Pn;
  const int pc = ok ? p : Pn - 1;                  // a lane past the end repeats the last problem and stores nothing
  const int RS = REG ? RT : R;
  const int ni = REG ? RT : R;                     // places the loops visit
  double* wl = dc_lds + tid;                       // RT = 0: w[i] at wl[i * T], g[i] at gl[i * T]
  double* gl = wl + (size_t)(REG ? 0 : R) * T;
  const double* zs = zg;
  if constexpr (STAGE) {
    double* zl = dc_lds + (REG ? 0 : 2 * (size_t)R * T);
    for (int e = tid; e < K * RS; e += T) zl[e] = zg[e];
    __syncthreads();
    zs = zl;
  }
  double wr[REG ? RT : 1], gr[REG ? RT : 1];
  auto W = [&](int i) -> double& { if constexpr (REG) return wr[i]; else return wl[(size_t)i * T]; };
  auto G = [&](int i) -> double& { if constexpr (REG) return gr[i]; else return gl[(size_t)i * T]; };
  const double* yp = yt + pc;
  double t = 0.0;
  for (int k = 0; k < K; ++k) t = t + yp[(size_t)k * Pn];
  // the lane's active set: every reference in stage 1 (the idle places R .. RT - 1 never)
  unsigned long long m0 = R >= 64 ? ~0ull : (1ull << R) - 1ull, m1 = R > 64 ? (R >= 128 ? ~0ull : (1ull << (R - 64)) - 1ull) : 0ull;
  auto active = [&](int i) -> bool { return ((i < 64 ? m0 >> i : m1 >> (i - 64)) & 1ull) != 0ull; };
  const double w0 = t / (double)R;
#pragma unroll
  for (int i = 0; i < ni; ++i) W(i) = i < R ? w0 : 0.0;
  double d = 0.0;
  const int n_stages = min_share != 0.0 ? 2 : 1;
  for (int stage = 0; stage < n_stages; ++stage) {
    if (stage == 1) {                              // pruning
      const double thr = min_share * t;
      unsigned long long a0 = 0ull, a1 = 0ull;
      double best = 0.0; int bi = 0;
#pragma unroll
      for (int i = 0; i < ni; ++i) {
        const double v = W(i);
        if (i < R && v >= thr) { if (i < 64) a0 |= 1ull << i; else a1 |= 1ull << (i - 64); }
        if (i == 0) best = v;
        else if (i < R && v > best) { best = v; bi = i; }
      }
      if ((a0 | a1) == 0ull) { if (bi < 64) a0 = 1ull << bi; else a1 = 1ull << (bi - 64); }
      m0 = a0; m1 = a1;
#pragma unroll
      for (int i = 0; i < ni; ++i) W(i) = active(i) ? W(i) : 0.0;
    }
    for (int step = 0; step < n_steps; ++step) {
#pragma unroll
      for (int i = 0; i < ni; ++i) G(i) = 0.0;
      for (int k = 0; k < K; ++k) kl_row<RT>(zs + (size_t)k * RS, yp[(size_t)k * Pn], R, W, G);
      d = 0.0;
#pragma unroll
      for (int i = 0; i < ni; ++i) {
        const double wo = W(i), wn = active(i) ? wo * G(i) : 0.0;
        const double v = fabs(wn - wo);
        d = v > d ? v : d;
        W(i) = wn;
      }
    }
  }
  double dot = 0.0, yy = 0.0, cc = 0.0, l1 = 0.0;
  for (int k = 0; k < K; ++k) {
    const double y = yp[(size_t)k * Pn];
    const double c = kl_fitted<RT>(zs + (size_t)k * RS, R, W);
    dot = dot + y * c; yy = yy + y * y; cc = cc + c * c; l1 = l1 + fabs(y - c);
  }
  if (!ok) return;
  const bool in = part[p] != 0;
  const int s = p / N, n = p - s * N;
  double* f = fitscr + (size_t)s * DC_NFIT * (size_t)N + (size_t)n;
  f[0] = in ? dot / dsqrt(yy * cc) : __builtin_nan("");
  f[(size_t)N] = in ? l1 / t : 0.0;
  f[2 * (size_t)N] = in ? d / t : 0.0;
  nact[p] = in ? __popcll(m0) + __popcll(m1) : 0;
  double* a = scr + (size_t)s * (size_t)R * (size_t)N + (size_t)n;
#pragma unroll
  for (int i = 0; i < ni; ++i) if (i < R) a[(size_t)i * N] = in ? W(i) : 0.0;
}

}  // namespace bnmf
