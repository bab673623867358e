// bayesnmf_amd/csrc/project.h — exposures of new tumours under the recorded signatures: for every used sample of the record_sample
// rings the KL (EM / multiplicative-update) refit of every column of a second data matrix X (K x J) to the sample's renormalised
// signatures, on the device (bnmf_project / bnmf_project_at).  Reads the P and A rings after the fact; no sweep kernel
// is involved, no random number is drawn and none of the chain's streams is consumed.
//
// Per used sample s (oldest first) and new tumour j:
//   cs[n]  = k_map_colsum's column sum of P_s[, n];   x[k,n] = P_s[k,n] / cs[n]   (bnmf_map's renormalisation)
//   factor n takes part iff A_s[n] != 0 and cs[n] > 0;  N_in = the number that do;  every other factor is skipped in every sum
//   below and has e_n = +0.0
//   t      = sum_k X[k,j]                               k ascending from +0.0
//   e_n    = t / (double)N_in
//   n_steps times:   for k ascending:  c = sum_n x[k,n] * e_n (n ascending from +0.0);  q = c > 0 ? X[k,j] / c : 0.0;
//                                      g_n = g_n + x[k,n] * q (each g_n from +0.0)
//                    then e_n = e_n * g_n;   d = max_n |e_n(new) - e_n(old)| (from +0.0, v > d ? v : d)
//   change = t > 0 ? d / t : 0.0                        d of the last step
//   with c_k of the final e:  dot = sum_k X c, xx = sum_k X X, cc = sum_k c c, l1 = sum_k |X - c|   (k ascending from +0.0)
//   cosine = dot / dsqrt(xx * cc)  (NaN by IEEE for an all-zero tumour or fit);   rel_l1 = t > 0 ? l1 / t : 0.0
//   a_s[n,j] = e_n  in the scratch [Sb][N][J]: attribution.h's k_attr_share and k_attr_stats (G := J) make load and series of it
// fit[0][j] = (sum_s cosine) / S, fit[1][j] = (sum_s rel_l1) / S (s ascending from +0.0), fit[2][j] = max_s change (from +0.0).
// The bits depend on the samples, used[], X and n_steps only: not on a tumour's place j, the batch size or the form of the kernel.
//
// Tiling: a lane owns one problem (s, j); adjacent lanes own adjacent j of one sample, so x is wave-uniform.  k_proj_x first leaves
// per sample the list of the factors that take part and their columns of x side by side (row k: x[k, idx[0]], x[k, idx[1]], ...,
// then +0.0 up to the row stride), so that the refit loops over N_in factors and never touches an excluded column: an Inf or NaN in
// one cannot reach c.  k_project<NT, STAGE>:
//   NT > 0: e and g in registers, NT = ceil(N / 8) * 8 <= 32 of each, the row stride is NT.  The places N_in .. NT - 1 hold x = +0.0
//           and e = +0.0 (e is re-selected to +0.0 at every update, whatever g became): c + 0.0 * 0.0 is c, bit for bit, since c is
//           never -0.0.  256 threads per workgroup.
//   NT = 0: e and g in lane-private LDS columns [N_in][64], N up to PJ_MAX_N; the loops run to N_in.  64 threads per workgroup.
//   STAGE:  the workgroup copies the sample's K rows of x to the LDS once and the lanes read them as broadcasts; else every lane reads
//           x through the caches at wave-uniform addresses (scalar loads): the same values.  Measured at the headline shape with e, g
//           in registers the uniform reads are the faster form, so the host stages x only beside e, g in the LDS, and
//           only while both fit 160 KB; BNMF_PROJ_STAGE = 0 / 1 asks for the other form (tests, tools/project_time.py).
// X is uploaded once k-major ([k][j]): a wave's reads of one row are contiguous.
#pragma once
#include "dmath.h"

namespace bnmf {

constexpr int PJ_T = 256;        // threads of k_project with e, g in registers
constexpr int PJ_TL = 64;        // ... with e, g in the LDS
constexpr int PJ_MAX_NT = 32;    // factors whose e, g stay in registers
constexpr int PJ_MAX_N = 128;    // factors at all
constexpr int PJ_NFIT = 3;       // fit rows: mean cosine, mean relative L1 error, largest last-step change
inline int proj_row_stride(int N) { return N <= PJ_MAX_NT ? ((N + 7) / 8) * 8 : N; }
inline size_t proj_lds_bytes(int K, int N, bool stage) {
  return ((N <= PJ_MAX_NT ? 0 : 2 * (size_t)N * PJ_TL) + (stage ? (size_t)K * proj_row_stride(N) : 0)) * sizeof(double);
}

// The KL update over one row k, shared with decompose.h (where the roles of x and X are exchanged): the places 0 .. ni - 1 of the row xk
// against the lane's E and G.  kl_fitted: c = sum_i xk[i] * E(i), i ascending from +0.0.  kl_row: that c, q = c > 0 ? X / c : 0.0,
// G(i) = G(i) + xk[i] * q.  NT > 0: ni = NT is a constant and the loops unroll over registers.
template <int NT, class FE> __device__ __forceinline__ double kl_fitted(const double* __restrict__ xk, int m, FE&& E) {
  const int ni = NT > 0 ? NT : m;
  double c = 0.0;
#pragma unroll
  for (int i = 0; i < ni; ++i) c = c + xk[i] * E(i);
  return c;
}
template <int NT, class FE, class FG> __device__ __forceinline__ void kl_row(const double* __restrict__ xk, double X, int m, FE&& E, FG&& G) {
  const int ni = NT > 0 ? NT : m;
  const double c = kl_fitted<NT>(xk, m, E);
  const double q = c > 0.0 ? X / c : 0.0;
#pragma unroll
  for (int i = 0; i < ni; ++i) G(i) = G(i) + xk[i] * q;
}

// One workgroup per sample of the batch: nin[s], idx[s][0 .. nin) ascending, xg[s][k][i] = P_s[k, idx[i]] / cs[idx[i]] (i < nin), +0.0
// up to the row stride NS.
__global__ __launch_bounds__(256) void k_proj_x(const double* ringP, const double* ringA, size_t lenP, int K, int N, int NS, const int* slots,
                                                const double* cs /* [Sb][N] */, double* xg /* [Sb][K][NS] */, int* nin /* [Sb] */,
                                                int* idx /* [Sb][N] */) {
  __shared__ int sidx[PJ_MAX_N];
  __shared__ int scount;
  const int s = (int)blockIdx.x, tid = (int)threadIdx.x;
  const size_t slot = (size_t)slots[s];
  const double* Ps = ringP + slot * lenP;
  const double* As = ringA + slot * (size_t)N;
  const double* c = cs + (size_t)s * N;
  if (tid == 0) {
    int m = 0;
    for (int n = 0; n < N; ++n) if (As[n] != 0.0 && c[n] > 0.0) sidx[m++] = n;
    scount = m;
    nin[s] = m;
    for (int i = 0; i < N; ++i) idx[(size_t)s * N + i] = i < m ? sidx[i] : -1;
  }
  __syncthreads();
  const int m = scount;
  double* xs = xg + (size_t)s * (size_t)K * (size_t)NS;
  for (int e = tid; e < K * NS; e += 256) {
    const int k = e / NS, i = e - k * NS;
    double v = 0.0;
    if (i < m) { const int n = sidx[i]; v = Ps[(size_t)k + (size_t)K * n] / c[n]; }
    xs[e] = v;
  }
}

template <int NT, bool STAGE>
__global__ __launch_bounds__(NT > 0 ? PJ_T : PJ_TL) void k_project(const double* __restrict__ xg, const int* __restrict__ nin,
                                                                    const int* __restrict__ idx, const double* __restrict__ Xt /* [K][J] */,
                                                                    const double* __restrict__ tX /* [J] */, int K, int N, int J, int n_steps,
                                                                    double* __restrict__ scr /* [Sb][N][J] */,
                                                                    double* __restrict__ fitscr /* [Sb][3][J] */) {
  constexpr bool REG = NT > 0;
  constexpr int T = REG ? PJ_T : PJ_TL;
  extern __shared__ double pj_lds[];
  const int tid = (int)threadIdx.x, s = (int)blockIdx.y;
  const int j = (int)blockIdx.x * T + tid;
  const bool ok = j < J;
  const int jc = ok ? j : J - 1;                   // a lane past the end repeats the last tumour and stores nothing
  const int m = nin[s];                            // factors that take part: workgroup-uniform
  const int NS = REG ? NT : N;
  const int ni = REG ? NT : m;                     // places the loops visit
  double* el = pj_lds + tid;                       // NT = 0: e[i] at el[i * T], g[i] at gl[i * T]
  double* gl = el + (size_t)(REG ? 0 : N) * T;
  const double* xs = xg + (size_t)s * (size_t)K * (size_t)NS;
  if constexpr (STAGE) {
    double* xl = pj_lds + (REG ? 0 : 2 * (size_t)N * T);
    for (int e = tid; e < K * NS; e += T) xl[e] = xs[e];
    __syncthreads();
    xs = xl;
  }
  double er[REG ? NT : 1], gr[REG ? NT : 1];
  auto E = [&](int i) -> double& { if constexpr (REG) return er[i]; else return el[(size_t)i * T]; };
  auto G = [&](int i) -> double& { if constexpr (REG) return gr[i]; else return gl[(size_t)i * T]; };
  const double* Xj = Xt + jc;
  const double t = tX[jc];
  const double e0 = m > 0 ? t / (double)m : 0.0;
#pragma unroll
  for (int i = 0; i < ni; ++i) E(i) = i < m ? e0 : 0.0;
  double d = 0.0;
  for (int step = 0; step < n_steps; ++step) {
#pragma unroll
    for (int i = 0; i < ni; ++i) G(i) = 0.0;
    for (int k = 0; k < K; ++k) {
      kl_row<NT>(xs + (size_t)k * NS, Xj[(size_t)k * J], m, E, G);
    }
    d = 0.0;
#pragma unroll
    for (int i = 0; i < ni; ++i) {
      const double eo = E(i), en = i < m ? eo * G(i) : 0.0;
      const double v = fabs(en - eo);
      d = v > d ? v : d;
      E(i) = en;
    }
  }
  double dot = 0.0, xx = 0.0, cc = 0.0, l1 = 0.0;
  for (int k = 0; k < K; ++k) {
    const double X = Xj[(size_t)k * J];
    const double c = kl_fitted<NT>(xs + (size_t)k * NS, m, E);
    dot = dot + X * c; xx = xx + X * X; cc = cc + c * c; l1 = l1 + fabs(X - c);
  }
  if (!ok) return;
  double* f = fitscr + (size_t)s * PJ_NFIT * (size_t)J + (size_t)j;
  f[0] = dot / dsqrt(xx * cc);
  f[(size_t)J] = t > 0.0 ? l1 / t : 0.0;
  f[2 * (size_t)J] = t > 0.0 ? d / t : 0.0;
  double* a = scr + (size_t)s * (size_t)N * (size_t)J + (size_t)j;
  const int* id = idx + (size_t)s * N;
  for (int n = 0; n < N; ++n) a[(size_t)n * J] = 0.0;
#pragma unroll
  for (int i = 0; i < ni; ++i) if (i < m) a[(size_t)id[i] * J] = E(i);
}

// A thread per new tumour continues st[3][J] (sum of cosine, sum of rel_l1, largest change) over the batch's samples in order; the
// last batch writes the fit rows.
__global__ __launch_bounds__(256) void k_proj_fit(const double* fitscr, int Sb, int J, int S, int first, int last, double* st, double* fit) {
  const int j = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (j >= J) return;
  double sc = 0.0, sl = 0.0, mx = 0.0;
  if (!first) { sc = st[j]; sl = st[(size_t)J + j]; mx = st[2 * (size_t)J + j]; }
  for (int s = 0; s < Sb; ++s) {
    const double* f = fitscr + (size_t)s * PJ_NFIT * (size_t)J + j;
    sc = sc + f[0];
    sl = sl + f[(size_t)J];
    const double v = f[2 * (size_t)J];
    mx = v > mx ? v : mx;
  }
  st[j] = sc; st[(size_t)J + j] = sl; st[2 * (size_t)J + j] = mx;
  if (last) { const double dS = (double)S; fit[j] = sc / dS; fit[(size_t)J + j] = sl / dS; fit[2 * (size_t)J + j] = mx; }
}

// the batch's scratch [Sb][N][J] laid out as E per sample: out[s][n + N j]
__global__ __launch_bounds__(256) void k_proj_exposures(const double* scr, int Sb, int N, int J, double* out) {
  const size_t NJ = (size_t)N * (size_t)J, i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)Sb * NJ) return;
  const size_t s = i / NJ, r = i % NJ, j = r / (size_t)N, n = r % (size_t)N;
  out[i] = scr[s * NJ + n * (size_t)J + j];
}

}  // namespace bnmf
