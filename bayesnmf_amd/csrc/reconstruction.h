// bayesnmf_amd/csrc/reconstruction.h — reconstruction quality per tumour over a recorded range: for every used sample of the
// record_sample rings the cosine between every tumour's observed profile and its fit, the relative L1 error and the RMSE, and per factor
// the cosine of the fit without that factor (leave one signature out) and the drop it costs, on the device (bnmf_reconstruction /
// bnmf_reconstruction_at).  Reads the P, E and A rings and the data after the fact; no sweep kernel is involved, no random
// number is drawn and none of the chain's streams is consumed.
//
// Per used sample s (oldest first), tumour g and mutation type k, m the data cell as a double:
//   f_n       = (P_s[k,n] * A_s[n]) * E_s[n,g]                   attribution.h's expression, the same bits
//   pre_0     = +0.0;  pre_{n+1} = pre_n + f_n                   n ascending
//   suf_{N-1} = +0.0;  suf_{n-1} = suf_n + f_n                   n descending
//   c = pre_N (waic.h's c_s, the same bits);   c_-n = pre_n + suf_n (the fit without factor n: no subtraction, never negative);   d = m - c
// Per (s, g), each sum over k ascending from +0.0 (project.h's order for its fit rows):
//   dot = sum m c   cc = sum c c   l1 = sum |d|   sse = sum d d   dot_-n = sum m c_-n   cc_-n = sum c_-n c_-n
// Per g, once, in the same order:  mm = sum m m   t = sum |m|
//   cosv(dot, cc) = mm > 0 ? (cc > 0 ? dot / dsqrt(mm * cc) : +0.0) : NaN
//   cos = cosv(dot, cc);  rel_l1 = t > 0 ? l1 / t : 0.0;  rmse = dsqrt(sse / (double)K)
//   cos_-n = A_s[n] != 0 ? cosv(dot_-n, cc_-n) : cos;   drop_n = A_s[n] != 0 ? cos - cos_-n : +0.0
// The remaining exposures are NOT refitted after the removal: drop_n is an upper bound of what removing signature n costs the tumour.
// Over s ascending attribution.h's Welford (d = a - mu; mu = mu + d * (1 / s); M2 = M2 + d * (a - mu)) and plain counts give
//   tumour [6][G]: mean cos, its variance (S - 1 form), the smallest cos (from +inf, v < d ? v : d), mean rel_l1, mean rmse,
//                  #(cos >= min_cosine) / S;  rows 0, 1, 2 and 5 are NaN where mm == 0
//   drop [4][N*G] (n + N g): mean drop_n, its variance, mean cos_-n, #(drop_n >= min_drop) / S;  NaN where mm == 0
//   series sum [S]: canon(cos over the defined tumours, an undefined one entered as +0.0; W = 1024) over g (block_tree<1024>'s order);
//                   the host divides it by the number of defined tumours
// The bits depend on the samples, used[], the data and the two thresholds only: not on the batch size, the tiling or the form of the kernel.
//
// Tiling: project.h's.  A lane owns one problem (s, g) and its k loop is the order of the sums: no cross-lane reduction.  Adjacent lanes
// own adjacent tumours of one sample, so the sample's row P_s[k, .] A_s is wave-uniform.  k_rec_data leaves the data k-major as doubles
// ([k][g]: a wave's read of one row is contiguous) with mm and t; k_rec_x leaves per sample the rows x[k][i] = P_s[k,i] * A_s[i], then
// +0.0 up to the row stride.  k_rec<NT, STAGE>:
//   NT > 0: the lane's column of E_s, pre_n and the 2 NT + 4 sums in registers, NT = ceil(N / 8) * 8 <= 32, the row stride is NT.  The
//           places N .. NT - 1 hold x = +0.0 and e = +0.0: pre + 0.0 * 0.0 is pre and suf + 0.0 * 0.0 is suf, bit for bit, since neither
//           is ever -0.0 (P, E >= 0 and A is 0 or 1).  256 threads per workgroup.
//   NT = 0: tiles of RC_TN factors.  Per tile and row the whole column is walked again: pre_n up the column, suf_n down to the tile, so
//           the same operations meet the same values; the lane reads its column of E_s through the caches.  The four sums of the full
//           fit are taken beside the first tile.  BNMF_REC_FORM = 1 asks for this form at any N.
//   STAGE:  the workgroup copies the sample's K rows of x to the LDS once and the lanes read them as broadcasts; else every lane reads x
//           at wave-uniform addresses through the caches: the same values.  This is project.h's choice, but measured at the headline
//           shape the staged form is the faster one here in the register form too, so the host stages x whenever it
//           fits 160 KB; BNMF_REC_STAGE = 0 / 1 asks for either form (tests, tools/reconstruction_time.py).
// The per-sample values go through the scratch [Sb][N + 3][G] (cos, rel_l1, rmse, then cosv(dot_-n, cc_-n) for every n) in batches;
// k_rec_stats continues the statistics from the previous batch in sample order, selects cos_-n and drop_n by A_s[n], and reduces the series.
// No atomics, no polling, no scratch memory.
#pragma once
#include "dmath.h"

namespace bnmf {

constexpr int RC_T = 256;        // threads of k_rec
constexpr int RC_MAX_NT = 32;    // factors whose sums stay in registers
constexpr int RC_TN = 8;         // factors of a tile of the tiled form
constexpr int RC_TT = 1024;      // threads of k_rec_stats: the W of the sum over g
constexpr int RC_NTUM = 6, RC_NDROP = 4;
inline int rec_row_stride(int N) { return N <= RC_MAX_NT ? ((N + 7) / 8) * 8 : N; }
inline size_t rec_lds_bytes(int K, int NS) { return (size_t)K * NS * sizeof(double); }

__device__ __forceinline__ double rec_cosv(double dot, double cc, double mm) {
  return mm > 0.0 ? (cc > 0.0 ? dot / dsqrt(mm * cc) : 0.0) : BNMF_NAN;
}

// (k_rec_data, k_rec_x and k_rec_stats use no template parameter: they are templates only for their place in the code object, behind
// every kernel that exists)
// A thread per tumour: Mt[k][g] = the data cell as a double, mm[g] = sum_k m m, tt[g] = sum_k |m|, k ascending from +0.0.
template <int>
__global__ __launch_bounds__(256) void k_rec_data(const int32_t* M, const double* Mf, int K, int G, double* Mt, double* mm, double* tt) {
  const int g = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (g >= G) return;
  double a = 0.0, t = 0.0;
  for (int k = 0; k < K; ++k) {
    const size_t i = (size_t)k + (size_t)K * (size_t)g;
    const double m = Mf ? Mf[i] : (double)M[i];
    Mt[(size_t)k * (size_t)G + (size_t)g] = m;
    a = a + m * m;
    t = t + dabs(m);
  }
  mm[g] = a; tt[g] = t;
}

// One workgroup per sample of the batch: xg[s][k][i] = P_s[k,i] * A_s[i] (i < N), +0.0 up to the row stride NS.
template <int>
__global__ __launch_bounds__(256) void k_rec_x(const double* ringP, const double* ringA, size_t lenP, int K, int N, int NS, const int* slots,
                                               double* xg /* [Sb][K][NS] */) {
  const int s = (int)blockIdx.x, tid = (int)threadIdx.x;
  const size_t slot = (size_t)slots[s];
  const double* Ps = ringP + slot * lenP;
  const double* As = ringA + slot * (size_t)N;
  double* xs = xg + (size_t)s * (size_t)K * (size_t)NS;
  for (int e = tid; e < K * NS; e += 256) {
    const int k = e / NS, i = e - k * NS;
    xs[e] = i < N ? Ps[(size_t)k + (size_t)K * i] * As[i] : 0.0;
  }
}

template <int NT, bool STAGE>
__global__ __launch_bounds__(RC_T) void k_rec(const double* __restrict__ xg, const double* __restrict__ ringE, size_t lenE,
                                              const int* __restrict__ slots, const double* __restrict__ Mt /* [K][G] */,
                                              const double* __restrict__ mmv, const double* __restrict__ ttv, int K, int N, int G,
                                              double* __restrict__ scr /* [Sb][N + 3][G] */) {
  constexpr bool REG = NT > 0;
  extern __shared__ double rc_lds[];
  const int tid = (int)threadIdx.x, s = (int)blockIdx.y;
  const int g = (int)blockIdx.x * RC_T + tid;
  const bool ok = g < G;
  const int gc = ok ? g : G - 1;                   // a lane past the end repeats the last tumour and stores nothing
  const int NS = REG ? NT : N;
  const double* xs = xg + (size_t)s * (size_t)K * (size_t)NS;
  if constexpr (STAGE) {
    for (int e = tid; e < K * NS; e += RC_T) rc_lds[e] = xs[e];
    __syncthreads();
    xs = rc_lds;
  }
  const double* Es = ringE + (size_t)slots[s] * lenE + (size_t)N * (size_t)gc;
  const double* Mg = Mt + gc;
  const double mm = mmv[gc], tt = ttv[gc];
  double* o = scr + (size_t)s * (size_t)(N + 3) * (size_t)G + (size_t)gc;
  double dot = 0.0, cc = 0.0, l1 = 0.0, sse = 0.0;

  if constexpr (REG) {
    double e[NT], dm[NT], cm[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i) { e[i] = i < N ? Es[i] : 0.0; dm[i] = 0.0; cm[i] = 0.0; }
    for (int k = 0; k < K; ++k) {
      const double* row = xs + (size_t)k * NT;
      const double m = Mg[(size_t)k * (size_t)G];
      double pre[NT];
      double p = 0.0;
#pragma unroll
      for (int i = 0; i < NT; ++i) { pre[i] = p; p = p + row[i] * e[i]; }
      const double d = m - p;
      dot = dot + m * p; cc = cc + p * p; l1 = l1 + dabs(d); sse = sse + d * d;
      double sf = 0.0;
#pragma unroll
      for (int i = NT - 1; i >= 0; --i) {
        const double c = pre[i] + sf;
        dm[i] = dm[i] + m * c;
        cm[i] = cm[i] + c * c;
        sf = sf + row[i] * e[i];
      }
    }
    if (!ok) return;
#pragma unroll
    for (int i = 0; i < NT; ++i) if (i < N) o[(size_t)(3 + i) * (size_t)G] = rec_cosv(dm[i], cm[i], mm);
  } else {
    for (int n0 = 0; n0 < N; n0 += RC_TN) {        // workgroup-uniform
      double dm[RC_TN], cm[RC_TN];
#pragma unroll
      for (int i = 0; i < RC_TN; ++i) { dm[i] = 0.0; cm[i] = 0.0; }
      const int n1 = min(n0 + RC_TN, N);
      for (int k = 0; k < K; ++k) {
        const double* row = xs + (size_t)k * NS;
        const double m = Mg[(size_t)k * (size_t)G];
        double pre[RC_TN];
        double p = 0.0;
        for (int n = 0; n < n0; ++n) p = p + row[n] * Es[n];
#pragma unroll
        for (int i = 0; i < RC_TN; ++i) if (n0 + i < N) { pre[i] = p; p = p + row[n0 + i] * Es[n0 + i]; }
        for (int n = n1; n < N; ++n) p = p + row[n] * Es[n];
        if (n0 == 0) {
          const double d = m - p;
          dot = dot + m * p; cc = cc + p * p; l1 = l1 + dabs(d); sse = sse + d * d;
        }
        double sf = 0.0;
        for (int n = N - 1; n >= n1; --n) sf = sf + row[n] * Es[n];
#pragma unroll
        for (int i = RC_TN - 1; i >= 0; --i)
          if (n0 + i < N) {
            const double c = pre[i] + sf;
            dm[i] = dm[i] + m * c;
            cm[i] = cm[i] + c * c;
            sf = sf + row[n0 + i] * Es[n0 + i];
          }
      }
      if (ok) {
#pragma unroll
        for (int i = 0; i < RC_TN; ++i) if (n0 + i < N) o[(size_t)(3 + n0 + i) * (size_t)G] = rec_cosv(dm[i], cm[i], mm);
      }
    }
    if (!ok) return;
  }
  o[0] = rec_cosv(dot, cc, mm);
  o[(size_t)G] = tt > 0.0 ? l1 / tt : 0.0;
  o[2 * (size_t)G] = dsqrt(sse / (double)K);
}

// Blocks 0 .. Sb - 1: block s reduces the sample's cos over g, an undefined tumour entered as +0.0 (ser[s0 + s]).  The blocks after them:
// a thread per element continues the statistics over the batch's samples in order.  Elements 0 .. G - 1 are the tumours (st[6][G]: mean
// and M2 of cos, the smallest cos, mean rel_l1, mean rmse, the count of cos >= min_cosine); element G + g + G n is (n, g) (sd[4][N*G],
// indexed g + G n as the scratch: mean and M2 of drop_n, mean cos_-n, the count of drop_n >= min_drop).  The last batch also writes the
// output rows, drop laid out as E (n + N g).
template <int>
__global__ __launch_bounds__(RC_TT) void k_rec_stats(const double* scr, const double* ringA, const int* slots, const double* mmv, int Sb, int N, int G,
                                                     int S, int s0, int last, double min_cosine, double min_drop, double* st, double* sd,
                                                     double* ser /* [S] */, double* tumour /* [6][G] */, double* drop /* [4][N*G] */) {
  __shared__ double buf[RC_TT];
  const int tid = (int)threadIdx.x, b = (int)blockIdx.x;
  const size_t per = (size_t)(N + 3) * (size_t)G;
  if (b < Sb) {                                    // block-uniform
    const double* x = scr + (size_t)b * per;
    double acc = 0.0;
    for (int g = tid; g < G; g += RC_TT) acc = acc + (mmv[g] > 0.0 ? x[g] : 0.0);
    const double r = block_tree<RC_TT>(acc, buf, tid);
    if (tid == 0) ser[(size_t)s0 + b] = r;
    return;
  }
  const size_t NG = (size_t)N * (size_t)G, e = (size_t)(b - Sb) * RC_TT + tid;
  if (e >= NG + (size_t)G) return;
  const double dS = (double)S, dS1 = (double)(S - 1);
  if (e < (size_t)G) {
    const size_t g = e;
    double mu = 0.0, m2 = 0.0, mn = BNMF_INF, ml = 0.0, mr = 0.0, cnt = 0.0;
    if (s0 > 0) { mu = st[g]; m2 = st[(size_t)G + g]; mn = st[2 * (size_t)G + g]; ml = st[3 * (size_t)G + g]; mr = st[4 * (size_t)G + g]; cnt = st[5 * (size_t)G + g]; }
    for (int s = 0; s < Sb; ++s) {
      const double* x = scr + (size_t)s * per + g;
      const double c = x[0], l = x[(size_t)G], r = x[2 * (size_t)G];
      const double rs = 1.0 / (double)(s0 + s + 1);
      const double d = c - mu;
      mu = mu + d * rs;
      m2 = m2 + d * (c - mu);
      mn = c < mn ? c : mn;
      const double dl = l - ml;
      ml = ml + dl * rs;
      const double dr = r - mr;
      mr = mr + dr * rs;
      cnt = cnt + (c >= min_cosine ? 1.0 : 0.0);   // a whole number below 2^53: exact
    }
    st[g] = mu; st[(size_t)G + g] = m2; st[2 * (size_t)G + g] = mn; st[3 * (size_t)G + g] = ml; st[4 * (size_t)G + g] = mr; st[5 * (size_t)G + g] = cnt;
    if (last) {
      const bool def = mmv[g] > 0.0;
      tumour[g] = def ? mu : BNMF_NAN; tumour[(size_t)G + g] = def ? m2 / dS1 : BNMF_NAN; tumour[2 * (size_t)G + g] = def ? mn : BNMF_NAN;
      tumour[3 * (size_t)G + g] = ml; tumour[4 * (size_t)G + g] = mr; tumour[5 * (size_t)G + g] = def ? cnt / dS : BNMF_NAN;
    }
    return;
  }
  const size_t i = e - (size_t)G, n = i / (size_t)G, g = i % (size_t)G;
  double mu = 0.0, m2 = 0.0, mc = 0.0, cnt = 0.0;
  if (s0 > 0) { mu = sd[i]; m2 = sd[NG + i]; mc = sd[2 * NG + i]; cnt = sd[3 * NG + i]; }
  for (int s = 0; s < Sb; ++s) {
    const double* x = scr + (size_t)s * per + g;
    const bool in = ringA[(size_t)slots[s] * (size_t)N + n] != 0.0;
    const double c = x[0], cv = x[(3 + n) * (size_t)G];
    const double cmn = in ? cv : c, dr = in ? c - cv : 0.0;
    const double rs = 1.0 / (double)(s0 + s + 1);
    const double d = dr - mu;
    mu = mu + d * rs;
    m2 = m2 + d * (dr - mu);
    const double dc = cmn - mc;
    mc = mc + dc * rs;
    cnt = cnt + (dr >= min_drop ? 1.0 : 0.0);
  }
  sd[i] = mu; sd[NG + i] = m2; sd[2 * NG + i] = mc; sd[3 * NG + i] = cnt;
  if (last) {
    const bool def = mmv[g] > 0.0;
    const size_t o = n + (size_t)N * g;
    drop[o] = def ? mu : BNMF_NAN; drop[NG + o] = def ? m2 / dS1 : BNMF_NAN; drop[2 * NG + o] = def ? mc : BNMF_NAN; drop[3 * NG + o] = def ? cnt / dS : BNMF_NAN;
  }
}

}  // namespace bnmf
