// bayesnmf_amd/csrc/prune.h — sparse per-tumour assignment with refit over a recorded range: for every used sample of the record_sample
// rings and every included tumour, backward elimination of the sample's signatures with a KL refit of the remaining exposures after every
// removal, until the fit's cosine would fall by more than max_loss, on the device (bnmf_prune / bnmf_prune_at).  This is the
// refit that reconstruction.h's drop_n leaves out.  Reads the P, E and A rings and the data after the fact; no sweep kernel is involved,
// no random number is drawn and none of the chain's streams is consumed.
//
// Only + - * /, dsqrt, |.|, comparisons and whole numbers, no contraction, every sum in the order given here.  The members are the m
// included tumours g_0 < g_1 < ... (position j); every kernel works on the member list, so include[] gives the bits of a cohort without
// the tumours left out.  Per used sample s (oldest first) and member g, with m_k the data cell as a double:
//   set-up    cs[n] = k_map_colsum's column sum of P_s[, n];  factor n takes part iff A_s[n] != 0 and cs[n] > 0;  the places
//             i = 0 .. N_in - 1 are project.h's idx (ascending n) and x[k,i] = P_s[k,idx[i]] / cs[idx[i]] (k_proj_x and its layout);
//             t = sum_k m_k, mm = sum_k m_k m_k (k ascending from +0.0);  warm start e_i = E_s[idx[i], g] * cs[idx[i]], the sample's own
//             renormalised exposure (contrast.h's x, the same bits)
//   step      project.h's kl_row over all places, k ascending, every g_i from +0.0 (a place that is not active holds e_i = +0.0 and adds
//             +0.0);  then e_i = active_i ? e_i * g_i : +0.0 and d = max_i |e_i(new) - e_i(old)| (from +0.0, v > d ? v : d)
//   cosine    with c_k = kl_fitted of the state:  dot = sum_k m_k c_k, cc = sum_k c_k c_k (k ascending from +0.0);
//             cos = rec_cosv(dot, cc, mm): NaN where mm == 0, +0.0 where cc == 0
//   round 0   all N_in places active;  n_steps steps from the warm start give the state and cos_0;  thr = cos_0 - max_loss
//   rounds    while more than one place is active: the candidates are the active places ordered by (e_i ascending, i ascending) in the
//             state;  for each in turn: copy the state, set e_i = +0.0, clear its flag, run n_steps steps, cos_t = the cosine, count the
//             trial;  the first with cos_t >= thr (a comparison with NaN is false) becomes the state and the next round starts;  if none of
//             a round passes, stop
//   a tumour with mm == 0 is undefined: no trials, NaN outputs
// Per (s, g) in the scratch: e_sparse[n] by factor number (exactly +0.0 for a removed or non-participating factor) and vals[5] = cos_0,
// cos_f (the cosine of the last accepted state), n_kept (the places still active), trials, change (t > 0 ? d / t : 0.0 of the last step
// of the last accepted state).  attribution.h's k_attr_share and k_attr_stats (G := m, min_load := the smallest positive double, so that
// its count is #(e_n > 0)) make the load rows of e_sparse; k_prn_stats continues the tumour rows over s ascending and reduces the series.
// The bits depend on the samples, used[], include, the data, n_steps and max_loss only: not on a tumour's place, the batch, the tiling or
// the form of the kernel.
//
// Tiling: project.h's.  A lane owns one problem (s, j); adjacent lanes own adjacent members of one sample, so x is wave-uniform.  The data
// are k-major ([k][j]: a wave's read of one row is contiguous), as k_rec_data leaves them.  A lane carries three vectors of places: the
// accepted state E, the working state W (round 0, then every trial) and g.  One loop serves round 0 and every trial, so the steps exist
// once in the code.  k_prune<NT, STAGE>:
//   NT > 0: E, W and g in registers, NT = ceil(N / 8) * 8 <= 32 of each, the row stride of x is NT; the places N_in .. NT - 1 hold
//           x = +0.0 and are never active (project.h's padding argument: c + 0.0 * 0.0 is c).  The candidate and its removal are selects
//           over compile-time indices, so nothing is indexed dynamically and nothing spills.  256 threads per workgroup; x read at
//           wave-uniform addresses through the caches (project.h's measured choice for this loop).
//   NT = 0: W and g in lane-private LDS columns [N][64] (128 KB at N = 128; a third column would pass the 160 KB a workgroup has), the
//           accepted state in the lane's column of a block of the call's device buffer, read once per trial and written once per accepted
//           state.  N up to PR_MAX_N; 64 threads per workgroup.  BNMF_PRN_FORM = 1 asks for this form at any N.
//   STAGE:  (NT = 0 only) the workgroup copies the sample's K rows of x to the LDS behind the columns while they fit 160 KB.
// Lanes of a wave finish at different trial counts; a lane that is done leaves the loop, idles and stores once.  No atomics, no polling,
// no scratch memory, no MFMA, no grid synchronisation.  All kernels are templates for their place in the code object.
#pragma once
#include "dmath.h"
#include "project.h"
#include "reconstruction.h"

namespace bnmf {

constexpr int PR_T = 256;        // threads of k_prune with the three vectors in registers
constexpr int PR_TL = 64;        // ... with W and g in the LDS
constexpr int PR_MAX_NT = 32;    // factors whose vectors stay in registers
constexpr int PR_MAX_N = 128;    // factors at all
constexpr int PR_TT = 1024;      // threads of k_prn_stats: the W of the sums over the members
constexpr int PR_NVAL = 5;       // per-sample values: cos_0, cos_f, n_kept, trials, change
constexpr int PR_NLOAD = 4, PR_NTUM = 7, PR_NSER = 2, PR_NSIG = 3;
inline int prn_row_stride(int N, bool reg) { return reg ? ((N + 7) / 8) * 8 : N; }
inline size_t prn_lds_bytes(int K, int N, bool reg, bool stage) {
  return reg ? 0 : (2 * (size_t)N * PR_TL + (stage ? (size_t)K * N : 0)) * sizeof(double);
}

// the flags of up to 128 places
struct PrnMask { unsigned long long lo, hi; };
__device__ __forceinline__ bool prn_on(const PrnMask& a, int i) { return i < 64 ? (a.lo >> i) & 1ull : (a.hi >> (i - 64)) & 1ull; }
__device__ __forceinline__ void prn_clear(PrnMask& a, int i) { if (i < 64) a.lo &= ~(1ull << i); else a.hi &= ~(1ull << (i - 64)); }

// A thread per member j: Mt[k][j] = the data cell of tumour members[j] as a double, mm[j] = sum_k m m, tt[j] = sum_k m, k ascending from +0.0.
template <int>
__global__ __launch_bounds__(256) void k_prn_data(const int32_t* M, const double* Mf, const int* members, int K, int m, double* Mt, double* mm, double* tt) {
  const int j = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (j >= m) return;
  const size_t g = (size_t)members[j];
  double a = 0.0, t = 0.0;
  for (int k = 0; k < K; ++k) {
    const size_t i = (size_t)k + (size_t)K * g;
    const double v = Mf ? Mf[i] : (double)M[i];
    Mt[(size_t)k * (size_t)m + (size_t)j] = v;
    a = a + v * v;
    t = t + v;
  }
  mm[j] = a; tt[j] = t;
}

struct PrnArgs {
  const double *xg /* [Sb][K][NS] */, *cs /* [Sb][N] */, *ringE, *Mt /* [K][m] */, *mm, *tt /* [m] */;
  const int *nin /* [Sb] */, *idx /* [Sb][N] */, *slots /* [Sb] */, *members /* [m] */;
  double *scr /* [Sb][N][m]: e_sparse */, *vals /* [Sb][PR_NVAL][m] */, *state /* [Sb][N][m]: the accepted state by place (NT = 0) */;
  size_t lenE; int K, N, G, m, n_steps; double max_loss;
};

template <int NT, bool STAGE>
__global__ __launch_bounds__(NT > 0 ? PR_T : PR_TL) void k_prune(PrnArgs a) {
  constexpr bool REG = NT > 0;
  constexpr int T = REG ? PR_T : PR_TL;
  constexpr int UN = REG ? NT : 1;                 // the loops over the places unroll over registers only
  extern __shared__ double pr_lds[];
  const int tid = (int)threadIdx.x, s = (int)blockIdx.y;
  const int K = a.K, N = a.N, J = a.m;
  const int j = (int)blockIdx.x * T + tid;
  const bool ok = j < J;
  const int jc = ok ? j : J - 1;                   // a lane past the end repeats the last member and stores nothing
  const int m = a.nin[s];                          // places that take part: workgroup-uniform
  const int NS = REG ? NT : N;
  const int ni = REG ? NT : m;                     // places the loops visit
  double* wl = pr_lds + tid;                       // NT = 0: W[i] at wl[i * T], g[i] at gl[i * T]
  double* gl = wl + (size_t)(REG ? 0 : N) * T;
  const double* xs = a.xg + (size_t)s * (size_t)K * (size_t)NS;
  if constexpr (STAGE) {
    double* xl = pr_lds + 2 * (size_t)N * T;
    for (int e = tid; e < K * NS; e += T) xl[e] = xs[e];
    __syncthreads();
    xs = xl;
  }
  double er[REG ? NT : 1], wr[REG ? NT : 1], gr[REG ? NT : 1];
  double* el = a.state + (size_t)s * (size_t)N * (size_t)J + (size_t)jc;   // NT = 0: E[i] at el[i * J] (lanes past the end share the last
                                                                           // member's column: they are lanes of its wave and write the same values to it)
  auto E = [&](int i) -> double& { if constexpr (REG) return er[i]; else return el[(size_t)i * J]; };
  auto W = [&](int i) -> double& { if constexpr (REG) return wr[i]; else return wl[(size_t)i * T]; };
  auto Gv = [&](int i) -> double& { if constexpr (REG) return gr[i]; else return gl[(size_t)i * T]; };
  const double* Mj = a.Mt + jc;
  const double t = a.tt[jc], mm = a.mm[jc];
  const bool def = mm > 0.0;
  const int* id = a.idx + (size_t)s * N;
  const double* cs = a.cs + (size_t)s * N;
  const double* Es = a.ringE + (size_t)a.slots[s] * a.lenE + (size_t)N * (size_t)a.members[jc];

  PrnMask act, wact;                               // the flags of the state and of the working state
  wact.lo = m >= 64 ? ~0ull : (1ull << m) - 1ull;
  wact.hi = m > 64 ? (m >= 128 ? ~0ull : (1ull << (m - 64)) - 1ull) : 0ull;
  act = wact;
#pragma unroll UN
  for (int i = 0; i < ni; ++i) {
    double v = 0.0;
    if (i < m) { const int n = id[i]; v = Es[n] * cs[n]; }
    W(i) = v;
  }
  int c = -1, nk = m;                              // c: the candidate on trial (-1: round 0);  nk: active places of the state
  double cos0 = BNMF_NAN, cosf = BNMF_NAN, thr = BNMF_NAN, chg = 0.0, trials = 0.0;
  double pe = -BNMF_INF; int pi = -1;              // the last candidate of this round that failed, as (e, place)
  double ce = 0.0;                                 // the state's e of the candidate on trial
  for (;;) {
    double d = 0.0;
    for (int step = 0; step < a.n_steps; ++step) {
#pragma unroll UN
      for (int i = 0; i < ni; ++i) Gv(i) = 0.0;
      for (int k = 0; k < K; ++k) kl_row<NT>(xs + (size_t)k * NS, Mj[(size_t)k * J], m, W, Gv);
      d = 0.0;
#pragma unroll UN
      for (int i = 0; i < ni; ++i) {
        const double eo = W(i), en = prn_on(wact, i) ? eo * Gv(i) : 0.0;
        const double v = dabs(en - eo);
        d = v > d ? v : d;
        W(i) = en;
      }
    }
    double dot = 0.0, cc = 0.0;
    for (int k = 0; k < K; ++k) {
      const double X = Mj[(size_t)k * J];
      const double f = kl_fitted<NT>(xs + (size_t)k * NS, m, W);
      dot = dot + X * f; cc = cc + f * f;
    }
    const double cosv = rec_cosv(dot, cc, mm);
    bool accept = true;
    if (c < 0) { cos0 = cosv; thr = cos0 - a.max_loss; }
    else { trials = trials + 1.0; accept = cosv >= thr; }
    if (accept) {
#pragma unroll UN
      for (int i = 0; i < ni; ++i) E(i) = W(i);
      act = wact; cosf = cosv; chg = t > 0.0 ? d / t : 0.0;
      if (c >= 0) --nk;
      pe = -BNMF_INF; pi = -1;
    } else {
      pe = ce; pi = c;
    }
    if (!def || nk <= 1) break;
    // the next candidate: the smallest (e_i, i) of the active places of the state above (pe, pi)
    int best = -1; double be = 0.0;
#pragma unroll UN
    for (int i = 0; i < ni; ++i) {
      const double v = E(i);
      const bool after = v > pe || (v == pe && i > pi);
      if (prn_on(act, i) && after && (best < 0 || v < be)) { best = i; be = v; }
    }
    if (best < 0) break;                           // every candidate of the round failed
    c = best; ce = be;
    wact = act; prn_clear(wact, c);
#pragma unroll UN
    for (int i = 0; i < ni; ++i) W(i) = i == c ? 0.0 : E(i);
  }
  if (!ok) return;
  double* v = a.vals + (size_t)s * PR_NVAL * (size_t)J + (size_t)j;
  v[0] = cos0; v[(size_t)J] = cosf; v[2 * (size_t)J] = def ? (double)nk : BNMF_NAN; v[3 * (size_t)J] = trials; v[4 * (size_t)J] = def ? chg : BNMF_NAN;
  double* o = a.scr + (size_t)s * (size_t)N * (size_t)J + (size_t)j;
  for (int n = 0; n < N; ++n) o[(size_t)n * J] = def ? 0.0 : BNMF_NAN;
  if (def) {
#pragma unroll UN
    for (int i = 0; i < ni; ++i) if (i < m) o[(size_t)id[i] * J] = E(i);
  }
}

// Blocks 0 .. 2 Sb - 1: block 2 s + r reduces over the members the sample's n_kept (r = 0) or cos_f (r = 1), an undefined tumour entered as
// +0.0 (ser[r][s0 + s]).  The blocks after them: a thread per member continues st[PR_NTUM][m] over the batch's samples in order: Welford
// means of cos_0 and cos_f, the sum of n_kept, its smallest (from +inf) and largest (from +0.0), the largest change (from +0.0), the sum
// of trials.  The last batch writes the tumour rows in member order (NaN for an undefined tumour).
template <int>
__global__ __launch_bounds__(PR_TT) void k_prn_stats(const double* vals, const double* mmv, int Sb, int m, int S, int s0, int last, double* st,
                                                     double* ser /* [2][S] */, double* tum /* [PR_NTUM][m] */) {
  __shared__ double buf[PR_TT];
  const int tid = (int)threadIdx.x, b = (int)blockIdx.x;
  const size_t per = (size_t)PR_NVAL * (size_t)m, M = (size_t)m;
  if (b < 2 * Sb) {                                // block-uniform
    const int s = b >> 1, r = b & 1;
    const double* x = vals + (size_t)s * per + (r ? M : 2 * M);
    double acc = 0.0;
    for (int j = tid; j < m; j += PR_TT) acc = acc + (mmv[j] > 0.0 ? x[j] : 0.0);
    const double v = block_tree<PR_TT>(acc, buf, tid);
    if (tid == 0) ser[(size_t)r * S + (size_t)s0 + s] = v;
    return;
  }
  const size_t j = (size_t)(b - 2 * Sb) * PR_TT + tid;
  if (j >= M) return;
  double m0 = 0.0, mf = 0.0, sk = 0.0, kmin = BNMF_INF, kmax = 0.0, cmax = 0.0, str = 0.0;
  if (s0 > 0) { m0 = st[j]; mf = st[M + j]; sk = st[2 * M + j]; kmin = st[3 * M + j]; kmax = st[4 * M + j]; cmax = st[5 * M + j]; str = st[6 * M + j]; }
  for (int s = 0; s < Sb; ++s) {
    const double* x = vals + (size_t)s * per + j;
    const double c0 = x[0], cf = x[M], nk = x[2 * M], tr = x[3 * M], ch = x[4 * M];
    const double rs = 1.0 / (double)(s0 + s + 1);
    const double d0 = c0 - m0;
    m0 = m0 + d0 * rs;
    const double df = cf - mf;
    mf = mf + df * rs;
    sk = sk + nk;                                  // whole numbers below 2^53: exact
    kmin = nk < kmin ? nk : kmin;
    kmax = nk > kmax ? nk : kmax;
    cmax = ch > cmax ? ch : cmax;
    str = str + tr;
  }
  st[j] = m0; st[M + j] = mf; st[2 * M + j] = sk; st[3 * M + j] = kmin; st[4 * M + j] = kmax; st[5 * M + j] = cmax; st[6 * M + j] = str;
  if (last) {
    const bool def = mmv[j] > 0.0;
    const double dS = (double)S;
    tum[j] = def ? m0 : BNMF_NAN; tum[M + j] = def ? mf : BNMF_NAN; tum[2 * M + j] = def ? sk / dS : BNMF_NAN; tum[3 * M + j] = def ? kmin : BNMF_NAN;
    tum[4 * M + j] = def ? kmax : BNMF_NAN; tum[5 * M + j] = def ? cmax : BNMF_NAN; tum[6 * M + j] = def ? str / dS : BNMF_NAN;
  }
}

}  // namespace bnmf
