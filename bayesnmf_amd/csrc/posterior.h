// bayesnmf_amd/csrc/posterior.h — the posterior calls on a recorded range of samples: bnmf_map, bnmf_waic, bnmf_ppc, bnmf_attribution,
// bnmf_mixing, bnmf_assign, bnmf_relabel, bnmf_project, bnmf_decompose, bnmf_contrast, bnmf_regress, bnmf_coactivity, bnmf_stability, bnmf_reconstruction, bnmf_similarity, bnmf_subtypes, bnmf_residuals, bnmf_tradeoff, bnmf_prune, bnmf_summary (each with its _at form) and bnmf_label_switching.  Host code only: the
// kernels are in kernels.h, waic.h, ppc.h, attribution.h, mixing.h, relabel.h, project.h, decompose.h, contrast.h, regress.h, coactivity.h, stability.h, reconstruction.h, similarity.h, subtypes.h, residuals.h, tradeoff.h, prune.h and summary.h.  Included by api.hip (one translation unit) behind sweep.h.
// The first part is the layer the calls share: the range and its slot list, the quiesce, the handle's one scratch buffer
// and its carver, the reference catalogue, the dynamic-LDS opt-in.  A call supplies its own checks, its carve list, its launches and
// its host reduction.
#pragma once
#include "reduce_host.h"   // the device-free reductions over the samples

// copy the `last_n` consecutive samples that end at iteration `end_iter` (oldest first) of a ring to the host: sample `it` lives in slot
// (it - 1) % (window + 1), so they are at most two contiguous runs
static int ring_read(const bnmf_handle* h, int id, int end_iter, int last_n, double* out) {
  const Arr& a = h->arr[id];
  const size_t len = id_len(h, id), C = (size_t)h->wcap, s0 = (size_t)(end_iter - last_n) % C;
  const size_t n1 = (s0 + (size_t)last_n <= C) ? (size_t)last_n : C - s0;
  HIPCHK(hipMemcpy(out, a.ring + s0 * len, n1 * len * sizeof(double), hipMemcpyDeviceToHost));
  if (n1 < (size_t)last_n) HIPCHK(hipMemcpy(out + n1 * len, a.ring, ((size_t)last_n - n1) * len * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

// ---- the range ----
// bnmf_X names the last n samples (at = false), bnmf_X_at the n samples that end at iteration end_iter.
struct Range { bool at; int end_iter, n; };

static int check_alive(const bnmf_handle* h, const char* fn) {
  if (h->poisoned) return fail(BNMF_ESTATE, "%s: the handle timed out inside a kernel; its state is invalid", fn);
  return 0;
}
static int check_recorded(const bnmf_handle* h, const char* fn) {
  if (int rc = check_alive(h, fn)) return rc;
  if (h->cfg.window <= 0) return fail(BNMF_ESTATE, "%s: the handle was created with window = 0", fn);
  return 0;
}
static int check_last(const bnmf_handle* h, const char* fn, int last_n) {
  const int W = h->cfg.window;
  if (last_n < 1 || last_n > W || last_n > h->iter) return fail(BNMF_ESIZE, "%s: last_n = %d but only min(window = %d, iter = %d) samples are kept", fn, last_n, W, h->iter);
  return 0;
}
// Iterations first..last must be recorded and still kept: [max(1, iter - window + 1), iter] (the ring holds window + 1 slots, the
// slot ahead of the oldest kept sample belongs to the iteration in flight).
static int check_kept(const bnmf_handle* h, const char* fn, long long first, long long last) {
  const int lo = std::max(1, h->iter - h->cfg.window + 1);
  if (first > last || first < lo || last > h->iter)
    return fail(BNMF_ESIZE, "%s: iterations %lld..%lld requested but only iterations %d..%d are kept (window = %d, iter = %d)", fn, first, last, lo,
                h->iter, h->cfg.window, h->iter);
  return 0;
}
// check `r` and make it explicit: afterwards r.end_iter is the range's last iteration in both forms
static int range_resolve(const bnmf_handle* h, const char* fn, Range& r) {
  if (r.at) return check_kept(h, fn, (long long)r.end_iter - r.n + 1, r.end_iter);
  r.end_iter = h->iter;
  return check_last(h, fn, r.n);
}
// what every call does first: `args_ok` is the call's null check (it includes h), then the handle, then the range
static int range_enter(const bnmf_handle* h, const char* fn, bool args_ok, Range& r) {
  if (!args_ok) return fail(BNMF_EINVAL, "%s: null argument", fn);
  if (int rc = check_recorded(h, fn)) return rc;
  return range_resolve(h, fn, r);
}
// The ring slots of the samples of `r` that used[] flags (null: all of them), oldest first; with `iters` their iterations behind them
// in the same vector.  strict: a used[s] outside {0, 1} is refused; else any non-zero value flags a sample (bnmf_assign).
static int range_slots(const bnmf_handle* h, const char* fn, const Range& r, const int32_t* used, bool strict, std::vector<int>& slots, bool iters = false) {
  slots.clear();
  for (int s = 0; s < r.n; ++s) {
    if (strict && used && used[s] != 0 && used[s] != 1) return fail(BNMF_EINVAL, "%s: used[%d] = %d is neither 0 nor 1", fn, s, (int)used[s]);
    if (!used || used[s]) slots.push_back((int)((size_t)(r.end_iter - r.n + s) % (size_t)h->wcap));
  }
  if (iters) for (int s = 0; s < r.n; ++s) if (!used || used[s]) slots.push_back(r.end_iter - r.n + 1 + s);
  return 0;
}

// ---- quiesce: nothing of the chain is in flight while a posterior call reads the rings ----
static int post_sync(const bnmf_handle* h) {
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipStreamSynchronize(h->side));
  HIPCHK(hipStreamSynchronize(h->side2));
  return 0;
}

// ---- scratch: one buffer per handle, grown on demand; a call carves it and leaves nothing in it that a later call reads ----
static int scratch_reserve(bnmf_handle* h, size_t need) {
  Scratch& s = h->scratch;
  if (need <= s.bytes) return 0;
  s.bytes = 0;                                            // first: a failed replacement leaves an empty scratch, not a stale size
  HIPCHK(hfree(h, s.p));
  HIPCHK(hmalloc(h, &s.p, need));
  s.bytes = need;
  return 0;
}
// bump carver: typed sub-blocks in the order taken, each aligned to 256 bytes
struct Carve {
  uintptr_t base; size_t off = 0;
  template <class T> T* take(size_t n) { T* p = (T*)(base + off); off += (n * sizeof(T) + 255) & ~(size_t)255; return p; }
};
// run a call's carve list twice: once to measure, then, the scratch reserved, to hand out the blocks
template <class List> static int carve(bnmf_handle* h, List list) {
  Carve measure{0};
  list(measure);
  if (int rc = scratch_reserve(h, measure.off)) return rc;
  Carve c{(uintptr_t)h->scratch.p};
  list(c);
  return 0;
}

// ---- the reference catalogue of bnmf_assign and bnmf_label_switching, and the assignment problem's LDS ----
// dRef: the catalogue row-major [k][j]; dN2 and rn2: its squared column norms, summed over k ascending (MAP_cosine is pinned bit for bit)
static int catalogue_upload(const double* ref, int K, int R, double* dRef, double* dN2, std::vector<double>& rn2) {
  std::vector<double> refT((size_t)K * R);
  rn2.assign(R, 0.0);
  for (int j = 0; j < R; ++j) for (int k = 0; k < K; ++k) { const double v = ref[k + (size_t)K * j]; refT[(size_t)k * R + j] = v; rn2[j] += v * v; }
  HIPCHK(hipMemcpy(dRef, refT.data(), refT.size() * 8, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(dN2, rn2.data(), R * 8, hipMemcpyHostToDevice));
  return 0;
}
static size_t hungarian_lds_bytes(int nrow, int ncol) { return (size_t)(ncol + 1) * (16 + 12) + (size_t)(nrow + 1) * 8; }

// ---- dynamic LDS above the 64 KB a kernel may use unasked: raise the kernel's limit to `limit` ----
static constexpr size_t LDS_CAP = 160 * 1024;
template <class Kern> static int opt_in_lds(Kern* kernel, size_t bytes, size_t limit = LDS_CAP) {
  if (bytes <= 64 * 1024) return 0;
  HIPCHK(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)limit));
  return 0;
}

// ---- the calls ----

// get_MAP_ over the samples of r
static int map_impl(bnmf_handle* h, const char* fn, Range r, double ci, double* P_mean, double* E_mean, double* A_mode, double* top_A,
                    double* P_lower, double* P_upper, double* E_lower, double* E_upper, int32_t* used, bnmf_map_info* info) {
  if (int rc = range_enter(h, fn, h && A_mode && info, r)) return rc;
  const int end_iter = r.end_iter, last_n = r.n;
  if (ci >= 1.0) return fail(BNMF_EINVAL, "bnmf_map: credible_interval must be below 1");
  const int K = h->cfg.K, N = h->cfg.N, G = h->cfg.G;
  const size_t lenP = (size_t)K * N, lenE = (size_t)N * G;
  if (!h->arr[BNMF_P].ring || !h->arr[BNMF_E].ring || !h->arr[BNMF_A].ring) return fail(BNMF_ESTATE, "bnmf_map: nothing recorded yet");
  if (int rc = post_sync(h)) return rc;
  // i. mode of A (get_mode): patterns as strings, most frequent first, ties in alphabetical order
  std::vector<double> Aw((size_t)last_n * N);
  if (int rc = ring_read(h, BNMF_A, end_iter, last_n, Aw.data())) return rc;
  std::vector<std::string> keys(last_n, std::string(N, '0'));
  std::map<std::string, int> tab;
  for (int s = 0; s < last_n; ++s) { for (int n = 0; n < N; ++n) if (Aw[(size_t)s * N + n] != 0.0) keys[s][n] = '1'; tab[keys[s]]++; }
  std::vector<std::pair<std::string, int>> ord(tab.begin(), tab.end());        // std::map iterates alphabetically
  std::stable_sort(ord.begin(), ord.end(), [](const auto& a, const auto& b) { return a.second > b.second; });
  const std::string& mode = ord[0].first;
  info->n_patterns = (int)ord.size();
  for (int i = 0; i < 5; ++i) {
    info->top_counts[i] = i < (int)ord.size() ? ord[i].second : 0;
    if (top_A) for (int n = 0; n < N; ++n) top_A[(size_t)i * N + n] = i < (int)ord.size() ? (ord[i].first[n] == '1' ? 1.0 : 0.0) : std::nan("");
  }
  std::vector<int32_t> is_mode(last_n);
  for (int s = 0; s < last_n; ++s) is_mode[s] = keys[s] == mode ? 1 : 0;
  if (used) std::copy(is_mode.begin(), is_mode.end(), used);
  std::vector<int> slots;
  if (int rc = range_slots(h, fn, r, is_mode.data(), false, slots)) return rc;
  const int nu = (int)slots.size();
  info->n_used = nu; info->_pad = 0;
  std::vector<double> Am(N);
  for (int n = 0; n < N; ++n) Am[n] = A_mode[n] = mode[n] == '1' ? 1.0 : 0.0;
  // ii-iii. renormalised means (and quantiles) on the device
  const bool want_ci = ci > 0.0 && (P_lower || P_upper || E_lower || E_upper);
  int kt = 0, jlo = 0, jhi = 0; double glo = 0.0, ghi = 0.0;
  if (want_ci) {                                    // quantile type 7: h = (n-1) p, j = floor(h), g = h - j
    const double plo = 0.5 - ci / 2.0, phi = 0.5 + ci / 2.0;
    const double hl = (nu - 1) * plo, hh = (nu - 1) * phi;
    jlo = (int)std::floor(hl); glo = hl - jlo; jhi = (int)std::floor(hh); ghi = hh - jhi;
    kt = std::min(nu, std::max(jlo + 2, nu - jhi));
  }
  // the bounds by sorting (k_map_quant) when the samples of 8 elements fit the LDS; else by the kt smallest / largest per lane
  int qS = 0;
  if (want_ci) { qS = ((nu + 63) / 64) * 64; if (qS > 2048) qS = 0; }
  if (want_ci && !qS && (size_t)kt * 2 * 64 * sizeof(double) > LDS_CAP)
    return fail(BNMF_EINVAL, "bnmf_map: credible_interval %.3g over %d samples needs %d order statistics per element (device limit 160): take the window with bnmf_window", ci, nu, kt);
  double *cs, *mP, *loP, *hiP, *mE, *loE, *hiE, *colsse, *dA; int* dslots;
  if (int rc = carve(h, [&](Carve& c) {
        cs = c.take<double>((size_t)nu * N);
        mP = c.take<double>(lenP); loP = c.take<double>(lenP); hiP = c.take<double>(lenP);
        mE = c.take<double>(lenE); loE = c.take<double>(lenE); hiE = c.take<double>(lenE);
        colsse = c.take<double>(2 * (size_t)G);         // colsse, then colkl
        dA = c.take<double>(N); dslots = c.take<int>(nu);
      })) return rc;
  double* colkl = colsse + G;
  HIPCHK(hipMemcpyAsync(dslots, slots.data(), nu * sizeof(int), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(dA, Am.data(), N * sizeof(double), hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(k_map_colsum, dim3(nu, N), dim3(64), 0, h->stream, (const double*)h->arr[BNMF_P].ring, lenP, K, N, (const int*)dslots, cs);
  if (!qS) {                                              // means (and, beyond 2,048 samples, the bounds) by a lane per element
    const size_t lds = (size_t)kt * 2 * 64 * sizeof(double);
    if (int rc = opt_in_lds(k_map_stats<0>, lds)) return rc;
    if (int rc = opt_in_lds(k_map_stats<1>, lds)) return rc;
    hipLaunchKernelGGL(k_map_stats<0>, dim3((unsigned)((lenP + 63) / 64)), dim3(64), lds, h->stream, (const double*)h->arr[BNMF_P].ring, lenP, K, N,
                       (const int*)dslots, nu, (const double*)cs, kt, jlo, glo, jhi, ghi, mP, loP, hiP);
    hipLaunchKernelGGL(k_map_stats<1>, dim3((unsigned)((lenE + 63) / 64)), dim3(64), lds, h->stream, (const double*)h->arr[BNMF_E].ring, lenE, K, N,
                       (const int*)dslots, nu, (const double*)cs, kt, jlo, glo, jhi, ghi, mE, loE, hiE);
  }
  if (qS) {
    const bool r16 = qS <= 1024;                           // 16 or 32 samples per lane column
    const size_t qS2 = r16 ? 1024 : 2048, qlds = qS2 * MQ_E * sizeof(double) + qS2 * sizeof(int);
    using QuantKernel = decltype(&k_map_quant<0, 16>);
    const QuantKernel q16[2] = {k_map_quant<0, 16>, k_map_quant<1, 16>}, q32[2] = {k_map_quant<0, 32>, k_map_quant<1, 32>};
    const QuantKernel* kquant = r16 ? q16 : q32;           // [side]
    auto go = [&](int side, const double* ring, size_t len, double* mn, double* lo, double* hi) {
      if (int rc = opt_in_lds(kquant[side], qlds, qlds)) return rc;
      hipLaunchKernelGGL(kquant[side], dim3((unsigned)((len + MQ_E - 1) / MQ_E)), dim3(MQ_T), qlds, h->stream, ring, len, K, N, (const int*)dslots, nu,
                         (const double*)cs, jlo, glo, jhi, ghi, mn, lo, hi);
      return 0;
    };
    if (int rc = go(0, h->arr[BNMF_P].ring, lenP, mP, loP, hiP)) return rc;
    if (int rc = go(1, h->arr[BNMF_E].ring, lenE, mE, loE, hiE)) return rc;
  }
  if (h->dMf) hipLaunchKernelGGL(k_map_fit<double>, dim3((G + 3) / 4), dim3(256), 0, h->stream, (const double*)h->dMf, (const double*)mP, (const double*)dA, (const double*)mE, K, N, G, colsse, colkl);
  else hipLaunchKernelGGL(k_map_fit<int32_t>, dim3((G + 3) / 4), dim3(256), 0, h->stream, (const int32_t*)h->dM, (const double*)mP, (const double*)dA, (const double*)mE, K, N, G, colsse, colkl);
  HIPCHK(hipGetLastError());
  if (P_mean) HIPCHK(hipMemcpyAsync(P_mean, mP, lenP * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (E_mean) HIPCHK(hipMemcpyAsync(E_mean, mE, lenE * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (want_ci) {
    if (P_lower) HIPCHK(hipMemcpyAsync(P_lower, loP, lenP * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (P_upper) HIPCHK(hipMemcpyAsync(P_upper, hiP, lenP * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (E_lower) HIPCHK(hipMemcpyAsync(E_lower, loE, lenE * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (E_upper) HIPCHK(hipMemcpyAsync(E_upper, hiE, lenE * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  }
  std::vector<double> col(2 * (size_t)G);
  HIPCHK(hipMemcpyAsync(col.data(), colsse, 2 * (size_t)G * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  double sse = 0.0, kl = 0.0;
  for (int g = 0; g < G; ++g) { sse += col[g]; kl += col[(size_t)G + g]; }
  info->rmse = std::sqrt(sse / ((double)K * (double)G));
  info->kl = kl;
  return 0;
}

// WAIC over the samples of r that used[] flags: k_waic (waic.h) leaves the per-column sums; the totals are their
// sequential sums over g, as map_impl sums colsse.
static int waic_impl(bnmf_handle* h, const char* fn, Range r, const int32_t* used, double* col, double* cell, bnmf_waic_info* info) {
  if (int rc = range_enter(h, fn, h && info, r)) return rc;
  const int K = h->cfg.K, N = h->cfg.N, G = h->cfg.G;
  const bool normal = h->cfg.likelihood == BNMF_NORMAL;
  std::vector<int> slots;
  if (int rc = range_slots(h, fn, r, used, true, slots)) return rc;
  const int S = (int)slots.size();
  if (S < 2) return fail(BNMF_ESIZE, "%s: %d used sample%s, the variance of the log-likelihood needs at least 2", fn, S, S == 1 ? "" : "s");
  if (!h->arr[BNMF_P].ring || !h->arr[BNMF_E].ring || !h->arr[BNMF_A].ring || (normal && !h->arr[BNMF_SIGMASQ].ring))
    return fail(BNMF_ESTATE, "%s: nothing recorded yet", fn);
  if (int rc = post_sync(h)) return rc;
  const size_t KG = (size_t)K * G, ncol = (size_t)WA_NCOL * G;
  double *dcol, *dcell; int* dslots;
  if (int rc = carve(h, [&](Carve& c) { dcol = c.take<double>(ncol); dcell = cell ? c.take<double>(2 * KG) : nullptr; dslots = c.take<int>(S); })) return rc;
  HIPCHK(hipMemcpyAsync(dslots, slots.data(), (size_t)S * sizeof(int), hipMemcpyHostToDevice, h->stream));
  WaicArgs a{};
  a.ringP = h->arr[BNMF_P].ring; a.ringE = h->arr[BNMF_E].ring; a.ringA = h->arr[BNMF_A].ring; a.ringS = normal ? h->arr[BNMF_SIGMASQ].ring : nullptr;
  a.M = h->dM; a.Mf = h->dMf; a.lgfact = h->dLut; a.slots = dslots; a.col = dcol; a.cell = dcell;
  a.lenP = (size_t)K * N; a.lenE = (size_t)N * G; a.K = K; a.N = N; a.G = G; a.S = S; a.maxM = h->maxM;
  size_t lds = waic_lds_bytes(N);
  a.stage = lds <= LDS_CAP ? 1 : 0;
  if (!a.stage) lds = 0;
  const auto kern = normal ? k_waic<true> : k_waic<false>;
  if (int rc = opt_in_lds(kern, lds)) return rc;
  hipLaunchKernelGGL(kern, dim3((unsigned)((G + WA_GC - 1) / WA_GC)), dim3(WA_T), lds, h->stream, a);
  HIPCHK(hipGetLastError());
  std::vector<double> hc(ncol);
  HIPCHK(hipMemcpyAsync(hc.data(), dcol, ncol * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (cell) HIPCHK(hipMemcpyAsync(cell, dcell, 2 * KG * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  double t[WA_NCOL] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int q = 0; q < WA_NCOL; ++q) for (int g = 0; g < G; ++g) t[q] += hc[(size_t)q * G + g];
  if (col) for (int q = 0; q < 3; ++q) std::memcpy(col + (size_t)q * G, hc.data() + (size_t)q * G, (size_t)G * sizeof(double));
  const double n = (double)K * (double)G;
  double var = n > 1.0 ? (t[4] - t[3] * (t[3] / n)) / (n - 1.0) : 0.0;   // variance of elpd over the cells from its two sums
  if (!(var > 0.0)) var = 0.0;
  info->n_used = S; info->n_high_var = (int32_t)t[5];
  info->lppd = t[0]; info->p_waic = t[1]; info->mean_loglik = t[2]; info->elpd_waic = t[3]; info->waic = -2.0 * t[3];
  info->se_elpd = std::sqrt(n * var);
  return 0;
}

// Posterior predictive checks over the samples of r that used[] flags: k_ppc leaves T[4][S][G], the tail cells per column and the cell
// values, k_ppc_totals the per-column rows and the series (ppc.h); the info fields are sequential scans of the series
// on the host.
static_assert(PP_NCOL == BNMF_PPC_NCOL && PP_VAR == (uint32_t)BNMF_V_YREP, "ppc.h and bnmf.h disagree");
static int ppc_impl(bnmf_handle* h, const char* fn, Range r, const int32_t* used, double* col, double* cell, double* series, bnmf_ppc_info* info) {
  if (int rc = range_enter(h, fn, h && info, r)) return rc;
  const int K = h->cfg.K, N = h->cfg.N, G = h->cfg.G;
  const bool normal = h->cfg.likelihood == BNMF_NORMAL;
  std::vector<int> sl;                              // slots, then iterations
  if (int rc = range_slots(h, fn, r, used, true, sl, true)) return rc;
  const int S = (int)sl.size() / 2;
  if (S < 2) return fail(BNMF_ESIZE, "%s: %d used sample%s, the variance of the replicates needs at least 2", fn, S, S == 1 ? "" : "s");
  if (!h->arr[BNMF_P].ring || !h->arr[BNMF_E].ring || !h->arr[BNMF_A].ring || (normal && !h->arr[BNMF_SIGMASQ].ring))
    return fail(BNMF_ESTATE, "%s: nothing recorded yet", fn);
  if (int rc = post_sync(h)) return rc;
  const size_t KG = (size_t)K * G, SG = (size_t)S * G, ncol = (size_t)(PP_NCOL + 1) * G;
  double *dT, *dcol, *dser, *dcell; int* dsl;
  if (int rc = carve(h, [&](Carve& c) {
        dT = c.take<double>(4 * SG); dcol = c.take<double>(ncol); dser = c.take<double>(4 * (size_t)S);
        dcell = cell ? c.take<double>(4 * KG) : nullptr; dsl = c.take<int>(2 * (size_t)S);
      })) return rc;
  HIPCHK(hipMemcpyAsync(dsl, sl.data(), 2 * (size_t)S * sizeof(int), hipMemcpyHostToDevice, h->stream));
  PpcArgs a{};
  a.ringP = h->arr[BNMF_P].ring; a.ringE = h->arr[BNMF_E].ring; a.ringA = h->arr[BNMF_A].ring; a.ringS = normal ? h->arr[BNMF_SIGMASQ].ring : nullptr;
  a.M = h->dM; a.Mf = h->dMf; a.slots = dsl; a.iters = dsl + S; a.T = dT; a.tail = dcol + (size_t)PP_NCOL * G; a.cell = dcell;
  a.lenP = (size_t)K * N; a.lenE = (size_t)N * G; a.K = K; a.N = N; a.G = G; a.S = S;
  a.k0 = (uint32_t)h->cfg.seed; a.k1 = (uint32_t)(h->cfg.seed >> 32) ^ h->cfg.chain_id;
  size_t lds = ppc_lds_bytes(N);
  a.stage = lds <= LDS_CAP ? 1 : 0;
  if (!a.stage) lds = 0;
  const auto kern = normal ? k_ppc<true> : k_ppc<false>;
  const auto ktot = normal ? k_ppc_totals<true> : k_ppc_totals<false>;
  if (int rc = opt_in_lds(kern, lds)) return rc;
  hipLaunchKernelGGL(kern, dim3((unsigned)((G + PP_GC - 1) / PP_GC)), dim3(PP_T), lds, h->stream, a);
  hipLaunchKernelGGL(ktot, dim3((unsigned)(4 * S + (G + PP_TT - 1) / PP_TT)), dim3(PP_TT), 0, h->stream, (const double*)dT, S, G, dser, dcol);
  HIPCHK(hipGetLastError());
  std::vector<double> hs(4 * (size_t)S), ht((size_t)G);
  HIPCHK(hipMemcpyAsync(hs.data(), dser, 4 * (size_t)S * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(ht.data(), dcol + (size_t)PP_NCOL * G, (size_t)G * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (col) HIPCHK(hipMemcpyAsync(col, dcol, (size_t)PP_NCOL * G * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (cell) HIPCHK(hipMemcpyAsync(cell, dcell, 4 * KG * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  if (series) std::memcpy(series, hs.data(), 4 * (size_t)S * sizeof(double));
  double t[4] = {0.0, 0.0, 0.0, 0.0}; int n1 = 0, n2 = 0;
  for (int s = 0; s < S; ++s) {
    for (int q = 0; q < 4; ++q) t[q] += hs[(size_t)q * S + s];
    n1 += hs[(size_t)S + s] >= hs[s] ? 1 : 0; n2 += hs[3 * (size_t)S + s] >= hs[2 * (size_t)S + s] ? 1 : 0;
  }
  int64_t nt = 0;
  for (int g = 0; g < G; ++g) nt += (int64_t)ht[g];
  info->n_used = S; info->n_tail_cells = nt;
  info->p_T1 = (double)n1 / (double)S; info->p_T2 = (double)n2 / (double)S;
  info->mean_T1_obs = t[0] / (double)S; info->mean_T1_rep = t[1] / (double)S; info->mean_T2_obs = t[2] / (double)S; info->mean_T2_rep = t[3] / (double)S;
  return 0;
}

// Signature attribution over the samples of r that used[] flags: per batch of samples k_attr leaves a_s[n,g] in the scratch,
// k_attr_share the reciprocal column totals, k_attr_stats continues the per-(n, g) statistics (zeroed by the first batch: a.first)
// and reduces the series (attribution.h); total and n_present are sequential scans on the host.
static_assert(AT_NLOAD == BNMF_ATTR_NLOAD, "attribution.h and bnmf.h disagree");
static constexpr size_t ATTR_SCRATCH_CAP = (size_t)256 << 20;   // bytes of a_s and u per batch
static int attr_impl(bnmf_handle* h, const char* fn, Range r, const int32_t* used, double min_load, double* load, double* prob, double* series,
                     bnmf_attr_info* info) {
  if (int rc = range_enter(h, fn, h && info, r)) return rc;
  const int K = h->cfg.K, N = h->cfg.N, G = h->cfg.G;
  const bool normal = h->cfg.likelihood == BNMF_NORMAL;
  if (!(min_load >= 0.0) || std::isinf(min_load)) return fail(BNMF_EINVAL, "%s: min_load = %g is not a finite number >= 0", fn, min_load);
  std::vector<int> slots;
  if (int rc = range_slots(h, fn, r, used, true, slots)) return rc;
  const int S = (int)slots.size();
  if (S < 2) return fail(BNMF_ESIZE, "%s: %d used sample%s, the variance of the loads needs at least 2", fn, S, S == 1 ? "" : "s");
  if (!h->arr[BNMF_P].ring || !h->arr[BNMF_E].ring || !h->arr[BNMF_A].ring) return fail(BNMF_ESTATE, "%s: nothing recorded yet", fn);
  if (int rc = post_sync(h)) return rc;
  const size_t NG = (size_t)N * G, KNG = (size_t)K * NG, per = (NG + (size_t)G) * sizeof(double);   // scratch bytes of one sample
  long long want = (long long)std::max<size_t>(1, ATTR_SCRATCH_CAP / per);
  if (const char* e = getenv("BNMF_ATTR_BATCH")) { const long long v = atoll(e); if (v >= 1) want = v; }   // tests: the batch size
  const int Sb = (int)std::min<long long>(want, S);
  double *dscr, *du, *dst, *dload, *dser, *dprob; int* dslots;
  if (int rc = carve(h, [&](Carve& c) {
        dscr = c.take<double>((size_t)Sb * NG); du = c.take<double>((size_t)Sb * G); dst = c.take<double>(AT_NLOAD * NG);
        dload = c.take<double>(AT_NLOAD * NG); dser = c.take<double>((size_t)S * N); dprob = prob ? c.take<double>(KNG) : nullptr;
        dslots = c.take<int>(S);
      })) return rc;
  HIPCHK(hipMemcpyAsync(dslots, slots.data(), (size_t)S * sizeof(int), hipMemcpyHostToDevice, h->stream));
  AttrArgs a{};
  a.ringP = h->arr[BNMF_P].ring; a.ringE = h->arr[BNMF_E].ring; a.ringA = h->arr[BNMF_A].ring; a.M = h->dM; a.scr = dscr; a.prob = dprob;
  a.lenP = (size_t)K * N; a.lenE = NG; a.K = K; a.N = N; a.G = G; a.S = S;
  size_t lds = attr_lds_bytes(N);
  a.stage = lds <= LDS_CAP ? 1 : 0;
  if (!a.stage) lds = 0;
  const auto kern = normal ? (prob ? k_attr<true, true> : k_attr<true, false>) : (prob ? k_attr<false, true> : k_attr<false, false>);
  if (int rc = opt_in_lds(kern, lds)) return rc;
  const dim3 grid((unsigned)((G + AT_GC - 1) / AT_GC)), block(AT_T);
  for (int s0 = 0; s0 < S; s0 += Sb) {
    const int nb = std::min(Sb, S - s0), last = s0 + nb == S ? 1 : 0;
    a.slots = dslots + s0; a.Sb = nb; a.first = s0 == 0 ? 1 : 0; a.last = last;
    hipLaunchKernelGGL(kern, grid, block, lds, h->stream, a);
    const size_t nsg = (size_t)nb * G;
    hipLaunchKernelGGL(k_attr_share, dim3((unsigned)((nsg + 255) / 256)), dim3(256), 0, h->stream, (const double*)dscr, nb, N, G, du);
    hipLaunchKernelGGL(k_attr_stats, dim3((unsigned)((size_t)nb * N + (NG + AT_TT - 1) / AT_TT)), dim3(AT_TT), 0, h->stream, (const double*)dscr,
                       (const double*)du, nb, N, G, S, s0, last, min_load, dst, dser, dload);
    HIPCHK(hipGetLastError());
  }
  std::vector<double> hs((size_t)S * N), hp(NG);
  HIPCHK(hipMemcpyAsync(hs.data(), dser, (size_t)S * N * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(hp.data(), dload + 3 * NG, NG * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (load) HIPCHK(hipMemcpyAsync(load, dload, AT_NLOAD * NG * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (prob) HIPCHK(hipMemcpyAsync(prob, dprob, KNG * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  if (series) std::memcpy(series, hs.data(), (size_t)S * N * sizeof(double));
  double t = 0.0;
  for (size_t i = 0; i < (size_t)S * N; ++i) t += hs[i];
  int64_t np = 0;
  for (size_t i = 0; i < NG; ++i) np += hp[i] >= 0.5 ? 1 : 0;
  info->n_used = S; info->_pad = 0; info->n_present = np; info->min_load = min_load; info->total = t / (double)S;
  return 0;
}

// Mixing diagnostics over the samples of r that used[] flags: k_map_colsum, then k_mixing (mixing.h) per side leaves the
// per-element rows; the summary is a sequential scan of them on the host, element index ascending, P then E, over the factors that
// keep[] flags.
static_assert(BNMF_NMIX == MX_NROW, "bnmf.h and mixing.h disagree on the rows of the per-element output");
static int mixing_impl(bnmf_handle* h, const char* fn, Range r, const int32_t* used, const int32_t* keep, double* P_out, double* E_out,
                       bnmf_mixing_info* info) {
  if (int rc = range_enter(h, fn, h && info, r)) return rc;
  const int K = h->cfg.K, N = h->cfg.N, G = h->cfg.G;
  std::vector<int> slots;
  if (int rc = range_slots(h, fn, r, used, true, slots)) return rc;
  if (keep) for (int n = 0; n < N; ++n) if (keep[n] != 0 && keep[n] != 1) return fail(BNMF_EINVAL, "%s: keep[%d] = %d is neither 0 nor 1", fn, n, (int)keep[n]);
  const int S = (int)slots.size();
  if (S < 4) return fail(BNMF_ESIZE, "%s: %d used sample%s, split R-hat needs at least 4 (a variance in each half)", fn, S, S == 1 ? "" : "s");
  static_assert(BNMF_MIXING_MAX_SAMPLES * (sizeof(double) + sizeof(int)) <= MX_LDS, "one element's series and the slot list fit the LDS");
  if (S > BNMF_MIXING_MAX_SAMPLES)
    return fail(BNMF_ESIZE, "%s: %d used samples but at most %d fit the device's 160 KB of LDS per element: thin the range with used[]", fn, S, BNMF_MIXING_MAX_SAMPLES);
  if (!h->arr[BNMF_P].ring || !h->arr[BNMF_E].ring) return fail(BNMF_ESTATE, "%s: nothing recorded yet", fn);
  if (int rc = post_sync(h)) return rc;
  const size_t lenP = (size_t)K * N, lenE = (size_t)N * G;
  double *cs, *oP, *oE; int* dslots;
  if (int rc = carve(h, [&](Carve& c) {
        cs = c.take<double>((size_t)S * N); oP = c.take<double>(MX_NROW * lenP); oE = c.take<double>(MX_NROW * lenE); dslots = c.take<int>(S);
      })) return rc;
  HIPCHK(hipMemcpyAsync(dslots, slots.data(), (size_t)S * sizeof(int), hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(k_map_colsum, dim3(S, N), dim3(64), 0, h->stream, (const double*)h->arr[BNMF_P].ring, lenP, K, N, (const int*)dslots, cs);
  const int epw = mixing_elements_per_group(S);
  const size_t lds = mixing_lds_bytes(epw, S);
  const double tau_min = 1.0 / std::log10((double)S);
  if (int rc = opt_in_lds(k_mixing<0>, lds, MX_LDS)) return rc;
  if (int rc = opt_in_lds(k_mixing<1>, lds, MX_LDS)) return rc;
  hipLaunchKernelGGL(k_mixing<0>, dim3((unsigned)((lenP + epw - 1) / epw)), dim3(64 * epw), lds, h->stream, (const double*)h->arr[BNMF_P].ring, lenP, K, N,
                     (const int*)dslots, S, (const double*)cs, tau_min, epw, oP);
  hipLaunchKernelGGL(k_mixing<1>, dim3((unsigned)((lenE + epw - 1) / epw)), dim3(64 * epw), lds, h->stream, (const double*)h->arr[BNMF_E].ring, lenE, K, N,
                     (const int*)dslots, S, (const double*)cs, tau_min, epw, oE);
  HIPCHK(hipGetLastError());
  std::vector<double> hP, hE;                       // the summary needs the rows whether or not the caller wants them
  if (!P_out) { hP.resize(MX_NROW * lenP); P_out = hP.data(); }
  if (!E_out) { hE.resize(MX_NROW * lenE); E_out = hE.data(); }
  HIPCHK(hipMemcpyAsync(P_out, oP, MX_NROW * lenP * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(E_out, oE, MX_NROW * lenE * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  std::memset(info, 0, sizeof *info);
  info->n_used = S; info->n_half = S / 2;
  const double nan = std::nan("");
  info->min_ess_P = info->min_ess_E = info->max_rhat_P = info->max_rhat_E = nan;
  info->min_ess_P_at = info->min_ess_E_at = info->max_rhat_P_at = info->max_rhat_E_at = -1;
  auto scan = [&](const double* o, size_t len, bool sideE, double& mn, int64_t& mn_at, double& mx, int64_t& mx_at) {
    for (size_t e = 0; e < len; ++e) {
      const int n = sideE ? (int)(e % (size_t)N) : (int)(e / (size_t)K);
      if (keep && !keep[n]) continue;
      const double ess = o[2 * len + e], rhat = o[4 * len + e];
      if (o[5 * len + e] == 0.0) info->n_const++;
      if (o[6 * len + e] == 1.0) info->n_ran_out++;
      if (ess < BNMF_MIXING_LOW_ESS) info->n_low_ess++;
      if (rhat > BNMF_MIXING_HIGH_RHAT) info->n_high_rhat++;
      if (!std::isnan(ess) && (mn_at < 0 || ess < mn)) { mn = ess; mn_at = (int64_t)e; }
      if (!std::isnan(rhat) && (mx_at < 0 || rhat > mx)) { mx = rhat; mx_at = (int64_t)e; }
    }
  };
  scan(P_out, lenP, false, info->min_ess_P, info->min_ess_P_at, info->max_rhat_P, info->max_rhat_P_at);
  scan(E_out, lenE, true, info->min_ess_E, info->min_ess_E_at, info->max_rhat_E, info->max_rhat_E_at);
  return 0;
}

static double quantile7(std::vector<double> x, double prob) {
  std::sort(x.begin(), x.end());
  const double hq = (x.size() - 1) * prob;
  const size_t j = (size_t)std::floor(hq);
  const double g = hq - (double)j;
  const double a = x[j], b = x[std::min(j + 1, x.size() - 1)];
  return a == b ? a : (1.0 - g) * a + g * b;              // k_map_quant's map_interp
}

// assign_signatures_ensemble_ over the samples of r that used[] flags (any non-zero value).  Its preconditions have their own wording:
// bnmf_assign refuses a handle without a P ring as one without a window, before it looks at last_n.
static int assign_impl(bnmf_handle* h, const char* fn, Range r, const int32_t* used, const double* ref, int R, const int32_t* keep, const double* MAP_P,
                       double ci, double* votes, int32_t* assigned, double* MAP_cosine, double* lower, double* upper) {
  if (!h || !ref || !votes || !assigned) return fail(BNMF_EINVAL, "%s: null argument", fn);
  if (int rc = check_alive(h, fn)) return rc;
  if (!r.at) {
    if (h->cfg.window <= 0 || !h->arr[BNMF_P].ring) return fail(BNMF_ESTATE, "bnmf_assign: no recorded samples (window = 0)");
  } else {
    if (int rc = check_recorded(h, fn)) return rc;
    if (!h->arr[BNMF_P].ring) return fail(BNMF_ESTATE, "bnmf_assign_at: nothing recorded yet");
  }
  if (int rc = range_resolve(h, fn, r)) return rc;
  if (R < 1) return fail(BNMF_EINVAL, "bnmf_assign: empty reference");
  const int K = h->cfg.K, N = h->cfg.N;
  std::vector<int> slots, sig;
  if (int rc = range_slots(h, fn, r, used, false, slots)) return rc;
  for (int n = 0; n < N; ++n) if (!keep || keep[n]) sig.push_back(n);
  const int nu = (int)slots.size(), nk = (int)sig.size();
  for (int i = 0; i < N * R; ++i) votes[i] = 0.0;
  for (int n = 0; n < N; ++n) { assigned[n] = -1; if (MAP_cosine) MAP_cosine[n] = std::nan(""); if (lower) lower[n] = std::nan(""); if (upper) upper[n] = std::nan(""); }
  if (nu == 0 || nk == 0) return 0;
  if (int rc = post_sync(h)) return rc;
  const size_t nout = (size_t)nu * nk * R;
  // one Hungarian assignment per sample (maximise the total cosine), one wave each; with more signatures than references the
  // references are the rows
  const bool tr = nk > R;
  const int nrow = tr ? R : nk, ncol = tr ? nk : R;
  double *dRef, *dN2, *dOut; int *dSl, *dSig; int32_t* dCol;
  if (int rc = carve(h, [&](Carve& c) {
        dRef = c.take<double>((size_t)K * R); dN2 = c.take<double>(R); dOut = c.take<double>(nout);
        dSl = c.take<int>(nu); dSig = c.take<int>(nk); dCol = c.take<int32_t>((size_t)nu * nrow);
      })) return rc;
  std::vector<double> rn2;
  if (int rc = catalogue_upload(ref, K, R, dRef, dN2, rn2)) return rc;
  HIPCHK(hipMemcpy(dSl, slots.data(), nu * sizeof(int), hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(dSig, sig.data(), nk * sizeof(int), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_ref_cosine, dim3(nu, nk), dim3(128), 0, h->stream, (const double*)h->arr[BNMF_P].ring, (size_t)K * N, K, (const int*)dSl,
                     (const int*)dSig, nk, (const double*)dRef, (const double*)dN2, R, dOut);
  HIPCHK(hipGetLastError());
  const size_t hung_lds = hungarian_lds_bytes(nrow, ncol);
  if (hung_lds > LDS_CAP) return fail(BNMF_ESIZE, "bnmf_assign: %d x %d assignment problem exceeds the LDS of one workgroup", nrow, ncol);
  if (int rc = opt_in_lds(k_hungarian, hung_lds, hung_lds)) return rc;
  HIPCHK(hipMemsetAsync(dCol, 0xff, (size_t)nu * nrow * sizeof(int32_t), h->stream));
  hipLaunchKernelGGL(k_hungarian, dim3(nu), dim3(64), hung_lds, h->stream, (const double*)dOut, nk, R, tr ? 1 : 0, dCol);
  HIPCHK(hipGetLastError());
  std::vector<double> cosv(nout);
  std::vector<int32_t> col((size_t)nu * nrow);
  HIPCHK(hipMemcpyAsync(cosv.data(), dOut, nout * 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(col.data(), dCol, col.size() * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  // the cosine of a chosen pair is its vote; the votes are summed in sample order
  for (int s = 0; s < nu; ++s) {
    const double* c = cosv.data() + (size_t)s * nk * R;
    const int32_t* a = col.data() + (size_t)s * nrow;
    for (int i = 0; i < nrow; ++i) if (a[i] < 0 || a[i] >= ncol) return fail(BNMF_ESTATE, "bnmf_assign: sample %d has no assignment (a cosine is not finite)", s);
    if (!tr) for (int i = 0; i < nk; ++i) votes[sig[i] + (size_t)N * a[i]] += c[(size_t)i * R + a[i]];
    else for (int j = 0; j < R; ++j) votes[sig[a[j]] + (size_t)N * j] += c[(size_t)a[j] * R + j];
  }
  for (int i = 0; i < nk; ++i) {                           // which.max(prop_votes): first maximum
    const int n = sig[i];
    int best = -1; double bv = 0.0;
    for (int j = 0; j < R; ++j) if (votes[n + (size_t)N * j] > bv) { bv = votes[n + (size_t)N * j]; best = j; }
    assigned[n] = best;
    if (best < 0) continue;
    if (MAP_P && MAP_cosine) {
      double dot = 0.0, nn = 0.0;
      for (int k = 0; k < K; ++k) { const double p = MAP_P[k + (size_t)K * n]; dot += p * ref[k + (size_t)K * best]; nn += p * p; }
      MAP_cosine[n] = dot / std::sqrt(nn * rn2[best]);
    }
    if (ci > 0.0 && ci < 1.0 && (lower || upper)) {
      std::vector<double> x(nu);
      for (int s = 0; s < nu; ++s) x[s] = cosv[((size_t)s * nk + i) * R + best];
      if (lower) lower[n] = quantile7(x, (1.0 - ci) / 2.0);
      if (upper) upper[n] = quantile7(x, 1.0 - (1.0 - ci) / 2.0);
    }
  }
  return 0;
}

// Label-switching correction over the samples of r that used[] flags: per round k_rl_pivot, the matching (k_rl_match, or past the LDS
// k_ref_cosine + k_hungarian + k_rl_finish over chunks of samples), k_rl_compact, then the two counts come to the host; between rounds
// k_rl_accum leaves the next pivot, after the last round the aligned mean and variance of both sides (relabel.h).
// confusion and the summary are sequential scans on the host.
static_assert(BNMF_NREL == RL_NROW, "bnmf.h and relabel.h disagree on the rows of the output");
static const size_t LS_CHUNK_BYTES = (size_t)256 << 20;         // bytes of cosines per chunk of samples, past the LDS (also bnmf_label_switching)
static constexpr size_t REL_SCRATCH_CAP = (size_t)256 << 20;    // bytes of aligned samples per batch
static int relabel_impl(bnmf_handle* h, const char* fn, Range r, const int32_t* used, const double* pivot_P, int max_rounds, int32_t* perm,
                        double* cosine, int64_t* confusion, double* P_out, double* E_out, double* aligned_P, double* aligned_E, bnmf_relabel_info* info) {
  if (int rc = range_enter(h, fn, h && info, r)) return rc;
  const int K = h->cfg.K, N = h->cfg.N, G = h->cfg.G;
  std::vector<int> slots;
  if (int rc = range_slots(h, fn, r, used, true, slots)) return rc;
  if (max_rounds < 1) return fail(BNMF_EINVAL, "%s: max_rounds = %d, at least 1 round is needed", fn, max_rounds);
  if (pivot_P)
    for (int j = 0; j < N; ++j) {
      bool zero = true;
      for (int k = 0; k < K; ++k) {
        const double v = pivot_P[(size_t)k + (size_t)K * j];
        if (!std::isfinite(v)) return fail(BNMF_EINVAL, "%s: column %d of pivot_P holds a value that is not finite (row %d)", fn, j, k);
        zero = zero && v == 0.0;
      }
      if (zero) return fail(BNMF_EINVAL, "%s: column %d of pivot_P is all zero: it has no cosine", fn, j);
    }
  const int S = (int)slots.size();
  if (S < 2) return fail(BNMF_ESIZE, "%s: %d used sample%s, an aligned variance needs at least 2", fn, S, S == 1 ? "" : "s");
  const size_t hung_lds = relabel_hung_lds(N), match_lds = relabel_match_lds(N);
  const bool fused = match_lds <= RL_LDS;
  if (!fused && hung_lds > RL_LDS) return fail(BNMF_ESIZE, "%s: the %d x %d assignment problem exceeds the LDS of one workgroup", fn, N, N);
  if (!h->arr[BNMF_P].ring || !h->arr[BNMF_E].ring) return fail(BNMF_ESTATE, "%s: nothing recorded yet", fn);
  if (int rc = post_sync(h)) return rc;
  const size_t lenP = (size_t)K * N, lenE = (size_t)N * G, SN = (size_t)S * N, per = (size_t)N * N * sizeof(double);
  const int chunk = fused ? 0 : (int)std::max<size_t>(1, std::min<size_t>((size_t)S, LS_CHUNK_BYTES / per));
  // the aligned samples leave in batches of whole samples, P then E through the same scratch
  const int bP = aligned_P ? (int)std::min<size_t>({(size_t)S, (size_t)65535, std::max<size_t>(1, REL_SCRATCH_CAP / (lenP * sizeof(double)))}) : 0;
  const int bE = aligned_E ? (int)std::min<size_t>({(size_t)S, (size_t)65535, std::max<size_t>(1, REL_SCRATCH_CAP / (lenE * sizeof(double)))}) : 0;
  double *dRef, *dN2, *dPiv, *cs, *oP, *oE, *dCs, *dCv, *dBat; int32_t *dPerm, *dInv, *dFlag, *dCol; int *dAl, *dSl, *dCnt, *dSig;
  if (int rc = carve(h, [&](Carve& c) {
        dRef = c.take<double>(lenP); dN2 = c.take<double>(N); dPiv = c.take<double>(lenP); cs = c.take<double>(SN);
        oP = c.take<double>(RL_NROW * lenP); oE = c.take<double>(RL_NROW * lenE); dCs = c.take<double>(SN);
        dPerm = c.take<int32_t>(SN); dInv = c.take<int32_t>(SN); dFlag = c.take<int32_t>(S);
        dAl = c.take<int>(S); dSl = c.take<int>(S); dCnt = c.take<int>(4); dSig = c.take<int>(N);
        dCv = c.take<double>((size_t)chunk * N * N); dCol = c.take<int32_t>((size_t)chunk * N);
        dBat = c.take<double>(std::max((size_t)bP * lenP, (size_t)bE * lenE));
      })) return rc;
  const double* ringP = h->arr[BNMF_P].ring;
  const double* ringE = h->arr[BNMF_E].ring;
  HIPCHK(hipMemcpyAsync(dSl, slots.data(), (size_t)S * sizeof(int), hipMemcpyHostToDevice, h->stream));
  if (pivot_P) HIPCHK(hipMemcpyAsync(dPiv, pivot_P, lenP * sizeof(double), hipMemcpyHostToDevice, h->stream));
  if (!fused) {
    std::vector<int> sig(N);
    for (int n = 0; n < N; ++n) sig[n] = n;
    HIPCHK(hipMemcpy(dSig, sig.data(), (size_t)N * sizeof(int), hipMemcpyHostToDevice));
    if (int rc = opt_in_lds(k_hungarian, hung_lds, hung_lds)) return rc;
  } else if (int rc = opt_in_lds(k_rl_match, match_lds, match_lds)) return rc;
  hipLaunchKernelGGL(k_map_colsum, dim3(S, N), dim3(64), 0, h->stream, ringP, lenP, K, N, (const int*)dSl, cs);
  const size_t tab = relabel_tab_bytes(S, N);
  const bool stage = tab <= RL_TAB_LDS;
  using AccumKernel = decltype(&k_rl_accum<0, true>);
  const AccumKernel staged[2] = {k_rl_accum<0, true>, k_rl_accum<1, true>}, direct[2] = {k_rl_accum<0, false>, k_rl_accum<1, false>};
  const AccumKernel* kaccum = stage ? staged : direct;     // [side]
  if (stage) for (int side = 0; side < 2; ++side) if (int rc = opt_in_lds(kaccum[side], tab, RL_TAB_LDS)) return rc;
  auto accum = [&](int side, int want_var) {
    const double* ring = side ? ringE : ringP;
    const size_t len = side ? lenE : lenP;
    const dim3 grid((unsigned)((len + (size_t)RL_E * (RL_AT / 64) - 1) / ((size_t)RL_E * (RL_AT / 64)))), block(RL_AT);
    hipLaunchKernelGGL(kaccum[side], grid, block, stage ? tab : 0, h->stream, ring, len, K, N, (const int*)dSl, (const int*)dAl, (const int*)dCnt,
                       (const int32_t*)dInv, (const double*)cs, want_var, side ? oE : oP);
  };
  const double* piv = pivot_P ? dPiv : ringP + (size_t)slots[S - 1] * lenP;      // NULL: the newest used sample's P
  int rounds = 0, converged = 0, cnt[2] = {0, 0};
  for (int rd = 1; rd <= max_rounds; ++rd) {
    const int first = rd == 1 ? 1 : 0;
    hipLaunchKernelGGL(k_rl_pivot, dim3((N + 63) / 64), dim3(64), 0, h->stream, piv, K, N, dRef, dN2);
    if (fused) {
      hipLaunchKernelGGL(k_rl_match, dim3(S), dim3(64), match_lds, h->stream, ringP, K, N, (const int*)dSl, (const double*)dRef, (const double*)dN2, first,
                         dPerm, dInv, dCs, dFlag);
    } else {
      for (int s0 = 0; s0 < S; s0 += chunk) {
        const int ns = std::min(chunk, S - s0);
        hipLaunchKernelGGL(k_ref_cosine, dim3(ns, N), dim3(128), 0, h->stream, ringP, lenP, K, (const int*)dSl + s0, (const int*)dSig, N,
                           (const double*)dRef, (const double*)dN2, N, dCv);
        HIPCHK(hipMemsetAsync(dCol, 0xff, (size_t)ns * N * sizeof(int32_t), h->stream));
        hipLaunchKernelGGL(k_hungarian, dim3(ns), dim3(64), hung_lds, h->stream, (const double*)dCv, N, N, 0, dCol);
        hipLaunchKernelGGL(k_rl_finish, dim3((ns + 63) / 64), dim3(64), 0, h->stream, (const double*)dCv, (const int32_t*)dCol, N, ns, first,
                           dPerm + (size_t)s0 * N, dInv + (size_t)s0 * N, dCs + (size_t)s0 * N, dFlag + s0);
      }
    }
    hipLaunchKernelGGL(k_rl_compact, dim3(1), dim3(64), 0, h->stream, (const int32_t*)dFlag, S, dAl, dCnt);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(cnt, dCnt, sizeof cnt, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    rounds = rd;
    if (cnt[0] < 2)
      return fail(BNMF_ESIZE, "%s: %d of the %d used samples could be aligned in round %d (a cosine that is not finite leaves a sample unmatched), at least 2 are needed",
                  fn, cnt[0], S, rd);
    if (cnt[1] == 0) { converged = 1; break; }
    if (rd == max_rounds) break;
    accum(0, 0);                                           // the next pivot: the aligned mean of the renormalised P
    piv = oP;
  }
  accum(0, 1);
  accum(1, 1);
  HIPCHK(hipGetLastError());
  std::vector<int32_t> hperm(SN);
  std::vector<double> hcos(SN);
  HIPCHK(hipMemcpyAsync(hperm.data(), dPerm, SN * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(hcos.data(), dCs, SN * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (P_out) HIPCHK(hipMemcpyAsync(P_out, oP, RL_NROW * lenP * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (E_out) HIPCHK(hipMemcpyAsync(E_out, oE, RL_NROW * lenE * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  auto gather = [&](int side, int nbmax, double* dst) -> int {
    const size_t len = side ? lenE : lenP;
    const auto kern = side ? k_rl_gather<1> : k_rl_gather<0>;
    for (int s0 = 0; s0 < S; s0 += nbmax) {
      const int nb = std::min(nbmax, S - s0);
      hipLaunchKernelGGL(kern, dim3((unsigned)((len + 255) / 256), (unsigned)nb), dim3(256), 0, h->stream, side ? ringE : ringP, len, K, N, (const int*)dSl,
                         (const int32_t*)dInv, (const int32_t*)dFlag, (const double*)cs, s0, dBat);
      HIPCHK(hipGetLastError());
      HIPCHK(hipMemcpyAsync(dst + (size_t)s0 * len, dBat, (size_t)nb * len * sizeof(double), hipMemcpyDeviceToHost, h->stream));
      HIPCHK(hipStreamSynchronize(h->stream));               // the next batch overwrites the scratch
    }
    return 0;
  };
  if (aligned_P) if (int rc = gather(0, bP, aligned_P)) return rc;
  if (aligned_E) if (int rc = gather(1, bE, aligned_E)) return rc;
  if (perm) std::memcpy(perm, hperm.data(), SN * sizeof(int32_t));
  if (cosine) std::memcpy(cosine, hcos.data(), SN * sizeof(double));
  if (confusion) for (size_t i = 0; i < (size_t)N * N; ++i) confusion[i] = 0;
  std::memset(info, 0, sizeof *info);
  info->n_used = S; info->n_aligned = cnt[0]; info->n_unmatched = S - cnt[0]; info->rounds = rounds; info->converged = converged;
  info->n_changed_last = cnt[1];
  double acc[64], mn = std::nan("");
  for (int l = 0; l < 64; ++l) acc[l] = 0.0;
  int64_t mn_at = -1;
  size_t t = 0;                                            // place in the (s, n) sequence of the aligned samples' cosines
  for (int s = 0; s < S; ++s) {
    const int32_t* pm = hperm.data() + (size_t)s * N;
    if (N > 0 && pm[0] < 0) continue;                      // unmatched
    bool ident = true;
    for (int n = 0; n < N; ++n) {
      const double c = hcos[(size_t)s * N + n];
      ident = ident && pm[n] == n;
      if (confusion) confusion[(size_t)n * N + pm[n]] += 1;
      acc[t & 63] = acc[t & 63] + c; ++t;
      if (mn_at < 0 || c < mn) { mn = c; mn_at = (int64_t)s * N + n; }
    }
    if (!ident) info->n_switched++;
  }
  for (int hh = 32; hh >= 1; hh >>= 1) for (int l = 0; l < hh; ++l) acc[l] = acc[l] + acc[l + hh];   // wave_tree64's order
  info->mean_cosine = acc[0] / (double)((size_t)cnt[0] * (size_t)N);
  info->min_cosine = mn; info->min_cosine_at = mn_at;
  return 0;
}

// Exposures of new tumours over the samples of r that used[] flags: k_map_colsum once, then per batch of samples k_proj_x (the columns
// of x that take part, side by side), k_project (the refit: a_s[n,j] and the fit values in the scratch), attribution.h's k_attr_share
// and k_attr_stats with G := J, k_proj_fit (project.h); the info fields are sequential scans on the host.
static_assert(BNMF_PROJ_NLOAD == AT_NLOAD && BNMF_PROJ_NFIT == PJ_NFIT && BNMF_PROJ_MAX_N == PJ_MAX_N, "project.h, attribution.h and bnmf.h disagree");
static constexpr size_t PROJ_SCRATCH_CAP = (size_t)256 << 20;   // bytes of a batch's blocks of the scratch
static int project_impl(bnmf_handle* h, const char* fn, Range r, const int32_t* used, const double* X, int J, int n_steps, double min_load, double* load,
                        double* fit, double* series, double* exposures, bnmf_project_info* info) {
  if (int rc = range_enter(h, fn, h && info && X, r)) return rc;
  const int K = h->cfg.K, N = h->cfg.N;
  if (h->cfg.likelihood == BNMF_NORMAL)
    return fail(BNMF_EMODEL, "%s: the handle has the Normal likelihood; its refit is a different algorithm (least squares, not the KL update) and is out of scope", fn);
  if (J < 1) return fail(BNMF_EINVAL, "%s: J = %d, at least 1 new tumour is needed", fn, J);
  if (n_steps < 1 || n_steps > 100000) return fail(BNMF_EINVAL, "%s: n_steps = %d is not in 1..100000", fn, n_steps);
  if (!(min_load >= 0.0) || std::isinf(min_load)) return fail(BNMF_EINVAL, "%s: min_load = %g is not a finite number >= 0", fn, min_load);
  std::vector<int> slots;
  if (int rc = range_slots(h, fn, r, used, true, slots)) return rc;
  std::vector<double> Xt((size_t)K * J), tX(J);            // X k-major, and t_j = sum_k X[k,j], k ascending from +0.0
  for (int j = 0; j < J; ++j) {
    double t = 0.0;
    for (int k = 0; k < K; ++k) {
      const double v = X[(size_t)k + (size_t)K * j];
      if (!(v >= 0.0) || std::isinf(v)) return fail(BNMF_EINVAL, "%s: X[%d, %d] = %g is not a finite number >= 0", fn, k, j, v);
      Xt[(size_t)k * J + j] = v;
      t = t + v;
    }
    tX[j] = t;
  }
  const int S = (int)slots.size();
  if (S < 2) return fail(BNMF_ESIZE, "%s: %d used sample%s, the variance of the exposures needs at least 2", fn, S, S == 1 ? "" : "s");
  if (N > PJ_MAX_N) return fail(BNMF_ESIZE, "%s: N = %d factors but at most BNMF_PROJ_MAX_N = %d fit a lane's columns of the LDS", fn, N, PJ_MAX_N);
  if (!h->arr[BNMF_P].ring || !h->arr[BNMF_A].ring) return fail(BNMF_ESTATE, "%s: nothing recorded yet", fn);
  if (int rc = post_sync(h)) return rc;
  const int NS = proj_row_stride(N);
  const size_t NJ = (size_t)N * J, KNS = (size_t)K * NS, lenP = (size_t)K * N;
  const size_t per = ((exposures ? 2 : 1) * NJ + (size_t)(1 + PJ_NFIT) * J + KNS + N) * sizeof(double);   // scratch bytes of one sample
  long long want = (long long)std::max<size_t>(1, PROJ_SCRATCH_CAP / per);
  if (const char* e = getenv("BNMF_PROJ_BATCH")) { const long long v = atoll(e); if (v >= 1) want = v; }   // tests: the batch size
  const int Sb = (int)std::min<long long>({want, (long long)S, 65535LL});                                  // (a batch is the grid's y)
  // x staged in the LDS only beside e and g there; with e and g in registers the wave-uniform reads through the caches measured faster
  const bool fits = proj_lds_bytes(K, N, true) <= LDS_CAP;
  bool stage = fits && N > PJ_MAX_NT;
  if (const char* e = getenv("BNMF_PROJ_STAGE")) stage = fits && atoi(e) != 0;                             // tests, tools: the other form
  const size_t lds = proj_lds_bytes(K, N, stage);
  if (lds > LDS_CAP) return fail(BNMF_ESIZE, "%s: N = %d factors need %zu bytes of LDS", fn, N, lds);      // (unreachable for N <= BNMF_PROJ_MAX_N)
  double *cs, *dXt, *dtX, *dxg, *dscr, *dfs, *du, *dst, *dload, *dser, *dfst, *dfit, *dexp; int *dslots, *dnin, *didx;
  if (int rc = carve(h, [&](Carve& c) {
        cs = c.take<double>((size_t)S * N); dXt = c.take<double>((size_t)K * J); dtX = c.take<double>(J); dxg = c.take<double>((size_t)Sb * KNS);
        dscr = c.take<double>((size_t)Sb * NJ); dfs = c.take<double>((size_t)Sb * PJ_NFIT * J); du = c.take<double>((size_t)Sb * J);
        dst = c.take<double>(AT_NLOAD * NJ); dload = c.take<double>(AT_NLOAD * NJ); dser = c.take<double>((size_t)S * N);
        dfst = c.take<double>((size_t)PJ_NFIT * J); dfit = c.take<double>((size_t)PJ_NFIT * J);
        dexp = exposures ? c.take<double>((size_t)Sb * NJ) : nullptr;
        dslots = c.take<int>(S); dnin = c.take<int>(Sb); didx = c.take<int>((size_t)Sb * N);
      })) return rc;
  HIPCHK(hipMemcpyAsync(dslots, slots.data(), (size_t)S * sizeof(int), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(dXt, Xt.data(), Xt.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(dtX, tX.data(), tX.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
  const double* ringP = h->arr[BNMF_P].ring;
  hipLaunchKernelGGL(k_map_colsum, dim3(S, N), dim3(64), 0, h->stream, ringP, lenP, K, N, (const int*)dslots, cs);
  using ProjKernel = decltype(&k_project<8, true>);
  const ProjKernel staged[5] = {k_project<0, true>, k_project<8, true>, k_project<16, true>, k_project<24, true>, k_project<32, true>};
  const ProjKernel direct[5] = {k_project<0, false>, k_project<8, false>, k_project<16, false>, k_project<24, false>, k_project<32, false>};
  const ProjKernel kern = (stage ? staged : direct)[N <= PJ_MAX_NT ? NS / 8 : 0];
  if (int rc = opt_in_lds(kern, lds)) return rc;
  const int T = N <= PJ_MAX_NT ? PJ_T : PJ_TL;
  for (int s0 = 0; s0 < S; s0 += Sb) {
    const int nb = std::min(Sb, S - s0), first = s0 == 0 ? 1 : 0, last = s0 + nb == S ? 1 : 0;
    hipLaunchKernelGGL(k_proj_x, dim3(nb), dim3(256), 0, h->stream, ringP, (const double*)h->arr[BNMF_A].ring, lenP, K, N, NS, (const int*)dslots + s0,
                       (const double*)cs + (size_t)s0 * N, dxg, dnin, didx);
    hipLaunchKernelGGL(kern, dim3((unsigned)((J + T - 1) / T), (unsigned)nb), dim3(T), lds, h->stream, (const double*)dxg, (const int*)dnin, (const int*)didx,
                       (const double*)dXt, (const double*)dtX, K, N, J, n_steps, dscr, dfs);
    const size_t nsj = (size_t)nb * J;
    hipLaunchKernelGGL(k_attr_share, dim3((unsigned)((nsj + 255) / 256)), dim3(256), 0, h->stream, (const double*)dscr, nb, N, J, du);
    hipLaunchKernelGGL(k_attr_stats, dim3((unsigned)((size_t)nb * N + (NJ + AT_TT - 1) / AT_TT)), dim3(AT_TT), 0, h->stream, (const double*)dscr,
                       (const double*)du, nb, N, J, S, s0, last, min_load, dst, dser, dload);
    hipLaunchKernelGGL(k_proj_fit, dim3((unsigned)((J + 255) / 256)), dim3(256), 0, h->stream, (const double*)dfs, nb, J, S, first, last, dfst, dfit);
    HIPCHK(hipGetLastError());
    if (exposures) {
      hipLaunchKernelGGL(k_proj_exposures, dim3((unsigned)(((size_t)nb * NJ + 255) / 256)), dim3(256), 0, h->stream, (const double*)dscr, nb, N, J, dexp);
      HIPCHK(hipGetLastError());
      HIPCHK(hipMemcpyAsync(exposures + (size_t)s0 * NJ, dexp, (size_t)nb * NJ * sizeof(double), hipMemcpyDeviceToHost, h->stream));
      HIPCHK(hipStreamSynchronize(h->stream));             // the next batch overwrites the scratch
    }
  }
  std::vector<double> hs((size_t)S * N), hp(NJ), hf((size_t)PJ_NFIT * J);
  HIPCHK(hipMemcpyAsync(hs.data(), dser, (size_t)S * N * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(hp.data(), dload + 3 * NJ, NJ * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(hf.data(), dfit, hf.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (load) HIPCHK(hipMemcpyAsync(load, dload, AT_NLOAD * NJ * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  if (series) std::memcpy(series, hs.data(), hs.size() * sizeof(double));
  if (fit) std::memcpy(fit, hf.data(), hf.size() * sizeof(double));
  double t = 0.0;
  for (size_t i = 0; i < (size_t)S * N; ++i) t += hs[i];
  int64_t np = 0;
  for (size_t i = 0; i < NJ; ++i) np += hp[i] >= 0.5 ? 1 : 0;
  double mx = 0.0, mn = std::nan(""); int64_t mn_at = -1;
  for (int j = 0; j < J; ++j) {
    const double c = hf[j], v = hf[2 * (size_t)J + j];
    if (v > mx) mx = v;
    if (!std::isnan(c) && (mn_at < 0 || c < mn)) { mn = c; mn_at = j; }
  }
  info->n_used = S; info->n_steps = n_steps; info->n_present = np; info->min_load = min_load; info->total = t / (double)S;
  info->max_rel_change = mx; info->min_cosine = mn; info->min_cosine_at = mn_at;
  return 0;
}

// Decomposition of the recorded signatures into a reference catalogue over the samples of r that used[] flags: the normalised catalogue
// once, k_map_colsum once, then per batch of samples k_dec_y (the flags and the renormalised columns, k-major), k_decompose (the two-stage
// refit: w_s[r,n], the fit values and nactive), attribution.h's k_attr_share and k_attr_stats with N := R, G := N, project.h's k_proj_fit
// with J := N (decompose.h); the info fields are sequential scans on the host.
static_assert(BNMF_DEC_NW == AT_NLOAD && BNMF_DEC_NFIT == DC_NFIT && BNMF_DEC_MAX_R == DC_MAX_R && DC_MAX_R <= 128, "decompose.h, attribution.h and bnmf.h disagree");
static constexpr size_t DEC_SCRATCH_CAP = (size_t)256 << 20;    // bytes of a batch's blocks of the scratch
static int decompose_impl(bnmf_handle* h, const char* fn, Range r, const int32_t* used, const double* ref, int R, const int32_t* keep, int n_steps,
                          double min_share, double* weight, double* fit, int32_t* nactive, int32_t* included, double* weights, bnmf_decompose_info* info) {
  if (int rc = range_enter(h, fn, h && info && ref, r)) return rc;
  const int K = h->cfg.K, N = h->cfg.N;
  std::vector<int> slots;
  if (int rc = range_slots(h, fn, r, used, true, slots)) return rc;
  if (keep) for (int n = 0; n < N; ++n) if (keep[n] != 0 && keep[n] != 1) return fail(BNMF_EINVAL, "%s: keep[%d] = %d is neither 0 nor 1", fn, n, (int)keep[n]);
  if (R < 1 || R > DC_MAX_R) return fail(BNMF_EINVAL, "%s: R = %d references, 1..BNMF_DEC_MAX_R = %d are possible", fn, R, DC_MAX_R);
  if (n_steps < 1 || n_steps > 100000) return fail(BNMF_EINVAL, "%s: n_steps = %d is not in 1..100000", fn, n_steps);
  if (!(min_share >= 0.0) || !(min_share < 1.0)) return fail(BNMF_EINVAL, "%s: min_share = %g is not a number in [0, 1)", fn, min_share);
  const int RS = proj_row_stride(R);
  std::vector<double> z((size_t)K * RS, 0.0);               // z[k][r] = ref[k,r] / rs[r], rs[r] = sum_k ref[k,r], k ascending from +0.0
  for (int j = 0; j < R; ++j)
    for (int k = 0; k < K; ++k) {
      const double v = ref[(size_t)k + (size_t)K * j];
      if (!(v >= 0.0) || std::isinf(v)) return fail(BNMF_EINVAL, "%s: reference_P[%d, %d] = %g is not a finite number >= 0", fn, k, j, v);
    }
  for (int j = 0; j < R; ++j) {
    double rs = 0.0;
    for (int k = 0; k < K; ++k) rs = rs + ref[(size_t)k + (size_t)K * j];
    if (!(rs > 0.0)) return fail(BNMF_EINVAL, "%s: column %d of reference_P is all zero: it has no share", fn, j);
    for (int k = 0; k < K; ++k) z[(size_t)k * RS + j] = ref[(size_t)k + (size_t)K * j] / rs;
  }
  const int S = (int)slots.size();
  if (S < 2) return fail(BNMF_ESIZE, "%s: %d used sample%s, the variance of the weights needs at least 2", fn, S, S == 1 ? "" : "s");
  if (!h->arr[BNMF_P].ring || !h->arr[BNMF_A].ring) return fail(BNMF_ESTATE, "%s: nothing recorded yet", fn);
  if (int rc = post_sync(h)) return rc;
  const size_t RN = (size_t)R * N, lenP = (size_t)K * N;
  const size_t per = ((weights ? 2 : 1) * RN + (size_t)(1 + DC_NFIT + K) * N) * sizeof(double) + (size_t)N * sizeof(int);   // scratch bytes of one sample
  long long want = (long long)std::max<size_t>(1, DEC_SCRATCH_CAP / per);
  if (const char* e = getenv("BNMF_DEC_BATCH")) { const long long v = atoll(e); if (v >= 1) want = v; }     // tests: the batch size
  const int Sb = (int)std::min<long long>({want, (long long)S, (long long)(INT_MAX / 2) / ((long long)K * N)});   // (K Sb N stays an int)
  // the catalogue through the caches at wave-uniform addresses: measured at the headline shape the staged catalogue beside
  // w and g in the LDS leaves one wave per CU where two fit without it and takes 1.8 times as long; with w and g in registers it is the
  // form bnmf_project measured faster.  Staged on request, while it fits 160 KB.
  const bool fits = proj_lds_bytes(K, R, true) <= LDS_CAP;
  bool stage = false;
  if (const char* e = getenv("BNMF_DEC_STAGE")) stage = fits && atoi(e) != 0;                               // tests, tools: the other form
  const size_t lds = proj_lds_bytes(K, R, stage);
  if (lds > LDS_CAP) return fail(BNMF_ESIZE, "%s: R = %d references need %zu bytes of LDS", fn, R, lds);    // (unreachable for R <= BNMF_DEC_MAX_R)
  double *cs, *dz, *dyt, *dscr, *dfs, *du, *dst, *dload, *dser, *dfst, *dfit, *dw; int *dslots, *dkeep, *dpart, *dnact;
  if (int rc = carve(h, [&](Carve& c) {
        cs = c.take<double>((size_t)S * N); dz = c.take<double>((size_t)K * RS); dyt = c.take<double>((size_t)K * Sb * N);
        dscr = c.take<double>((size_t)Sb * RN); dfs = c.take<double>((size_t)Sb * DC_NFIT * N); du = c.take<double>((size_t)Sb * N);
        dst = c.take<double>(AT_NLOAD * RN); dload = c.take<double>(AT_NLOAD * RN); dser = c.take<double>((size_t)S * R);
        dfst = c.take<double>((size_t)DC_NFIT * N); dfit = c.take<double>((size_t)DC_NFIT * N);
        dw = weights ? c.take<double>((size_t)Sb * RN) : nullptr;
        dslots = c.take<int>(S); dkeep = c.take<int>(N); dpart = c.take<int>((size_t)Sb * N); dnact = c.take<int>((size_t)S * N);
      })) return rc;
  std::vector<int> hkeep(N, 1);
  if (keep) for (int n = 0; n < N; ++n) hkeep[n] = keep[n];
  HIPCHK(hipMemcpyAsync(dslots, slots.data(), (size_t)S * sizeof(int), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(dkeep, hkeep.data(), (size_t)N * sizeof(int), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(dz, z.data(), z.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
  const double* ringP = h->arr[BNMF_P].ring;
  hipLaunchKernelGGL(k_map_colsum, dim3(S, N), dim3(64), 0, h->stream, ringP, lenP, K, N, (const int*)dslots, cs);
  using DecKernel = decltype(&k_decompose<8, true>);
  const DecKernel staged[5] = {k_decompose<0, true>, k_decompose<8, true>, k_decompose<16, true>, k_decompose<24, true>, k_decompose<32, true>};
  const DecKernel direct[5] = {k_decompose<0, false>, k_decompose<8, false>, k_decompose<16, false>, k_decompose<24, false>, k_decompose<32, false>};
  const DecKernel kern = (stage ? staged : direct)[R <= PJ_MAX_NT ? RS / 8 : 0];
  if (int rc = opt_in_lds(kern, lds)) return rc;
  const int T = R <= PJ_MAX_NT ? PJ_T : PJ_TL;
  for (int s0 = 0; s0 < S; s0 += Sb) {
    const int nb = std::min(Sb, S - s0), first = s0 == 0 ? 1 : 0, last = s0 + nb == S ? 1 : 0, Pn = nb * N;
    hipLaunchKernelGGL(k_dec_y, dim3((unsigned)(((size_t)K * Pn + 255) / 256)), dim3(256), 0, h->stream, ringP, (const double*)h->arr[BNMF_A].ring, lenP, K, N,
                       Pn, (const int*)dslots + s0, (const double*)cs + (size_t)s0 * N, (const int*)dkeep, dyt, dpart);
    hipLaunchKernelGGL(kern, dim3((unsigned)((Pn + T - 1) / T)), dim3(T), lds, h->stream, (const double*)dz, (const double*)dyt, (const int*)dpart, K, R, N, Pn,
                       n_steps, min_share, dscr, dfs, dnact + (size_t)s0 * N);
    hipLaunchKernelGGL(k_attr_share, dim3((unsigned)((Pn + 255) / 256)), dim3(256), 0, h->stream, (const double*)dscr, nb, R, N, du);
    hipLaunchKernelGGL(k_attr_stats, dim3((unsigned)((size_t)nb * R + (RN + AT_TT - 1) / AT_TT)), dim3(AT_TT), 0, h->stream, (const double*)dscr,
                       (const double*)du, nb, R, N, S, s0, last, min_share, dst, dser, dload);
    hipLaunchKernelGGL(k_proj_fit, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, h->stream, (const double*)dfs, nb, N, S, first, last, dfst, dfit);
    HIPCHK(hipGetLastError());
    if (weights) {
      hipLaunchKernelGGL(k_proj_exposures, dim3((unsigned)(((size_t)nb * RN + 255) / 256)), dim3(256), 0, h->stream, (const double*)dscr, nb, R, N, dw);
      HIPCHK(hipGetLastError());
      HIPCHK(hipMemcpyAsync(weights + (size_t)s0 * RN, dw, (size_t)nb * RN * sizeof(double), hipMemcpyDeviceToHost, h->stream));
      HIPCHK(hipStreamSynchronize(h->stream));               // the next batch overwrites the scratch
    }
  }
  std::vector<double> hp(RN), hf((size_t)DC_NFIT * N);
  std::vector<int32_t> hn((size_t)S * N);
  HIPCHK(hipMemcpyAsync(hp.data(), dload + 3 * RN, RN * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(hf.data(), dfit, hf.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(hn.data(), dnact, hn.size() * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  if (weight) HIPCHK(hipMemcpyAsync(weight, dload, AT_NLOAD * RN * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  if (fit) std::memcpy(fit, hf.data(), hf.size() * sizeof(double));
  if (nactive) std::memcpy(nactive, hn.data(), hn.size() * sizeof(int32_t));
  if (included) for (int n = 0; n < N; ++n) { int32_t c = 0; for (int s = 0; s < S; ++s) c += hn[(size_t)s * N + n] > 0 ? 1 : 0; included[n] = c; }
  int64_t np = 0;
  for (size_t i = 0; i < RN; ++i) np += hp[i] >= 0.5 ? 1 : 0;
  double mx = 0.0, mn = std::nan(""); int64_t mn_at = -1;
  for (int n = 0; n < N; ++n) {
    const double c = hf[n], v = hf[2 * (size_t)N + n];
    if (v > mx) mx = v;
    if (!std::isnan(c) && (mn_at < 0 || c < mn)) { mn = c; mn_at = n; }
  }
  info->n_used = S; info->n_steps = n_steps; info->R = R; info->_pad = 0; info->n_present = np; info->min_share = min_share;
  info->max_rel_change = mx; info->min_cosine = mn; info->min_cosine_at = mn_at;
  return 0;
}

// ---- bnmf_contrast's host reduction; no device and no handle, so that a stand-alone host program can run it ----
// (con_canon64 and con_rows: reduce_host.h)
// ser [3][S][N*C] -> group [3][4][N*C], pair [3][6][N*NP] (each may be null), n_credible[3]
static void contrast_reduce(const double* ser, int S, int N, int C, double ci, double* group, double* pair, int64_t* n_credible) {
  const size_t NC = (size_t)N * C, NP = (size_t)C * (C - 1) / 2, NNP = (size_t)N * NP;
  std::vector<double> x(S), tmp(S);
  double prow[BNMF_CON_NPROW];
  for (int q = 0; q < BNMF_CON_NSTAT; ++q) {
    const double* v = ser + (size_t)q * S * NC;
    n_credible[q] = 0;
    if (group)
      for (size_t e = 0; e < NC; ++e) {
        for (int s = 0; s < S; ++s) x[s] = v[(size_t)s * NC + e];
        con_rows(x.data(), S, ci, tmp.data(), group + (size_t)q * BNMF_CON_NGROW * NC + e, NC);
      }
    size_t p = 0;
    for (int a = 0; a < C; ++a)
      for (int b = a + 1; b < C; ++b, ++p)
        for (int n = 0; n < N; ++n) {
          int gt = 0, lt = 0;
          for (int s = 0; s < S; ++s) {
            const double d = v[(size_t)s * NC + n + (size_t)N * a] - v[(size_t)s * NC + n + (size_t)N * b];
            x[s] = d; gt += d > 0.0 ? 1 : 0; lt += d < 0.0 ? 1 : 0;
          }
          con_rows(x.data(), S, ci, tmp.data(), prow, 1);
          prow[4] = (double)gt / (double)S; prow[5] = (double)lt / (double)S;
          if (prow[2] > 0.0 || prow[3] < 0.0) n_credible[q]++;
          if (pair) for (int i = 0; i < BNMF_CON_NPROW; ++i) pair[((size_t)q * BNMF_CON_NPROW + i) * NNP + n + (size_t)N * p] = prow[i];
        }
  }
}

// Group contrasts over the samples of r that used[] flags: k_map_colsum, then k_contrast (contrast.h) leaves the per-sample
// group values [3][S][N*C] in the scratch, a wave per (group, sample) over member lists built here; the statistics over the samples and
// the pairs are contrast_reduce's.
static_assert(CT_NSTAT == BNMF_CON_NSTAT, "contrast.h and bnmf.h disagree");
static int contrast_impl(bnmf_handle* h, const char* fn, Range r, const int32_t* used, const int32_t* groups, double min_load, double ci, double* group,
                         double* pair, double* series, int32_t* sizes, bnmf_contrast_info* info) {
  if (int rc = range_enter(h, fn, h && info && groups, r)) return rc;
  const int K = h->cfg.K, N = h->cfg.N, G = h->cfg.G;
  std::vector<int> slots;
  if (int rc = range_slots(h, fn, r, used, true, slots)) return rc;
  int C = 0, left = 0;
  for (int g = 0; g < G; ++g) {
    if (groups[g] < -1 || groups[g] >= BNMF_CON_MAX_GROUPS)
      return fail(BNMF_EINVAL, "%s: groups[%d] = %d is not a label in -1..%d", fn, g, (int)groups[g], BNMF_CON_MAX_GROUPS - 1);
    if (groups[g] < 0) ++left; else C = std::max(C, (int)groups[g] + 1);
  }
  std::vector<int> goff(C + 1, 0), members(G - left);
  for (int g = 0; g < G; ++g) if (groups[g] >= 0) goff[groups[g] + 1]++;
  for (int c = 0; c < C; ++c) if (!goff[c + 1]) return fail(BNMF_EINVAL, "%s: group %d has no member (the labels run to %d)", fn, c, C - 1);
  if (C == 0) return fail(BNMF_EINVAL, "%s: no tumour is in any group", fn);
  for (int c = 0; c < C; ++c) goff[c + 1] += goff[c];
  { std::vector<int> at(goff.begin(), goff.end() - 1); for (int g = 0; g < G; ++g) if (groups[g] >= 0) members[at[groups[g]]++] = g; }   // ascending inside a group
  if (!(min_load >= 0.0) || std::isinf(min_load)) return fail(BNMF_EINVAL, "%s: min_load = %g is not a finite number >= 0", fn, min_load);
  if (!(ci < 1.0)) return fail(BNMF_EINVAL, "%s: credible_interval = %g must be below 1", fn, ci);
  const int S = (int)slots.size();
  if (S < 2) return fail(BNMF_ESIZE, "%s: %d used sample%s, the variance over the samples needs at least 2", fn, S, S == 1 ? "" : "s");
  if (!h->arr[BNMF_P].ring || !h->arr[BNMF_E].ring || !h->arr[BNMF_A].ring) return fail(BNMF_ESTATE, "%s: nothing recorded yet", fn);
  if (int rc = post_sync(h)) return rc;
  const size_t NC = (size_t)N * C, nser = (size_t)CT_NSTAT * S * NC, lenP = (size_t)K * N;
  double *cs, *dser; int *dslots, *dmem, *doff;
  if (int rc = carve(h, [&](Carve& c) {
        cs = c.take<double>((size_t)S * N); dser = c.take<double>(nser); dslots = c.take<int>(S); dmem = c.take<int>(members.size()); doff = c.take<int>(C + 1);
      })) return rc;
  HIPCHK(hipMemcpyAsync(dslots, slots.data(), (size_t)S * sizeof(int), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(dmem, members.data(), members.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(doff, goff.data(), goff.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(k_map_colsum, dim3(S, N), dim3(64), 0, h->stream, (const double*)h->arr[BNMF_P].ring, lenP, K, N, (const int*)dslots, cs);
  ConArgs a{};
  a.ringE = h->arr[BNMF_E].ring; a.ringA = h->arr[BNMF_A].ring; a.cs = cs; a.slots = dslots; a.members = dmem; a.goff = doff; a.out = dser;
  a.lenE = (size_t)N * G; a.N = N; a.C = C; a.S = S; a.min_load = min_load;
  bool reg = N <= CT_MAX_REG;
  if (const char* e = getenv("BNMF_CON_FORM")) reg = reg && atoi(e) == 0;                                  // tests, tools: the tiled form
  using ConKernel = decltype(&k_contrast<8, true>);
  const ConKernel regs[4] = {k_contrast<8, true>, k_contrast<16, true>, k_contrast<24, true>, k_contrast<32, true>};
  for (int s0 = 0; s0 < S; s0 += 65535) {                                                                  // (the samples are the grid's y)
    const int nb = std::min(65535, S - s0);
    ConArgs b = a; b.cs = cs + (size_t)s0 * N; b.slots = dslots + s0; b.out = dser + (size_t)s0 * NC;
    if (reg) hipLaunchKernelGGL(regs[(N - 1) / 8], dim3(C, nb), dim3(64), 0, h->stream, b);
    else hipLaunchKernelGGL((k_contrast<CT_TN, false>), dim3(C, nb, (N + CT_TN - 1) / CT_TN), dim3(64), 0, h->stream, b);
  }
  HIPCHK(hipGetLastError());
  std::vector<double> hs(nser);
  HIPCHK(hipMemcpyAsync(hs.data(), dser, nser * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  if (series) std::memcpy(series, hs.data(), nser * sizeof(double));
  if (sizes) for (int c = 0; c < C; ++c) sizes[c] = goff[c + 1] - goff[c];
  std::memset(info, 0, sizeof *info);
  contrast_reduce(hs.data(), S, N, C, ci, group, C > 1 ? pair : nullptr, info->n_credible);
  info->n_used = S; info->n_groups = C; info->n_pairs = C * (C - 1) / 2; info->n_left_out = left; info->min_load = min_load; info->credible_interval = ci;
  return 0;
}

// ---- bnmf_regress's host parts; no device and no handle, so that a stand-alone host program can run them ----
// canonB: the blocked canonical sum of v[0 .. m): blocks of BNMF_REG_BLOCK, each con_canon64, added with b ascending from +0.0
static double reg_canonB(const double* v, size_t m) {
  double t = 0.0;
  for (size_t i0 = 0; i0 < m; i0 += BNMF_REG_BLOCK) t = t + con_canon64(v + i0, std::min((size_t)BNMF_REG_BLOCK, m - i0), 1);
  return t;
}
// D [m][Q] row-major in member order -> L [Q][Q] row-major, the Cholesky factor of the Gram matrix (the upper triangle 0).  Returns -1, or
// the first column j whose pivot d_j is not > 0 or not finite.  ratio = min_j d_j / Gm[j][j] and at = its j (the first wins a tie).
static int regress_factor(const double* D, size_t m, int Q, double* L, double& ratio, int& at) {
  std::vector<double> Gm((size_t)Q * Q), v(m);
  for (int j = 0; j < Q; ++j)
    for (int k = 0; k <= j; ++k) {
      for (size_t i = 0; i < m; ++i) v[i] = D[i * Q + j] * D[i * Q + k];
      Gm[(size_t)j * Q + k] = Gm[(size_t)k * Q + j] = reg_canonB(v.data(), m);
    }
  std::fill(L, L + (size_t)Q * Q, 0.0);
  at = -1;
  for (int j = 0; j < Q; ++j) {
    double d = Gm[(size_t)j * Q + j];
    for (int t = 0; t < j; ++t) d = d - L[j * Q + t] * L[j * Q + t];
    if (!(d > 0.0) || std::isinf(d)) return j;
    const double rj = d / Gm[(size_t)j * Q + j];
    if (at < 0 || rj < ratio) { ratio = rj; at = j; }
    L[j * Q + j] = std::sqrt(d);
    for (int i = j + 1; i < Q; ++i) {
      double w = Gm[(size_t)i * Q + j];
      for (int t = 0; t < j; ++t) w = w - L[i * Q + t] * L[j * Q + t];
      L[i * Q + j] = w / L[j * Q + j];
    }
  }
  return -1;
}
// cser [3][S][N*Q], r2 and s2 [3][S][N] -> coef [3][6][N*Q], fit [3][5][N] (each may be null), n_credible [3][BNMF_REG_MAX_Q].  Every
// (q, n, j) and (q, n) is a series of its own with its own sort: they are dealt to up to 16 threads (zplan.h's way); the counts are taken
// from the finished rows, so the result does not depend on the threads.
static void regress_reduce(const double* cser, const double* r2, const double* s2, int S, int N, int Q, double ci, double* coef, double* fit,
                           int64_t (*n_credible)[BNMF_REG_MAX_Q]) {
  const size_t NQ = (size_t)N * Q;
  const long ncoef = (long)(BNMF_REG_NSTAT * NQ), nfit = (long)BNMF_REG_NSTAT * N;
  std::vector<double> bounds(2 * (size_t)ncoef);            // lower, upper per (q, e): what n_credible counts, also without coef
  auto work = [&](long lo, long hi) {
    std::vector<double> x(S), tmp(S);
    double row[4];
    for (long i = lo; i < hi; ++i) {
      if (i < ncoef) {                                      // a coefficient's series
        const size_t q = (size_t)i / NQ, e = (size_t)i % NQ;
        const double* v = cser + q * S * NQ + e;
        int gt = 0, lt = 0;
        for (int s = 0; s < S; ++s) { const double b = v[(size_t)s * NQ]; x[s] = b; gt += b > 0.0 ? 1 : 0; lt += b < 0.0 ? 1 : 0; }
        con_rows(x.data(), S, ci, tmp.data(), row, 1);
        bounds[2 * i] = row[2]; bounds[2 * i + 1] = row[3];
        if (!coef) continue;
        double* o = coef + q * BNMF_REG_NCROW * NQ + e;
        for (int k = 0; k < 4; ++k) o[(size_t)k * NQ] = row[k];
        o[4 * NQ] = (double)gt / (double)S; o[5 * NQ] = (double)lt / (double)S;
      } else if (fit) {                                     // a factor's r2 and sigma2 series
        const size_t q = (size_t)(i - ncoef) / N, n = (size_t)(i - ncoef) % N;
        double* o = fit + q * BNMF_REG_NFIT * N + n;
        int nv = 0;
        for (int s = 0; s < S; ++s) { const double r = r2[(q * S + s) * N + n]; if (!std::isnan(r)) x[nv++] = r; }
        row[0] = row[2] = row[3] = std::nan("");
        if (nv) con_rows(x.data(), nv, ci, tmp.data(), row, 1);
        o[0] = row[0]; o[(size_t)N] = row[2]; o[2 * (size_t)N] = row[3]; o[3 * (size_t)N] = (double)nv;
        for (int s = 0; s < S; ++s) x[s] = s2[(q * S + s) * N + n];
        o[4 * (size_t)N] = con_canon64(x.data(), S, 1) / (double)S;
      }
    }
  };
  const long nwork = ncoef + nfit;
  deal_threads(nwork, work);
  for (int q = 0; q < BNMF_REG_NSTAT; ++q) {
    for (int j = 0; j < BNMF_REG_MAX_Q; ++j) n_credible[q][j] = 0;
    for (size_t e = 0; e < NQ; ++e) if (bounds[2 * (q * NQ + e)] > 0.0 || bounds[2 * (q * NQ + e) + 1] < 0.0) n_credible[q][e / N]++;
  }
}

// Regression of exposures on tumour covariates over the samples of r that used[] flags (regress.h): the member list, the
// design in member order and its Cholesky factor are made here; k_map_colsum, then k_regress_total, k_regress_moments, k_regress_solve,
// k_regress_resid and k_regress_fit leave the coefficients, r2 and sigma2 of every used sample in the scratch; the statistics over the samples are
// regress_reduce's.
static_assert(RG_BLOCK == BNMF_REG_BLOCK && RG_MAX_Q == BNMF_REG_MAX_Q && RG_NSTAT == BNMF_REG_NSTAT, "regress.h and bnmf.h disagree");
static int regress_impl(bnmf_handle* h, const char* fn, Range r, const int32_t* used, const double* design, int Q, const int32_t* include, double ci,
                        double* coef, double* fit, double* coef_series, double* r2_series, bnmf_regress_info* info) {
  if (int rc = range_enter(h, fn, h && info && design, r)) return rc;
  const int K = h->cfg.K, N = h->cfg.N, G = h->cfg.G;
  std::vector<int> slots;
  if (int rc = range_slots(h, fn, r, used, true, slots)) return rc;
  std::vector<int> members;
  for (int g = 0; g < G; ++g) {
    if (include && include[g] != 0 && include[g] != 1) return fail(BNMF_EINVAL, "%s: include[%d] = %d is neither 0 nor 1", fn, g, (int)include[g]);
    if (!include || include[g]) members.push_back(g);
  }
  const int m = (int)members.size();
  if (Q < 1 || Q > BNMF_REG_MAX_Q) return fail(BNMF_EINVAL, "%s: Q = %d design columns, 1..%d are possible", fn, Q, BNMF_REG_MAX_Q);
  std::vector<double> D((size_t)m * Q);                     // row-major in member order
  for (int i = 0; i < m; ++i)
    for (int j = 0; j < Q; ++j) {
      const double v = design[(size_t)members[i] + (size_t)G * j];
      if (std::isnan(v) || std::isinf(v)) return fail(BNMF_EINVAL, "%s: design[%d, %d] = %g of an included tumour is not finite", fn, members[i], j, v);
      D[(size_t)i * Q + j] = v;
    }
  if (!(ci < 1.0)) return fail(BNMF_EINVAL, "%s: credible_interval = %g must be below 1", fn, ci);
  const int S = (int)slots.size();
  if (S < 2) return fail(BNMF_ESIZE, "%s: %d used sample%s, the variance over the samples needs at least 2", fn, S, S == 1 ? "" : "s");
  if (m <= Q) return fail(BNMF_ESIZE, "%s: %d included tumour%s for Q = %d design columns, more than Q are needed", fn, m, m == 1 ? "" : "s", Q);
  std::vector<double> L((size_t)Q * Q);
  double ratio = 0.0; int ratio_at = -1;
  const int bad = regress_factor(D.data(), (size_t)m, Q, L.data(), ratio, ratio_at);
  if (bad >= 0) return fail(BNMF_EINVAL, "%s: design is not of full column rank (column %d is a combination of the columns before it)", fn, bad);
  if (!h->arr[BNMF_P].ring || !h->arr[BNMF_E].ring || !h->arr[BNMF_A].ring) return fail(BNMF_ESTATE, "%s: nothing recorded yet", fn);
  if (int rc = post_sync(h)) return rc;
  const int nb = (m + RG_BLOCK - 1) / RG_BLOCK;
  const size_t SN = (size_t)RG_NSTAT * S * N, NQ = (size_t)N * Q, lenP = (size_t)K * N;
  RegArgs a{};
  double* cs; int *dslots, *dmem; double *dD, *dL;
  if (int rc = carve(h, [&](Carve& c) {
        cs = c.take<double>((size_t)S * N); a.part = c.take<double>(SN * nb * (Q + 1)); a.part2 = c.take<double>(SN * nb * 2);
        a.coef = c.take<double>(SN * Q); a.ybar = c.take<double>(SN); a.r2 = c.take<double>(SN); a.sigma2 = c.take<double>(SN);
        a.u = c.take<double>((size_t)S * m);
        dD = c.take<double>(D.size()); dL = c.take<double>(L.size()); dslots = c.take<int>(S); dmem = c.take<int>(m);
      })) return rc;
  HIPCHK(hipMemcpyAsync(dslots, slots.data(), (size_t)S * sizeof(int), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(dmem, members.data(), (size_t)m * sizeof(int), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(dD, D.data(), D.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(dL, L.data(), L.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(k_map_colsum, dim3(S, N), dim3(64), 0, h->stream, (const double*)h->arr[BNMF_P].ring, lenP, K, N, (const int*)dslots, cs);
  a.ringE = h->arr[BNMF_E].ring; a.ringA = h->arr[BNMF_A].ring; a.cs = cs; a.slots = dslots; a.members = dmem; a.D = dD; a.L = dL;
  a.lenE = (size_t)N * G; a.N = N; a.Q = Q; a.S = S; a.m = m; a.nb = nb;
  int form = 0;
  if (const char* e = getenv("BNMF_REG_FORM")) form = atoi(e) != 0;                                        // tests, tools: the narrow tiles
  const int TN = form ? 2 : 4, TQ = form ? 2 : 4;
  const int ntn = (N + TN - 1) / TN, ntq = (Q + TQ - 1) / TQ; const unsigned nlane = (unsigned)((SN + 63) / 64);
  auto passes = [&](auto kern, unsigned units) {                                                           // (the samples are the grid's y)
    for (int s0 = 0; s0 < S; s0 += 65535) {
      RegArgs b = a; b.cs = cs + (size_t)s0 * N; b.slots = dslots + s0;
      b.part = a.part + (size_t)s0 * nb * RG_NSTAT * N * (Q + 1); b.part2 = a.part2 + (size_t)s0 * nb * RG_NSTAT * N * 2;
      b.coef = a.coef + (size_t)s0 * NQ; b.ybar = a.ybar + (size_t)s0 * N; b.u = a.u + (size_t)s0 * m;
      hipLaunchKernelGGL(kern, dim3(units, std::min(65535, S - s0)), dim3(64), 0, h->stream, b);
    }
  };
  passes(k_regress_total<RG_TC>, (unsigned)((m + 63) / 64));
  if (form) passes(k_regress_moments<2, 2>, reg_units(ntn * ntq, nb)); else passes(k_regress_moments<4, 4>, reg_units(ntn * ntq, nb));
  hipLaunchKernelGGL(k_regress_solve<RG_MAX_Q>, dim3(nlane), dim3(64), 0, h->stream, a);
  if (form) passes(k_regress_resid<2>, reg_units(ntn, nb)); else passes(k_regress_resid<4>, reg_units(ntn, nb));
  hipLaunchKernelGGL(k_regress_fit<RG_NSTAT>, dim3(nlane), dim3(64), 0, h->stream, a);
  HIPCHK(hipGetLastError());
  std::vector<double> hc(SN * Q), hr(SN), hs2(SN);
  HIPCHK(hipMemcpyAsync(hc.data(), a.coef, hc.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(hr.data(), a.r2, SN * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(hs2.data(), a.sigma2, SN * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  if (coef_series) std::memcpy(coef_series, hc.data(), hc.size() * sizeof(double));
  if (r2_series) std::memcpy(r2_series, hr.data(), SN * sizeof(double));
  std::memset(info, 0, sizeof *info);
  regress_reduce(hc.data(), hr.data(), hs2.data(), S, N, Q, ci, coef, fit, info->n_credible);
  info->n_used = S; info->Q = Q; info->n_included = m; info->n_left_out = G - m; info->n_blocks = nb; info->min_pivot_at = ratio_at;
  info->credible_interval = ci; info->min_pivot_ratio = ratio;
  return 0;
}

// Co-activity of signatures over the samples of r that used[] flags (coactivity.h): the member list is made here;
// k_map_colsum and k_coa_cosine run once over the range; then per batch of samples (their ranks are S N m int32: the batch keeps the
// scratch under COA_SCRATCH_CAP, as attr_impl's does) k_coa_mean, k_coa_mu, k_coa_pairs, the rank transform (k_coa_rank, or k_coa_sort +
// k_coa_search through sorted chunks), k_coa_rsum and k_coa_tail leave the four values of every pair in the series; the statistics over
// the samples are coactivity_reduce's.
static_assert(CO_NSTAT == BNMF_COA_NSTAT, "coactivity.h and bnmf.h disagree");
static constexpr size_t COA_SCRATCH_CAP = (size_t)256 << 20;    // bytes of ranks, sorted chunks and block partials per batch
static constexpr int COA_CHUNK = 16384, COA_WIDTH = 1024;       // doubles of a sorted chunk, threads of the sorting workgroup (measured)
static int coactivity_impl(bnmf_handle* h, const char* fn, Range r, const int32_t* used, const int32_t* include, double min_load, double ci,
                           double* pair, double* series, bnmf_coactivity_info* info) {
  if (int rc = range_enter(h, fn, h && info, r)) return rc;
  const int K = h->cfg.K, N = h->cfg.N, G = h->cfg.G;
  std::vector<int> slots;
  if (int rc = range_slots(h, fn, r, used, true, slots)) return rc;
  std::vector<int> members;
  for (int g = 0; g < G; ++g) {
    if (include && include[g] != 0 && include[g] != 1) return fail(BNMF_EINVAL, "%s: include[%d] = %d is neither 0 nor 1", fn, g, (int)include[g]);
    if (!include || include[g]) members.push_back(g);
  }
  const int m = (int)members.size();
  if (!(min_load >= 0.0) || std::isinf(min_load)) return fail(BNMF_EINVAL, "%s: min_load = %g is not a finite number >= 0", fn, min_load);
  if (!(ci < 1.0)) return fail(BNMF_EINVAL, "%s: credible_interval = %g must be below 1", fn, ci);
  if (N < 2) return fail(BNMF_ESIZE, "%s: N = %d factor%s, a pair needs at least 2", fn, N, N == 1 ? "" : "s");
  const int S = (int)slots.size();
  if (S < 2) return fail(BNMF_ESIZE, "%s: %d used sample%s, the variance over the samples needs at least 2", fn, S, S == 1 ? "" : "s");
  if (m < 3) return fail(BNMF_ESIZE, "%s: %d included tumour%s, a correlation needs at least 3", fn, m, m == 1 ? "" : "s");
  if (m > BNMF_COA_MAX_M) return fail(BNMF_ESIZE, "%s: %d included tumours, at most %d keep the rank sums inside int64", fn, m, BNMF_COA_MAX_M);
  if (!h->arr[BNMF_P].ring || !h->arr[BNMF_E].ring || !h->arr[BNMF_A].ring) return fail(BNMF_ESTATE, "%s: nothing recorded yet", fn);
  if (int rc = post_sync(h)) return rc;
  auto env_int = [](const char* name, long long dflt) { const char* e = getenv(name); const long long v = e ? atoll(e) : 0; return v >= 1 ? v : dflt; };
  int form = 0;
  if (const char* e = getenv("BNMF_COA_FORM")) form = atoi(e) != 0;                                        // tests, tools: narrow tiles, ranks through the scratch
  int chunk = CO_MIN_CHUNK;                                                                                // a power of two in 64 .. 16,384
  { const long long want = std::min<long long>(env_int("BNMF_COA_CHUNK", COA_CHUNK), CO_MAX_CHUNK); while ((long long)chunk * 2 <= want) chunk *= 2; }
  const int width = (int)env_int("BNMF_COA_WIDTH", COA_WIDTH);                                            // tools: 256, 512 or 1,024 threads
  const int nchunk = (m + chunk - 1) / chunk;
  const bool general = form || nchunk > 1;
  int n2 = CO_MIN_CHUNK;                                                                                   // keys of the one-chunk form
  while (n2 < m && n2 < chunk) n2 *= 2;
  const int nb = (m + RG_BLOCK - 1) / RG_BLOCK, NP = N * (N - 1) / 2;
  const size_t NN = (size_t)N * N, lenP = (size_t)K * N;
  const size_t per = (size_t)N * m * 4 + (general ? (size_t)N * nchunk * chunk * 8 : 0) + (size_t)nb * (N * 8 + NN * 12) + NN * 8 + (size_t)N * 12 + 6 * 256;
  const int Sb = (int)std::min<long long>({env_int("BNMF_COA_BATCH", (long long)std::max<size_t>(1, COA_SCRATCH_CAP / per)), (long long)S, 65535LL});
  CoaArgs a{};
  double* cs; int *dslots, *dmem;
  if (int rc = carve(h, [&](Carve& c) {
        cs = c.take<double>((size_t)S * N); a.ser = c.take<double>((size_t)CO_NSTAT * S * NP);
        a.partM = c.take<double>((size_t)Sb * nb * N); a.mu = c.take<double>((size_t)Sb * N); a.partS = c.take<double>((size_t)Sb * nb * NN);
        a.partC = c.take<int>((size_t)Sb * nb * NN); a.c = c.take<int>((size_t)Sb * N * m);
        a.sorted = general ? c.take<double>((size_t)Sb * N * nchunk * chunk) : nullptr;
        a.flag = c.take<int>((size_t)Sb * N); a.T = c.take<long long>((size_t)Sb * NN);
        dslots = c.take<int>(S); dmem = c.take<int>(m);
      })) return rc;
  HIPCHK(hipMemcpyAsync(dslots, slots.data(), (size_t)S * sizeof(int), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(dmem, members.data(), (size_t)m * sizeof(int), hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(k_map_colsum, dim3(S, N), dim3(64), 0, h->stream, (const double*)h->arr[BNMF_P].ring, lenP, K, N, (const int*)dslots, cs);
  a.ringE = h->arr[BNMF_E].ring; a.ringA = h->arr[BNMF_A].ring; a.ringP = h->arr[BNMF_P].ring; a.cs = cs; a.slots = dslots; a.members = dmem;
  a.lenE = (size_t)N * G; a.lenP = lenP; a.N = N; a.K = K; a.S = S; a.m = m; a.nb = nb; a.chunk = chunk; a.nchunk = nchunk; a.min_load = min_load;
  const int T = form ? 2 : 4, nt = (N + T - 1) / T, ntp = nt * (nt + 1) / 2;
  const size_t lds = (size_t)(general ? chunk : n2) * sizeof(double);
  using RankKernel = decltype(&k_coa_rank<1024>);
  using SortKernel = decltype(&k_coa_sort<1024>);
  const int wi = width <= 256 ? 0 : width <= 512 ? 1 : 2, wt = 256 << wi;
  const RankKernel krank[3] = {k_coa_rank<256>, k_coa_rank<512>, k_coa_rank<1024>};
  const SortKernel ksort[3] = {k_coa_sort<256>, k_coa_sort<512>, k_coa_sort<1024>};
  if (int rc = general ? opt_in_lds(ksort[wi], lds, lds) : opt_in_lds(krank[wi], lds, lds)) return rc;   // (the workgroup vote keeps a static word of its own: ask for the keys only)
  for (int s0 = 0; s0 < S; s0 += Sb) {
    const int ns = std::min(Sb, S - s0);
    a.s0 = s0;
    hipLaunchKernelGGL(k_coa_cosine<CO_NSTAT>, dim3((unsigned)((NP + 63) / 64), ns), dim3(64), 0, h->stream, a);
    if (form) hipLaunchKernelGGL(k_coa_mean<2>, dim3(reg_units(nt, nb), ns), dim3(64), 0, h->stream, a);
    else hipLaunchKernelGGL(k_coa_mean<4>, dim3(reg_units(nt, nb), ns), dim3(64), 0, h->stream, a);
    hipLaunchKernelGGL(k_coa_mu<CO_NSTAT>, dim3((unsigned)(((size_t)ns * N + 63) / 64)), dim3(64), 0, h->stream, a, ns);
    if (form) hipLaunchKernelGGL(k_coa_pairs<2>, dim3(reg_units(ntp, nb), ns), dim3(64), 0, h->stream, a);
    else hipLaunchKernelGGL(k_coa_pairs<4>, dim3(reg_units(ntp, nb), ns), dim3(64), 0, h->stream, a);
    if (!general) hipLaunchKernelGGL(krank[wi], dim3(N, ns), dim3(wt), lds, h->stream, a, n2);
    else {
      HIPCHK(hipMemsetAsync(a.flag, 0, (size_t)ns * N * sizeof(int), h->stream));
      hipLaunchKernelGGL(ksort[wi], dim3((unsigned)N * nchunk, ns), dim3(wt), lds, h->stream, a);
      hipLaunchKernelGGL(k_coa_search<256>, dim3((unsigned)((m + 255) / 256), N, ns), dim3(256), 0, h->stream, a);
    }
    if (form) hipLaunchKernelGGL(k_coa_rsum<2>, dim3(ntp, ns), dim3(64), 0, h->stream, a);
    else hipLaunchKernelGGL(k_coa_rsum<4>, dim3(ntp, ns), dim3(64), 0, h->stream, a);
    hipLaunchKernelGGL(k_coa_tail<CO_NSTAT>, dim3((unsigned)(((size_t)ns * NP + 63) / 64)), dim3(64), 0, h->stream, a, ns);
    HIPCHK(hipGetLastError());
  }
  const size_t nser = (size_t)CO_NSTAT * S * NP;
  std::vector<double> hs(nser);
  HIPCHK(hipMemcpyAsync(hs.data(), a.ser, nser * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  if (series) std::memcpy(series, hs.data(), nser * sizeof(double));
  std::memset(info, 0, sizeof *info);
  coactivity_reduce(hs.data(), S, NP, ci, pair, info->n_credible, &info->max_cosine_at, &info->max_cosine);
  info->n_used = S; info->n_included = m; info->n_left_out = G - m; info->n_pairs = NP; info->n_blocks = nb; info->min_load = min_load;
  info->credible_interval = ci;
  return 0;
}

// Silhouette stability of the recorded signatures over the samples of r that used[] flags (stability.h): k_stab_norm leaves
// the squared norm of every ring point, from which the members and the packed order (cluster by cluster, member-list order) are made here;
// k_stab_gather packs the columns, k_stab_pairs leaves the block partials of D, the blocks are added in order here and everything from D
// on is stability_reduce's.
static_assert(BNMF_REG_BLOCK == RG_BLOCK, "regress.h and bnmf.h disagree");
static int stability_impl(bnmf_handle* h, const char* fn, Range r, const int32_t* used, const int32_t* labels, const double* extra_P,
                          const int32_t* extra_label, int X, double* point, double* factor, double* between, double* medoid, int64_t* medoid_at,
                          bnmf_stability_info* info) {
  if (int rc = range_enter(h, fn, h && info, r)) return rc;
  const int K = h->cfg.K, N = h->cfg.N;
  std::vector<int> slots;
  if (int rc = range_slots(h, fn, r, used, true, slots)) return rc;
  const int S = (int)slots.size();
  std::vector<int> rows;                                                     // the row of the range of used sample s
  for (int s = 0; s < r.n; ++s) if (!used || used[s]) rows.push_back(s);
  if (labels)
    for (int s : rows) for (int n = 0; n < N; ++n) {
      const int v = labels[(size_t)s * N + n];
      if (v < -1 || v >= N) return fail(BNMF_EINVAL, "%s: labels[%d][%d] = %d is outside -1 .. %d (sample %d of the range, factor %d)", fn, s, n, v, N - 1, s, n);
    }
  if (X < 0) return fail(BNMF_EINVAL, "%s: X = %d extra columns", fn, X);
  if (X > 0 && (!extra_P || !extra_label)) return fail(BNMF_EINVAL, "%s: X = %d extra columns but extra_P or extra_label is null", fn, X);
  for (int x = 0; x < X; ++x) {
    if (extra_label[x] < 0 || extra_label[x] >= N) return fail(BNMF_EINVAL, "%s: extra_label[%d] = %d is outside 0 .. %d", fn, x, (int)extra_label[x], N - 1);
    bool any = false;
    for (int k = 0; k < K; ++k) {
      const double v = extra_P[(size_t)K * x + k];
      if (!std::isfinite(v)) return fail(BNMF_EINVAL, "%s: extra_P[%d, %d] = %g is not finite", fn, k, x, v);
      any = any || v != 0.0;
    }
    if (!any) return fail(BNMF_EINVAL, "%s: extra column %d is all zero", fn, x);
  }
  if (N < 2) return fail(BNMF_ESIZE, "%s: N = %d factor%s, a silhouette needs at least 2 clusters", fn, N, N == 1 ? "" : "s");
  if (S < 2) return fail(BNMF_ESIZE, "%s: %d used sample%s, a cluster of draws needs at least 2", fn, S, S == 1 ? "" : "s");
  if (!h->arr[BNMF_P].ring || !h->arr[BNMF_A].ring) return fail(BNMF_ESTATE, "%s: nothing recorded yet", fn);
  if (int rc = post_sync(h)) return rc;
  const long SN = (long)S * N, NPT = SN + X;
  StabArgs a{};
  a.ringP = h->arr[BNMF_P].ring; a.ringA = h->arr[BNMF_A].ring; a.lenP = (size_t)K * N; a.N = N; a.K = K; a.S = S;
  int* dslots;
  if (int rc = carve(h, [&](Carve& c) { a.ok = c.take<int>((size_t)SN); dslots = c.take<int>(S); })) return rc;
  HIPCHK(hipMemcpyAsync(dslots, slots.data(), (size_t)S * sizeof(int), hipMemcpyHostToDevice, h->stream));
  a.slots = dslots;
  // (k_stab_norm and k_stab_gather use no template parameter: they are templates only for their place in the code object)
  hipLaunchKernelGGL(k_stab_norm<BNMF_STAB_NPOINT>, dim3((unsigned)((SN + 63) / 64)), dim3(64), 0, h->stream, a);
  HIPCHK(hipGetLastError());
  std::vector<int> ok((size_t)SN);
  HIPCHK(hipMemcpyAsync(ok.data(), a.ok, (size_t)SN * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  // the member lists: ring members by ascending index, then the extras by ascending x
  std::vector<int32_t> off(N + 1, 0);
  std::vector<int> lab((size_t)NPT, -1);
  for (int s = 0; s < S; ++s) for (int n = 0; n < N; ++n) {
    const int j = labels ? labels[(size_t)rows[s] * N + n] : n;
    if (j != -1 && ok[(size_t)s * N + n]) { lab[(size_t)s * N + n] = j; ++off[j + 1]; }
  }
  for (int x = 0; x < X; ++x) { lab[(size_t)SN + x] = extra_label[x]; ++off[extra_label[x] + 1]; }
  for (int j = 0; j < N; ++j) off[j + 1] += off[j];
  const long M = off[N];
  if (M < 2) return fail(BNMF_ESIZE, "%s: %ld member%s in all, a silhouette needs at least 2", fn, M, M == 1 ? "" : "s");
  if (M > BNMF_STAB_MAX_POINTS) return fail(BNMF_ESIZE, "%s: %ld members, at most %d are taken", fn, M, BNMF_STAB_MAX_POINTS);
  const int Mp = (int)((M + ST_ROWS - 1) / ST_ROWS) * ST_ROWS;
  std::vector<int> src(Mp, -1), fill(off.begin(), off.end() - 1), ustart, uend, ucl;
  std::vector<int64_t> pt((size_t)M);
  for (long i = 0; i < NPT; ++i) if (lab[i] >= 0) { const int q = fill[lab[i]]++; src[q] = (int)i; pt[q] = i; }
  for (int j = 0; j < N; ++j)
    for (int q = off[j]; q < off[j + 1]; q += RG_BLOCK) { ustart.push_back(q); uend.push_back(std::min<int>(q + RG_BLOCK, off[j + 1])); ucl.push_back(j); }
  const int U = (int)ustart.size();
  double* dextra; int *dsrc, *dus, *due;
  if (int rc = carve(h, [&](Carve& c) {
        dslots = c.take<int>(S); dextra = c.take<double>((size_t)K * std::max(X, 1)); dsrc = c.take<int>(Mp); dus = c.take<int>(U); due = c.take<int>(U);
        a.packed = c.take<double>((size_t)K * Mp); a.nn = c.take<double>(Mp); a.part = c.take<double>((size_t)M * U);
      })) return rc;
  HIPCHK(hipMemcpyAsync(dslots, slots.data(), (size_t)S * sizeof(int), hipMemcpyHostToDevice, h->stream));
  if (X > 0) HIPCHK(hipMemcpyAsync(dextra, extra_P, (size_t)K * X * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(dsrc, src.data(), (size_t)Mp * sizeof(int), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(dus, ustart.data(), (size_t)U * sizeof(int), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(due, uend.data(), (size_t)U * sizeof(int), hipMemcpyHostToDevice, h->stream));
  a.slots = dslots; a.extra = dextra; a.src = dsrc; a.ustart = dus; a.uend = due; a.ok = nullptr; a.M = (int)M; a.Mp = Mp; a.U = U;
  hipLaunchKernelGGL(k_stab_gather<BNMF_STAB_NPOINT>, dim3((unsigned)((Mp + 63) / 64)), dim3(64), 0, h->stream, a);
  const int per = ST_ROWS * ST_WAVES;
  hipLaunchKernelGGL(k_stab_pairs<ST_ROWS>, dim3((unsigned)U, (unsigned)((M + per - 1) / per)), dim3(64 * ST_WAVES), 0, h->stream, a);
  HIPCHK(hipGetLastError());
  std::vector<double> part((size_t)M * U), D((size_t)M * N, 0.0);
  HIPCHK(hipMemcpyAsync(part.data(), a.part, part.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  for (long q = 0; q < M; ++q) for (int u = 0; u < U; ++u) D[(size_t)q * N + ucl[u]] = D[(size_t)q * N + ucl[u]] + part[(size_t)q * U + u];   // the blocks in order from +0.0
  std::memset(info, 0, sizeof *info);
  std::vector<int64_t> mpos(N);
  stability_reduce(D.data(), M, N, off.data(), pt.data(), NPT, point, factor, between, medoid_at, mpos.data(), info);
  info->n_used = S; info->n_extra = X; info->n_left_out = (int32_t)(NPT - M);
  if (medoid) {
    std::vector<double> col(K);
    for (int j = 0; j < N; ++j) {
      if (mpos[j] < 0) { for (int k = 0; k < K; ++k) medoid[(size_t)K * j + k] = std::nan(""); continue; }
      HIPCHK(hipMemcpy2D(col.data(), sizeof(double), a.packed + mpos[j], (size_t)Mp * sizeof(double), sizeof(double), (size_t)K, hipMemcpyDeviceToHost));
      stability_medoid(col.data(), 1, K, medoid + (size_t)K * j);
    }
  }
  return 0;
}

// Reconstruction quality per tumour over the samples of r that used[] flags (reconstruction.h): k_rec_data once (the data
// k-major as doubles, mm and t per tumour), then per batch of samples k_rec_x (the rows P_s diag(A_s)), k_rec (a lane per (s, g): the
// per-sample values in the scratch) and k_rec_stats (the statistics continued in sample order, the series); the series' division, the
// signature rows and the info fields are reconstruction_reduce's.
static_assert(RC_NTUM == BNMF_REC_NTUM && RC_NDROP == BNMF_REC_NDROP, "reconstruction.h and bnmf.h disagree");
static constexpr size_t REC_SCRATCH_CAP = (size_t)256 << 20;    // bytes of a batch's blocks of the scratch
static int reconstruction_impl(bnmf_handle* h, const char* fn, Range r, const int32_t* used, double min_cosine, double min_drop, double* tumour,
                               double* drop, double* series, double* signature, bnmf_reconstruction_info* info) {
  if (int rc = range_enter(h, fn, h && info, r)) return rc;
  const int K = h->cfg.K, N = h->cfg.N, G = h->cfg.G;
  if (!std::isfinite(min_cosine)) return fail(BNMF_EINVAL, "%s: min_cosine = %g is not a finite number", fn, min_cosine);
  if (!std::isfinite(min_drop)) return fail(BNMF_EINVAL, "%s: min_drop = %g is not a finite number", fn, min_drop);
  std::vector<int> slots;
  if (int rc = range_slots(h, fn, r, used, true, slots)) return rc;
  const int S = (int)slots.size();
  if (S < 2) return fail(BNMF_ESIZE, "%s: %d used sample%s, the variance of the cosines needs at least 2", fn, S, S == 1 ? "" : "s");
  if (!h->arr[BNMF_P].ring || !h->arr[BNMF_E].ring || !h->arr[BNMF_A].ring) return fail(BNMF_ESTATE, "%s: nothing recorded yet", fn);
  if (int rc = post_sync(h)) return rc;
  bool reg = N <= RC_MAX_NT;
  if (const char* e = getenv("BNMF_REC_FORM")) if (atoi(e) == 1) reg = false;                              // tests, tools: the tiled form
  const int NS = reg ? rec_row_stride(N) : N;
  const size_t NG = (size_t)N * G, KNS = (size_t)K * NS, rows = (size_t)(N + 3) * G;
  const size_t per = (rows + KNS) * sizeof(double);                                                        // scratch bytes of one sample
  long long want = (long long)std::max<size_t>(1, REC_SCRATCH_CAP / per);
  if (const char* e = getenv("BNMF_REC_BATCH")) { const long long v = atoll(e); if (v >= 1) want = v; }   // tests: the batch size
  const int Sb = (int)std::min<long long>({want, (long long)S, 65535LL});                                  // (a batch is the grid's y)
  // x staged in the LDS while it fits: measured faster than the wave-uniform reads through the caches in the register form too
  // (DESIGN.md 23), unlike bnmf_project's refit
  const bool fits = rec_lds_bytes(K, NS) <= LDS_CAP;
  bool stage = fits;
  if (const char* e = getenv("BNMF_REC_STAGE")) stage = fits && atoi(e) != 0;                              // tests, tools: the other choice
  const size_t lds = stage ? rec_lds_bytes(K, NS) : 0;
  double *dMt, *dmm, *dtt, *dxg, *dscr, *dst, *dsd, *dser, *dtum, *ddrop; int* dslots;
  if (int rc = carve(h, [&](Carve& c) {
        dMt = c.take<double>((size_t)K * G); dmm = c.take<double>(G); dtt = c.take<double>(G); dxg = c.take<double>((size_t)Sb * KNS);
        dscr = c.take<double>((size_t)Sb * rows); dst = c.take<double>((size_t)RC_NTUM * G); dsd = c.take<double>(RC_NDROP * NG);
        dser = c.take<double>(S); dtum = c.take<double>((size_t)RC_NTUM * G); ddrop = c.take<double>(RC_NDROP * NG); dslots = c.take<int>(S);
      })) return rc;
  HIPCHK(hipMemcpyAsync(dslots, slots.data(), (size_t)S * sizeof(int), hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(k_rec_data<RC_NTUM>, dim3((unsigned)((G + 255) / 256)), dim3(256), 0, h->stream, (const int32_t*)h->dM, (const double*)h->dMf, K, G, dMt, dmm, dtt);
  using RecKernel = decltype(&k_rec<8, true>);
  const RecKernel staged[5] = {k_rec<0, true>, k_rec<8, true>, k_rec<16, true>, k_rec<24, true>, k_rec<32, true>};
  const RecKernel direct[5] = {k_rec<0, false>, k_rec<8, false>, k_rec<16, false>, k_rec<24, false>, k_rec<32, false>};
  const RecKernel kern = (stage ? staged : direct)[reg ? NS / 8 : 0];
  if (int rc = opt_in_lds(kern, lds)) return rc;
  const double *ringP = h->arr[BNMF_P].ring, *ringE = h->arr[BNMF_E].ring, *ringA = h->arr[BNMF_A].ring;
  for (int s0 = 0; s0 < S; s0 += Sb) {
    const int nb = std::min(Sb, S - s0), last = s0 + nb == S ? 1 : 0;
    hipLaunchKernelGGL(k_rec_x<RC_NTUM>, dim3(nb), dim3(256), 0, h->stream, ringP, ringA, (size_t)K * N, K, N, NS, (const int*)dslots + s0, dxg);
    hipLaunchKernelGGL(kern, dim3((unsigned)((G + RC_T - 1) / RC_T), (unsigned)nb), dim3(RC_T), lds, h->stream, (const double*)dxg, ringE, NG,
                       (const int*)dslots + s0, (const double*)dMt, (const double*)dmm, (const double*)dtt, K, N, G, dscr);
    hipLaunchKernelGGL(k_rec_stats<RC_NTUM>, dim3((unsigned)((size_t)nb + (NG + (size_t)G + RC_TT - 1) / RC_TT)), dim3(RC_TT), 0, h->stream, (const double*)dscr, ringA,
                       (const int*)dslots + s0, (const double*)dmm, nb, N, G, S, s0, last, min_cosine, min_drop, dst, dsd, dser, dtum, ddrop);
    HIPCHK(hipGetLastError());
  }
  std::vector<double> ht, hd, hs(S), hm(G);                      // the info fields need the rows whether or not the caller wants them
  if (!tumour) { ht.resize((size_t)RC_NTUM * G); tumour = ht.data(); }
  if (!drop) { hd.resize(RC_NDROP * NG); drop = hd.data(); }
  HIPCHK(hipMemcpyAsync(tumour, dtum, (size_t)RC_NTUM * G * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(drop, ddrop, RC_NDROP * NG * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(hs.data(), dser, hs.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(hm.data(), dmm, hm.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  std::memset(info, 0, sizeof *info);
  reconstruction_reduce(tumour, drop, hm.data(), hs.data(), S, N, G, min_cosine, signature, info);
  info->n_used = S; info->min_cosine = min_cosine; info->min_drop = min_drop;
  if (series) std::memcpy(series, hs.data(), hs.size() * sizeof(double));
  return 0;
}

// Similarity of tumours over the samples of r that used[] flags (similarity.h): the member list and the row list are made
// here; k_map_colsum and k_sim_norm run once over the range; then per band of rows k_sim_pairs leaves mean, variance and p_similar of
// every (row, member) in the scratch, k_sim_select takes the row's neighbours, typicality and degree, and the rows that are queries are
// copied out.  The row list is the member list, or, when only dense is asked for, the queries alone.  The outputs by tumour and the info
// fields are similarity_finish's.
static_assert(SM_NROW == BNMF_SIM_NNROW && SM_NROW == BNMF_SIM_NDROW && SM_NROW == BNMF_SIM_NTUM && SM_MAX_K == BNMF_SIM_MAX_K, "similarity.h and bnmf.h disagree");
static constexpr size_t SIM_SCRATCH_CAP = (size_t)256 << 20;    // bytes of the call's scratch: the norms and a band's results
static int similarity_impl(bnmf_handle* h, const char* fn, Range r, const int32_t* used, const int32_t* include, const int32_t* query, int Q, int top_k,
                           double min_cosine, int32_t* neighbour_at, double* neighbour, double* dense, double* tumour, bnmf_similarity_info* info) {
  if (int rc = range_enter(h, fn, h && info, r)) return rc;
  const int K = h->cfg.K, N = h->cfg.N, G = h->cfg.G;
  std::vector<int> slots;
  if (int rc = range_slots(h, fn, r, used, true, slots)) return rc;
  std::vector<int> members, place(G, -1);                  // place[g]: g's position in the member list
  for (int g = 0; g < G; ++g) {
    if (include && include[g] != 0 && include[g] != 1) return fail(BNMF_EINVAL, "%s: include[%d] = %d is neither 0 nor 1", fn, g, (int)include[g]);
    if (!include || include[g]) { place[g] = (int)members.size(); members.push_back(g); }
  }
  const int m = (int)members.size();
  if (Q < 0) return fail(BNMF_EINVAL, "%s: Q = %d is negative", fn, Q);
  if (Q > 0 && !query) return fail(BNMF_EINVAL, "%s: Q = %d but query is null", fn, Q);
  for (int q = 0; q < Q; ++q) {
    if (query[q] < 0 || query[q] >= G) return fail(BNMF_EINVAL, "%s: query[%d] = %d is outside 0..%d", fn, q, (int)query[q], G - 1);
    if (place[query[q]] < 0) return fail(BNMF_EINVAL, "%s: query[%d] = %d is a tumour that include[] leaves out", fn, q, (int)query[q]);
  }
  if (top_k < 0 || top_k > BNMF_SIM_MAX_K) return fail(BNMF_EINVAL, "%s: top_k = %d is outside 0..%d", fn, top_k, BNMF_SIM_MAX_K);
  if (!std::isfinite(min_cosine)) return fail(BNMF_EINVAL, "%s: min_cosine = %g is not a finite number", fn, min_cosine);
  const int S = (int)slots.size();
  if (S < 2) return fail(BNMF_ESIZE, "%s: %d used sample%s, the variance of the cosines needs at least 2", fn, S, S == 1 ? "" : "s");
  if (m < 2) return fail(BNMF_ESIZE, "%s: %d included tumour%s, a pair needs 2", fn, m, m == 1 ? "" : "s");
  if (!h->arr[BNMF_P].ring || !h->arr[BNMF_E].ring || !h->arr[BNMF_A].ring) return fail(BNMF_ESTATE, "%s: nothing recorded yet", fn);
  if (int rc = post_sync(h)) return rc;
  const bool all = !(top_k == 0 && !tumour && Q > 0);       // the pass over all pairs
  std::vector<int> rows(all ? m : Q);
  for (size_t i = 0; i < rows.size(); ++i) rows[i] = all ? (int)i : place[query[i]];
  const int nrows = (int)rows.size(), k = top_k;
  const size_t fixed = ((size_t)S * N + (size_t)S * m) * sizeof(double), per = (size_t)SM_NROW * m * sizeof(double);   // the norms; a row of a band
  long long want = (long long)std::max<size_t>(1, (SIM_SCRATCH_CAP > fixed ? SIM_SCRATCH_CAP - fixed : 0) / per);
  if (want > SM_TILE) want -= want % SM_TILE;              // whole tiles of rows
  if (const char* e = getenv("BNMF_SIM_BAND")) { const long long v = atoll(e); if (v >= 1) want = v; }    // tests, tools: the rows of a band
  const int B = (int)std::min<long long>(want, nrows);
  SimArgs a{};
  double *cs, *dnn, *dres, *dnb = nullptr, *dtum = nullptr; int *dslots, *dmem, *drows; int32_t* dnat = nullptr;
  if (int rc = carve(h, [&](Carve& c) {
        cs = c.take<double>((size_t)S * N); dnn = c.take<double>((size_t)S * m); dres = c.take<double>((size_t)SM_NROW * B * m);
        if (all) { dnat = c.take<int32_t>((size_t)m * k); dnb = c.take<double>((size_t)SM_NROW * m * k); dtum = c.take<double>((size_t)SM_NROW * m); }
        dslots = c.take<int>(S); dmem = c.take<int>(m); drows = c.take<int>(nrows);
      })) return rc;
  HIPCHK(hipMemcpyAsync(dslots, slots.data(), (size_t)S * sizeof(int), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(dmem, members.data(), (size_t)m * sizeof(int), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(drows, rows.data(), (size_t)nrows * sizeof(int), hipMemcpyHostToDevice, h->stream));
  const double *ringE = h->arr[BNMF_E].ring, *ringA = h->arr[BNMF_A].ring;
  const size_t lenE = (size_t)N * G;
  hipLaunchKernelGGL(k_map_colsum, dim3(S, N), dim3(64), 0, h->stream, (const double*)h->arr[BNMF_P].ring, (size_t)K * N, K, N, (const int*)dslots, cs);
  hipLaunchKernelGGL(k_sim_norm<SM_NROW>, dim3((unsigned)(((size_t)S * m + 255) / 256)), dim3(256), 0, h->stream, ringE, ringA, (const double*)cs,
                     (const int*)dslots, (const int*)dmem, lenE, N, S, m, dnn);
  a.ringE = ringE; a.ringA = ringA; a.cs = cs; a.nn = dnn; a.slots = dslots; a.members = dmem; a.res = dres; a.lenE = lenE; a.N = N; a.S = S; a.m = m;
  a.min_cosine = min_cosine;
  // the queries' rows in member order, [3][Q][m]: row r of a band is copied out where it is a query's
  std::vector<double> hq(dense ? (size_t)SM_NROW * Q * m : 0);
  for (int r0 = 0; r0 < nrows; r0 += B) {
    const int nr = std::min(B, nrows - r0);
    a.rows = drows + r0; a.nr = nr;
    hipLaunchKernelGGL(k_sim_pairs<SM_NROW>, dim3((unsigned)((m + SM_TILE - 1) / SM_TILE), (unsigned)((nr + SM_TILE - 1) / SM_TILE)), dim3(SM_T), 0, h->stream, a);
    if (all) hipLaunchKernelGGL(k_sim_select<SM_NROW>, dim3(nr), dim3(64), 0, h->stream, (const double*)dres, (const int*)(drows + r0), m, nr, r0, k, dnat, dnb,
                                (size_t)m * k, dtum, (size_t)m);
    HIPCHK(hipGetLastError());
    if (dense)
      for (int q = 0; q < Q; ++q) {
        const int lr = (all ? place[query[q]] : q) - r0;    // the query's row of this band
        if (lr < 0 || lr >= nr) continue;
        for (int t = 0; t < SM_NROW; ++t)
          HIPCHK(hipMemcpyAsync(hq.data() + ((size_t)t * Q + q) * m, dres + ((size_t)t * nr + lr) * m, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, h->stream));
      }
  }
  std::vector<int32_t> hnat(all ? (size_t)m * k : 0);
  std::vector<double> hnb(all ? (size_t)SM_NROW * m * k : 0), htum(all ? (size_t)SM_NROW * m : 0);
  if (all) {
    if (!hnat.empty()) HIPCHK(hipMemcpyAsync(hnat.data(), dnat, hnat.size() * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    if (!hnb.empty()) HIPCHK(hipMemcpyAsync(hnb.data(), dnb, hnb.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(htum.data(), dtum, htum.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  }
  HIPCHK(hipStreamSynchronize(h->stream));
  std::memset(info, 0, sizeof *info);
  similarity_finish(members.data(), m, G, k, all ? hnat.data() : nullptr, all ? hnb.data() : nullptr, all ? htum.data() : nullptr, neighbour_at, neighbour,
                    tumour, info);
  info->n_used = S; info->top_k = top_k; info->n_query = Q; info->min_cosine = min_cosine;
  if (dense) {
    std::fill(dense, dense + (size_t)SM_NROW * Q * G, std::nan(""));
    for (int t = 0; t < SM_NROW; ++t)
      for (int q = 0; q < Q; ++q) {
        const double* src = hq.data() + ((size_t)t * Q + q) * m;
        double* dst = dense + ((size_t)t * Q + q) * G;
        for (int i = 0; i < m; ++i) if (members[i] != query[q]) dst[members[i]] = src[i];
      }
  }
  return 0;
}

// Subtypes of tumours over the samples of r that used[] flags (subtypes.h): the member list, the matched samples and
// their perm rows are made here; k_map_colsum runs once over the matched samples; then per batch of samples k_subtypes runs every
// sample's Lloyd steps with the labels in the scratch, k_sub_count adds the batch to the whole-number counts and, if asked for, the
// batch's labels are copied out.  The outputs by tumour, the moments of the centres and sizes and the info fields are subtypes_finish's.
static_assert(SB_NTUM == BNMF_SUB_NTUM && SB_NCROW == BNMF_SUB_NCROW && SB_NSER == BNMF_SUB_NSER && SB_MAX_C == BNMF_SUB_MAX_C && SB_MAX_N == BNMF_SUB_MAX_N,
              "subtypes.h and bnmf.h disagree");
static constexpr size_t SUB_SCRATCH_CAP = (size_t)256 << 20;    // bytes of a batch's labels, dmin and u
static int subtypes_impl(bnmf_handle* h, const char* fn, Range r, const int32_t* used, const int32_t* include, const int32_t* perm, const double* centres0,
                         int C, int n_steps, const int32_t* query, int Q, double min_certainty, double* membership, int32_t* label, double* tumour,
                         double* centre, double* size, double* together, int32_t* labels, double* series, bnmf_subtypes_info* info) {
  if (int rc = range_enter(h, fn, h && info && centres0, r)) return rc;
  const int K = h->cfg.K, N = h->cfg.N, G = h->cfg.G;
  std::vector<int> slots;
  if (int rc = range_slots(h, fn, r, used, true, slots)) return rc;
  std::vector<int> members, place(G, -1);                  // place[g]: g's position in the member list
  for (int g = 0; g < G; ++g) {
    if (include && include[g] != 0 && include[g] != 1) return fail(BNMF_EINVAL, "%s: include[%d] = %d is neither 0 nor 1", fn, g, (int)include[g]);
    if (!include || include[g]) { place[g] = (int)members.size(); members.push_back(g); }
  }
  const int m = (int)members.size();
  if (C < 2 || C > BNMF_SUB_MAX_C) return fail(BNMF_EINVAL, "%s: C = %d is outside 2..%d", fn, C, BNMF_SUB_MAX_C);
  if (n_steps < 1 || n_steps > BNMF_SUB_MAX_STEPS) return fail(BNMF_EINVAL, "%s: n_steps = %d is outside 1..%d", fn, n_steps, BNMF_SUB_MAX_STEPS);
  if (Q < 0) return fail(BNMF_EINVAL, "%s: Q = %d is negative", fn, Q);
  if (Q > 0 && !query) return fail(BNMF_EINVAL, "%s: Q = %d but query is null", fn, Q);
  for (int q = 0; q < Q; ++q) {
    if (query[q] < 0 || query[q] >= G) return fail(BNMF_EINVAL, "%s: query[%d] = %d is outside 0..%d", fn, q, (int)query[q], G - 1);
    if (place[query[q]] < 0) return fail(BNMF_EINVAL, "%s: query[%d] = %d is a tumour that include[] leaves out", fn, q, (int)query[q]);
  }
  for (int c = 0; c < C; ++c) for (int j = 0; j < N; ++j) {
    const double v = centres0[j + (size_t)N * c];
    if (!std::isfinite(v) || v < 0.0) return fail(BNMF_EINVAL, "%s: centres0[%d, %d] = %g is not a finite number >= 0", fn, j, c, v);
  }
  if (!(min_certainty >= 0.0 && min_certainty <= 1.0)) return fail(BNMF_EINVAL, "%s: min_certainty = %g is outside [0, 1]", fn, min_certainty);
  // the matched samples: rows[] is the row of the range of every used sample, mrow[] the used sample of every matched one
  std::vector<int> rows, mrow, mslots, hperm;
  for (int s = 0; s < r.n; ++s) if (!used || used[s]) rows.push_back(s);
  const int S = (int)slots.size();
  for (int s = 0; s < S; ++s) {
    const int32_t* pr = perm ? perm + (size_t)rows[s] * N : nullptr;
    bool none = pr != nullptr;
    for (int n = 0; pr && n < N; ++n) none = none && pr[n] == -1;
    if (none) continue;
    if (pr) {
      std::vector<char> seen(N, 0);
      for (int n = 0; n < N; ++n) {
        if (pr[n] < 0 || pr[n] >= N || seen[pr[n]])
          return fail(BNMF_EINVAL, "%s: perm[%d] is neither a permutation of 0..%d nor -1 throughout (sample %d of the range, factor %d: %d)", fn, rows[s], N - 1,
                      rows[s], n, (int)pr[n]);
        seen[pr[n]] = 1;
      }
    }
    mrow.push_back(s); mslots.push_back(slots[s]);
    for (int n = 0; n < N; ++n) hperm.push_back(pr ? pr[n] : n);
  }
  const int Sm = (int)mrow.size();
  if (S < 2) return fail(BNMF_ESIZE, "%s: %d used sample%s, the variance over the samples needs at least 2", fn, S, S == 1 ? "" : "s");
  if (Sm < 2) return fail(BNMF_ESIZE, "%s: %d matched sample%s of %d used, the variance over the samples needs at least 2", fn, Sm, Sm == 1 ? "" : "s", S);
  if (m < C) return fail(BNMF_ESIZE, "%s: %d included tumour%s for C = %d subtypes", fn, m, m == 1 ? "" : "s", C);
  if (N > BNMF_SUB_MAX_N) return fail(BNMF_ESIZE, "%s: N = %d factors, at most %d are taken", fn, N, BNMF_SUB_MAX_N);
  if (!h->arr[BNMF_P].ring || !h->arr[BNMF_E].ring || !h->arr[BNMF_A].ring) return fail(BNMF_ESTATE, "%s: nothing recorded yet", fn);
  if (int rc = post_sync(h)) return rc;
  bool small = N <= 8 && C <= 4;
  if (const char* e = getenv("BNMF_SUB_FORM")) if (atoi(e) == 1) small = false;                            // tests, tools: the tiled form
  const size_t per = (size_t)m * (sizeof(int32_t) + 2 * sizeof(double));                                   // scratch bytes of one sample
  long long want = (long long)std::max<size_t>(1, SUB_SCRATCH_CAP / per);
  if (const char* e = getenv("BNMF_SUB_BATCH")) { const long long v = atoll(e); if (v >= 1) want = v; }   // tests: the batch size
  const int Sb = (int)std::min<long long>(want, Sm);
  const size_t NC = (size_t)N * C;
  std::vector<int> qplace(std::max(Q, 1), 0);
  for (int q = 0; q < Q; ++q) qplace[q] = place[query[q]];
  SubArgs a{};
  double *cs, *dc0; int *dslots, *dmem, *dperm, *dqp; int32_t *dcnt, *dasg, *dtog, *dboth;
  if (int rc = carve(h, [&](Carve& c) {
        cs = c.take<double>((size_t)Sm * N); dc0 = c.take<double>(NC); a.centre = c.take<double>((size_t)Sm * NC); a.size = c.take<int32_t>((size_t)Sm * C);
        a.inertia = c.take<double>(Sm); a.steps = c.take<int32_t>(Sm); a.assigned = c.take<int32_t>(Sm); a.changed = c.take<int32_t>(Sm);
        a.lab = c.take<int32_t>((size_t)Sb * m); a.dmin = c.take<double>((size_t)Sb * m); a.u = c.take<double>((size_t)Sb * m);
        dcnt = c.take<int32_t>((size_t)(C + 1 + 2 * Q) * m);                                               // cnt [C][m], assigned [m], together [Q][m], both [Q][m]
        dslots = c.take<int>(Sm); dmem = c.take<int>(m); dperm = c.take<int>((size_t)Sm * N); dqp = c.take<int>(std::max(Q, 1));
      })) return rc;
  dasg = dcnt + (size_t)C * m; dtog = dasg + m; dboth = dtog + (size_t)Q * m;
  HIPCHK(hipMemcpyAsync(dslots, mslots.data(), (size_t)Sm * sizeof(int), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(dmem, members.data(), (size_t)m * sizeof(int), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(dperm, hperm.data(), (size_t)Sm * N * sizeof(int), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(dqp, qplace.data(), (size_t)std::max(Q, 1) * sizeof(int), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(dc0, centres0, NC * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemsetAsync(dcnt, 0, (size_t)(C + 1 + 2 * Q) * m * sizeof(int32_t), h->stream));
  hipLaunchKernelGGL(k_map_colsum, dim3(Sm, N), dim3(64), 0, h->stream, (const double*)h->arr[BNMF_P].ring, (size_t)K * N, K, N, (const int*)dslots, cs);
  a.ringE = h->arr[BNMF_E].ring; a.ringA = h->arr[BNMF_A].ring; a.cs = cs; a.slots = dslots; a.members = dmem; a.perm = dperm; a.centres0 = dc0;
  a.lenE = (size_t)N * G; a.N = N; a.C = C; a.m = m; a.n_steps = n_steps;
  std::vector<int32_t> hlab(labels ? (size_t)Sb * m : 0);
  if (labels) std::fill(labels, labels + (size_t)S * G, (int32_t)-2);
  for (int s0 = 0; s0 < Sm; s0 += Sb) {
    const int ns = std::min(Sb, Sm - s0);
    a.s0 = s0;
    if (small) hipLaunchKernelGGL((k_subtypes<8, 4>), dim3(ns), dim3(SB_T), 0, h->stream, a);
    else hipLaunchKernelGGL((k_subtypes<4, 8>), dim3(ns), dim3(SB_T), 0, h->stream, a);
    for (int q0 = 0; q0 == 0 || q0 < Q; q0 += SB_QSLICE) {       // the queries in slices: the grid's y is 16 bits wide
      const int nq = std::min(SB_QSLICE, Q - q0);
      hipLaunchKernelGGL(k_sub_count<SB_NTUM>, dim3((unsigned)((m + 255) / 256), (unsigned)(1 + nq)), dim3(256), 0, h->stream, (const int32_t*)a.lab, ns, m, C,
                         (const int*)dqp + q0, dcnt, dasg, dtog + (size_t)q0 * m, dboth + (size_t)q0 * m, q0 == 0 ? 1 : 0);
    }
    HIPCHK(hipGetLastError());
    if (labels) {                                             // the batch's labels leave the device before the next batch overwrites them
      HIPCHK(hipMemcpyAsync(hlab.data(), a.lab, (size_t)ns * m * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
      HIPCHK(hipStreamSynchronize(h->stream));
      for (int s = 0; s < ns; ++s) {
        int32_t* dst = labels + (size_t)mrow[s0 + s] * G;
        for (int i = 0; i < m; ++i) dst[members[i]] = hlab[(size_t)s * m + i];
      }
    }
  }
  std::vector<int32_t> hcnt((size_t)(C + 1 + 2 * Q) * m), hsize((size_t)Sm * C), hsteps(Sm), hasg(Sm), hchg(Sm);
  std::vector<double> hcen((size_t)Sm * NC), hin(Sm);
  HIPCHK(hipMemcpyAsync(hcnt.data(), dcnt, hcnt.size() * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(hsize.data(), a.size, hsize.size() * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(hsteps.data(), a.steps, (size_t)Sm * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(hasg.data(), a.assigned, (size_t)Sm * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(hchg.data(), a.changed, (size_t)Sm * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(hcen.data(), a.centre, hcen.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(hin.data(), a.inertia, (size_t)Sm * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  std::memset(info, 0, sizeof *info);
  const int32_t* pc = hcnt.data();
  subtypes_finish(members.data(), m, G, N, C, Sm, pc, pc + (size_t)C * m, Q, query, pc + (size_t)(C + 1) * m, pc + (size_t)(C + 1 + Q) * m, hcen.data(),
                  hsize.data(), min_certainty, membership, label, tumour, centre, size, together, info);
  info->n_used = S; info->n_matched = Sm; info->n_unmatched = S - Sm; info->C = C; info->n_steps = n_steps; info->n_query = Q; info->min_certainty = min_certainty;
  for (int s = 0; s < Sm; ++s) info->n_not_converged += (hsteps[s] == n_steps && hchg[s]) ? 1 : 0;
  if (series) {
    std::fill(series, series + (size_t)SB_NSER * S, std::nan(""));
    for (int s = 0; s < Sm; ++s) {
      series[mrow[s]] = hin[s]; series[(size_t)S + mrow[s]] = (double)hsteps[s]; series[2 * (size_t)S + mrow[s]] = (double)hasg[s];
    }
  }
  return 0;
}

// Residual structure over the samples of r that used[] flags (residuals.h): the member list is made here; k_rec_data leaves
// the data k-major once; then per batch of samples k_rec_x, k_res_z (z and chi in the scratch), k_res_b, k_res_gram (C_s), k_res_power
// (the component, the series, flat), k_res_score and k_res_accum (the accumulators of the mean matrix), and the batch's scores and chi
// are copied out.  k_res_mean ends the mean matrix; its component, the alignment, the moments and the info fields are residuals_finish's.
static_assert(RS_NTYPE == BNMF_RES_NTYPE && RS_NCOMP == BNMF_RES_NCOMP && RS_NTUM == BNMF_RES_NTUM && RS_NSER == BNMF_RES_NSER && RS_MAX_K == BNMF_RES_MAX_K,
              "residuals.h and bnmf.h disagree");
static constexpr size_t RES_SCRATCH_CAP = (size_t)256 << 20;    // bytes of a batch's z, C_s, scores, chi and x
static int residuals_impl(bnmf_handle* h, const char* fn, Range r, const int32_t* used, const int32_t* include, int n_steps, double max_dispersion, double* gram,
                          double* type, double* component, double* tumour, double* series, bnmf_residuals_info* info) {
  if (int rc = range_enter(h, fn, h && info, r)) return rc;
  const int K = h->cfg.K, N = h->cfg.N, G = h->cfg.G;
  const bool normal = h->cfg.likelihood == BNMF_NORMAL;
  std::vector<int> slots;
  if (int rc = range_slots(h, fn, r, used, true, slots)) return rc;
  std::vector<int> members;
  for (int g = 0; g < G; ++g) {
    if (include && include[g] != 0 && include[g] != 1) return fail(BNMF_EINVAL, "%s: include[%d] = %d is neither 0 nor 1", fn, g, (int)include[g]);
    if (!include || include[g]) members.push_back(g);
  }
  const int m = (int)members.size(), S = (int)slots.size();
  if (n_steps < 1 || n_steps > BNMF_RES_MAX_STEPS) return fail(BNMF_EINVAL, "%s: n_steps = %d is outside 1..%d", fn, n_steps, BNMF_RES_MAX_STEPS);
  if (!(max_dispersion >= 0.0)) return fail(BNMF_EINVAL, "%s: max_dispersion = %g is NaN or negative", fn, max_dispersion);
  if (S < 2) return fail(BNMF_ESIZE, "%s: %d used sample%s, the variance over the samples needs at least 2", fn, S, S == 1 ? "" : "s");
  if (m < 2) return fail(BNMF_ESIZE, "%s: %d included tumour%s, at least 2 are needed", fn, m, m == 1 ? "" : "s");
  if (K > BNMF_RES_MAX_K) return fail(BNMF_ESIZE, "%s: K = %d mutation types, at most %d are taken", fn, K, BNMF_RES_MAX_K);
  if (!h->arr[BNMF_P].ring || !h->arr[BNMF_E].ring || !h->arr[BNMF_A].ring || (normal && !h->arr[BNMF_SIGMASQ].ring))
    return fail(BNMF_ESTATE, "%s: nothing recorded yet", fn);
  if (int rc = post_sync(h)) return rc;
  int form = 0;
  if (const char* e = getenv("BNMF_RES_FORM")) if (atoi(e) == 1) form = 1;                                // tests, tools: the small tile, any N
  const bool reg = form == 0 && N <= RS_MAX_NT;
  const int NS = reg ? ((N + 7) / 8) * 8 : N;
  const size_t KK = (size_t)K * K, Km = (size_t)K * m, KNS = (size_t)K * NS;
  const size_t per = (Km + KK + 2 * (size_t)m + KNS) * sizeof(double);                                     // scratch bytes of one sample
  long long want = (long long)std::max<size_t>(1, RES_SCRATCH_CAP / per);
  if (const char* e = getenv("BNMF_RES_BATCH")) { const long long v = atoll(e); if (v >= 1) want = v; }   // tests: the batch size
  const int Sb = (int)std::min<long long>({want, (long long)S, 65535LL});                                  // (a batch is the grid's y)
  ResArgs a{};
  double *dMt, *dmm, *dtt, *dxg, *dacc, *dgram; int *dslots, *dmem;
  if (int rc = carve(h, [&](Carve& c) {
        dMt = c.take<double>((size_t)K * G); dmm = c.take<double>(G); dtt = c.take<double>(G); dxg = c.take<double>((size_t)Sb * KNS);
        a.z = c.take<double>((size_t)Sb * Km); a.chi = c.take<double>((size_t)Sb * m); a.t = c.take<double>((size_t)Sb * m); a.C = c.take<double>((size_t)Sb * KK);
        a.b = c.take<double>((size_t)S * K); a.q = c.take<double>((size_t)S * K); a.v = c.take<double>((size_t)S * K); a.ser = c.take<double>(4 * (size_t)S);
        a.flat = c.take<int>(S); dacc = c.take<double>(64 * KK); dgram = c.take<double>(KK); dslots = c.take<int>(S); dmem = c.take<int>(m);
      })) return rc;
  HIPCHK(hipMemcpyAsync(dslots, slots.data(), (size_t)S * sizeof(int), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(dmem, members.data(), (size_t)m * sizeof(int), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemsetAsync(dacc, 0, 64 * KK * sizeof(double), h->stream));
  hipLaunchKernelGGL(k_rec_data<RC_NTUM>, dim3((unsigned)((G + 255) / 256)), dim3(256), 0, h->stream, (const int32_t*)h->dM, (const double*)h->dMf, K, G, dMt, dmm, dtt);
  a.ringE = h->arr[BNMF_E].ring; a.ringS = normal ? h->arr[BNMF_SIGMASQ].ring : nullptr; a.xg = dxg; a.Mt = dMt; a.slots = dslots; a.members = dmem;
  a.lenE = (size_t)N * G; a.K = K; a.N = N; a.NS = NS; a.G = G; a.m = m; a.S = S; a.n_steps = n_steps;
  using ZKernel = decltype(&k_res_z<false, 0>);
  const ZKernel zp[5] = {k_res_z<false, 0>, k_res_z<false, 8>, k_res_z<false, 16>, k_res_z<false, 24>, k_res_z<false, 32>};
  const ZKernel zn[5] = {k_res_z<true, 0>, k_res_z<true, 8>, k_res_z<true, 16>, k_res_z<true, 24>, k_res_z<true, 32>};
  const ZKernel kz = (normal ? zn : zp)[reg ? NS / 8 : 0];
  const int T = form == 0 ? 8 : 4, nt = (K + T - 1) / T;
  const unsigned ntp = (unsigned)((size_t)nt * (nt + 1) / 2), gm = (unsigned)((m + RS_T - 1) / RS_T), gk = (unsigned)((KK + 255) / 256);
  const double *ringP = h->arr[BNMF_P].ring, *ringA = h->arr[BNMF_A].ring;
  std::vector<double> ht((size_t)S * m), hchi((size_t)S * m);
  for (int s0 = 0; s0 < S; s0 += Sb) {
    const int nb = std::min(Sb, S - s0);
    a.s0 = s0;
    hipLaunchKernelGGL(k_rec_x<RC_NTUM>, dim3(nb), dim3(256), 0, h->stream, ringP, ringA, (size_t)K * N, K, N, NS, (const int*)dslots + s0, dxg);
    hipLaunchKernelGGL(kz, dim3(gm, (unsigned)nb), dim3(RS_T), 0, h->stream, a);
    hipLaunchKernelGGL(k_res_b<RS_NTYPE>, dim3((unsigned)K, (unsigned)nb), dim3(64), 0, h->stream, a);
    if (form == 0) hipLaunchKernelGGL(k_res_gram<8>, dim3(ntp, (unsigned)nb), dim3(64), 0, h->stream, a);
    else hipLaunchKernelGGL(k_res_gram<4>, dim3(ntp, (unsigned)nb), dim3(64), 0, h->stream, a);
    hipLaunchKernelGGL(k_res_power<RS_NTYPE>, dim3((unsigned)nb), dim3(RS_T), 2 * (size_t)K * sizeof(double), h->stream, a);
    hipLaunchKernelGGL(k_res_score<RS_NTYPE>, dim3(gm, (unsigned)nb), dim3(RS_T), 0, h->stream, a);
    hipLaunchKernelGGL(k_res_accum<RS_NTYPE>, dim3(gk), dim3(256), 0, h->stream, (const double*)a.C, (const int*)a.flat, s0, nb, KK, dacc);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(ht.data() + (size_t)s0 * m, a.t, (size_t)nb * m * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(hchi.data() + (size_t)s0 * m, a.chi, (size_t)nb * m * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  }
  hipLaunchKernelGGL(k_res_mean<RS_NTYPE>, dim3(gk), dim3(256), 0, h->stream, (const int*)a.flat, S, KK, dacc, dgram);
  HIPCHK(hipGetLastError());
  std::vector<double> hb((size_t)S * K), hq((size_t)S * K), hv((size_t)S * K), hser(4 * (size_t)S), hg(KK);
  std::vector<int32_t> hflat(S);
  HIPCHK(hipMemcpyAsync(hb.data(), a.b, hb.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(hq.data(), a.q, hq.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(hv.data(), a.v, hv.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(hser.data(), a.ser, hser.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(hflat.data(), a.flat, (size_t)S * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(hg.data(), dgram, KK * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  int Sp = 0;
  for (int s = 0; s < S; ++s) Sp += hflat[s] ? 0 : 1;
  if (Sp < 2) return fail(BNMF_ESIZE, "%s: %d sample%s of %d used that %s not flat, the variance over the samples needs at least 2", fn, Sp, Sp == 1 ? "" : "s", S,
                          Sp == 1 ? "is" : "are");
  std::memset(info, 0, sizeof *info);
  residuals_finish(members.data(), m, G, K, S, n_steps, max_dispersion, hflat.data(), hg.data(), hser.data(), hb.data(), hq.data(), hv.data(), ht.data(),
                   hchi.data(), type, component, tumour, series, info);
  info->n_used = S; info->n_steps = n_steps; info->max_dispersion = max_dispersion;
  if (gram) std::memcpy(gram, hg.data(), KK * sizeof(double));
  return 0;
}

// Trade-offs between signatures within a tumour over the samples of r that used[] flags (tradeoff.h): the member list, the
// matched samples and their perm rows are made here; k_map_colsum runs once over the matched samples, k_trd_prep turns them into tables by
// aligned place and k_trd_mean leaves every member's means.  Then per band of members, whose N x N covariances fit TRD_SCRATCH_CAP:
// k_trd_comoment, k_trd_finish, k_trd_pair and k_trd_dense.  The divisions of the pair rows and the info fields are tradeoff_finish's.
static_assert(TD_NTUM == BNMF_TRD_NTUM && TD_NPAIR == BNMF_TRD_NPAIR && TD_NSET == BNMF_TRD_NSET && TD_MAX_C == BNMF_TRD_MAX_C && TD_MAX_N == BNMF_TRD_MAX_N,
              "tradeoff.h and bnmf.h disagree");
static constexpr size_t TRD_SCRATCH_CAP = (size_t)256 << 20;    // bytes of a band's covariances
static int tradeoff_impl(bnmf_handle* h, const char* fn, Range r, const int32_t* used, const int32_t* include, const int32_t* perm, const int32_t* sets, int C,
                         const int32_t* query, int Q, double min_corr, double* tumour, int32_t* pair_at, double* pair, double* dense, double* setstat,
                         bnmf_tradeoff_info* info) {
  if (int rc = range_enter(h, fn, h && info, r)) return rc;
  const int K = h->cfg.K, N = h->cfg.N, G = h->cfg.G;
  std::vector<int> slots;
  if (int rc = range_slots(h, fn, r, used, true, slots)) return rc;
  std::vector<int> members, place(G, -1);                  // place[g]: g's position in the member list
  for (int g = 0; g < G; ++g) {
    if (include && include[g] != 0 && include[g] != 1) return fail(BNMF_EINVAL, "%s: include[%d] = %d is neither 0 nor 1", fn, g, (int)include[g]);
    if (!include || include[g]) { place[g] = (int)members.size(); members.push_back(g); }
  }
  const int m = (int)members.size();
  if (C < 0 || C > BNMF_TRD_MAX_C) return fail(BNMF_EINVAL, "%s: C = %d is outside 0..%d", fn, C, BNMF_TRD_MAX_C);
  if (C > 0 && !sets) return fail(BNMF_EINVAL, "%s: C = %d but sets is null", fn, C);
  if (C > 0) {
    std::vector<int> size(C, 0);
    for (int n = 0; n < N; ++n) {
      if (sets[n] < -1 || sets[n] >= C) return fail(BNMF_EINVAL, "%s: sets[%d] = %d is outside -1..%d", fn, n, (int)sets[n], C - 1);
      if (sets[n] >= 0) ++size[sets[n]];
    }
    for (int c = 0; c < C; ++c) if (!size[c]) return fail(BNMF_EINVAL, "%s: set %d is empty", fn, c);
  }
  if (Q < 0) return fail(BNMF_EINVAL, "%s: Q = %d is negative", fn, Q);
  if (Q > 0 && !query) return fail(BNMF_EINVAL, "%s: Q = %d but query is null", fn, Q);
  for (int q = 0; q < Q; ++q) {
    if (query[q] < 0 || query[q] >= G) return fail(BNMF_EINVAL, "%s: query[%d] = %d is outside 0..%d", fn, q, (int)query[q], G - 1);
    if (place[query[q]] < 0) return fail(BNMF_EINVAL, "%s: query[%d] = %d is a tumour that include[] leaves out", fn, q, (int)query[q]);
  }
  if (!(min_corr >= 0.0 && min_corr <= 1.0)) return fail(BNMF_EINVAL, "%s: min_corr = %g is outside [0, 1]", fn, min_corr);
  // the matched samples: rows[] is the row of the range of every used sample
  std::vector<int> rows, mslots, hperm;
  for (int s = 0; s < r.n; ++s) if (!used || used[s]) rows.push_back(s);
  const int S = (int)slots.size();
  for (int s = 0; s < S; ++s) {
    const int32_t* pr = perm ? perm + (size_t)rows[s] * N : nullptr;
    bool none = pr != nullptr;
    for (int n = 0; pr && n < N; ++n) none = none && pr[n] == -1;
    if (none) continue;
    if (pr) {
      std::vector<char> seen(N, 0);
      for (int n = 0; n < N; ++n) {
        if (pr[n] < 0 || pr[n] >= N || seen[pr[n]])
          return fail(BNMF_EINVAL, "%s: perm[%d] is neither a permutation of 0..%d nor -1 throughout (sample %d of the range, factor %d: %d)", fn, rows[s], N - 1,
                      rows[s], n, (int)pr[n]);
        seen[pr[n]] = 1;
      }
    }
    mslots.push_back(slots[s]);
    for (int n = 0; n < N; ++n) hperm.push_back(pr ? pr[n] : n);
  }
  const int Sm = (int)mslots.size();
  if (S < 2) return fail(BNMF_ESIZE, "%s: %d used sample%s, the covariance over the samples needs at least 2", fn, S, S == 1 ? "" : "s");
  if (Sm < 2) return fail(BNMF_ESIZE, "%s: %d matched sample%s of %d used, the covariance over the samples needs at least 2", fn, Sm, Sm == 1 ? "" : "s", S);
  if (m < 1) return fail(BNMF_ESIZE, "%s: no included tumour", fn);
  if (N > BNMF_TRD_MAX_N) return fail(BNMF_ESIZE, "%s: N = %d factors, at most %d are taken", fn, N, BNMF_TRD_MAX_N);
  if (!h->arr[BNMF_P].ring || !h->arr[BNMF_E].ring || !h->arr[BNMF_A].ring) return fail(BNMF_ESTATE, "%s: nothing recorded yet", fn);
  if (int rc = post_sync(h)) return rc;
  int TL = 16;
  if (const char* e = getenv("BNMF_TRD_FORM")) if (atoi(e) == 1) TL = 8;                                   // tests, tools: the tile of 8
  const size_t NN = (size_t)N * N;
  long long want = (long long)std::max<size_t>(1, TRD_SCRATCH_CAP / (NN * sizeof(double)));
  if (want < m && want >= RG_BLOCK) want -= want % RG_BLOCK;                                              // whole blocks of canonB: no accumulator crosses a band
  if (const char* e = getenv("BNMF_TRD_BAND")) { const long long v = atoll(e); if (v >= 1) want = v; }   // tests: the members of a band
  const int mb = (int)std::min<long long>(want, m);
  const bool crosses = mb < m && mb % RG_BLOCK != 0;                                                      // a band ends inside a block of canonB
  std::vector<int> qplace(std::max(Q, 1), 0);
  for (int q = 0; q < Q; ++q) qplace[q] = place[query[q]];
  TrdArgs a{};
  double *cs, *df, *dtum, *dsst, *drun, *dcarry, *ddense; long long* doff; int *don, *dslots, *dmem, *dperm, *dqp, *dsets; int32_t *dpat, *dcnt;
  if (int rc = carve(h, [&](Carve& c) {
        cs = c.take<double>((size_t)Sm * N); df = c.take<double>((size_t)Sm * N); doff = c.take<long long>((size_t)Sm * N); don = c.take<int>((size_t)Sm * N);
        a.mu = c.take<double>((size_t)m * N); a.cov = c.take<double>(NN * mb); dtum = c.take<double>((size_t)TD_NTUM * m); dpat = c.take<int32_t>(m);
        dsst = c.take<double>((size_t)TD_NSET * std::max(C, 1) * m); drun = c.take<double>(NN * 2); dcnt = c.take<int32_t>(NN * 3);
        dcarry = c.take<double>(crosses ? NN * 2 * 64 : 1); ddense = c.take<double>((size_t)std::max(Q, 1) * 2 * NN);
        dslots = c.take<int>(Sm); dmem = c.take<int>(m); dperm = c.take<int>((size_t)Sm * N); dqp = c.take<int>(std::max(Q, 1)); dsets = c.take<int>(N);
      })) return rc;
  HIPCHK(hipMemcpyAsync(dslots, mslots.data(), (size_t)Sm * sizeof(int), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(dmem, members.data(), (size_t)m * sizeof(int), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(dperm, hperm.data(), (size_t)Sm * N * sizeof(int), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(dqp, qplace.data(), (size_t)std::max(Q, 1) * sizeof(int), hipMemcpyHostToDevice, h->stream));
  if (C > 0) HIPCHK(hipMemcpyAsync(dsets, sets, (size_t)N * sizeof(int), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemsetAsync(drun, 0, NN * 2 * sizeof(double), h->stream));
  HIPCHK(hipMemsetAsync(dcnt, 0, NN * 3 * sizeof(int32_t), h->stream));
  if (crosses) HIPCHK(hipMemsetAsync(dcarry, 0, NN * 2 * 64 * sizeof(double), h->stream));
  hipLaunchKernelGGL(k_map_colsum, dim3(Sm, N), dim3(64), 0, h->stream, (const double*)h->arr[BNMF_P].ring, (size_t)K * N, K, N, (const int*)dslots, cs);
  hipLaunchKernelGGL(k_trd_prep<TD_NTUM>, dim3((unsigned)(((size_t)Sm * N + 255) / 256)), dim3(256), 0, h->stream, (const double*)h->arr[BNMF_A].ring, (const double*)cs,
                     (const int*)dslots, (const int*)dperm, N, Sm, (size_t)N * G, doff, df, don);
  a.ringE = h->arr[BNMF_E].ring; a.off = doff; a.f = df; a.on = don; a.members = dmem; a.N = N; a.S = Sm; a.m = m; a.mb = mb;
  hipLaunchKernelGGL(k_trd_mean<TD_NTUM>, dim3((unsigned)(((size_t)m * N + 255) / 256)), dim3(256), 0, h->stream, a);
  const int items = trd_items(N, TL), MB = TD_T / std::min(items, TD_T);
  for (int i0 = 0; i0 < m; i0 += mb) {
    a.i0 = i0; a.cnt = std::min(mb, m - i0);
    const dim3 gc((unsigned)((a.cnt + MB - 1) / MB), (unsigned)((items + TD_T - 1) / TD_T));
    if (TL == 16) hipLaunchKernelGGL(k_trd_comoment<16>, gc, dim3(TD_T), 0, h->stream, a);
    else hipLaunchKernelGGL(k_trd_comoment<8>, gc, dim3(TD_T), 0, h->stream, a);
    hipLaunchKernelGGL(k_trd_finish<TD_NTUM>, dim3((unsigned)((a.cnt + 255) / 256)), dim3(256), 0, h->stream, a, (const int*)dsets, C, dtum, dpat, dsst);
    if (N > 1) hipLaunchKernelGGL(k_trd_pair<TD_NTUM>, dim3((unsigned)N, (unsigned)N), dim3(64), 0, h->stream, a, min_corr, crosses ? dcarry : (double*)nullptr, drun, dcnt);
    if (Q > 0 && dense) hipLaunchKernelGGL(k_trd_dense<TD_NTUM>, dim3((unsigned)Q), dim3(256), 0, h->stream, a, (const int*)dqp, ddense);
    HIPCHK(hipGetLastError());
  }
  std::vector<double> htum((size_t)TD_NTUM * m), hsst((size_t)TD_NSET * C * m), hrun(NN * 2);
  std::vector<int32_t> hpat(m), hcnt(NN * 3);
  HIPCHK(hipMemcpyAsync(htum.data(), dtum, htum.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(hpat.data(), dpat, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  if (C > 0) HIPCHK(hipMemcpyAsync(hsst.data(), dsst, hsst.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(hrun.data(), drun, hrun.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(hcnt.data(), dcnt, hcnt.size() * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  if (Q > 0 && dense) HIPCHK(hipMemcpyAsync(dense, ddense, (size_t)Q * 2 * NN * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  std::memset(info, 0, sizeof *info);
  tradeoff_finish(members.data(), m, G, N, C, min_corr, htum.data(), hpat.data(), hsst.data(), hrun.data(), hcnt.data(), tumour, pair_at, pair, setstat, info);
  info->n_used = S; info->n_matched = Sm; info->n_unmatched = S - Sm; info->n_sets = C; info->n_query = Q; info->min_corr = min_corr;
  return 0;
}

// Sparse per-tumour assignment with refit over the samples of r that used[] flags (prune.h): the member list is made here;
// k_prn_data (the members' data k-major, mm and t) and k_map_colsum run once; then per batch of samples project.h's k_proj_x (the columns
// of x that take part), k_prune (a lane per (s, member): the elimination; e_sparse and the five values in the scratch), attribution.h's
// k_attr_share and k_attr_stats with G := m and k_prn_stats (the tumour rows continued in sample order, the series).  The outputs by
// tumour, the signature rows and the info fields are prune_finish's.
static_assert(PR_NLOAD == BNMF_PRN_NLOAD && PR_NLOAD == AT_NLOAD && PR_NTUM == BNMF_PRN_NTUM && PR_NSER == BNMF_PRN_NSER && PR_NSIG == BNMF_PRN_NSIG &&
                  PR_MAX_N == BNMF_PRN_MAX_N && PR_MAX_N <= PJ_MAX_N, "prune.h, attribution.h, project.h and bnmf.h disagree");
static constexpr size_t PRN_SCRATCH_CAP = (size_t)256 << 20;    // bytes of a batch's blocks of the scratch
static int prune_impl(bnmf_handle* h, const char* fn, Range r, const int32_t* used, const int32_t* include, int n_steps, double max_loss, double* load,
                      double* tumour, double* series, double* signature, double* exposures, bnmf_prune_info* info) {
  if (int rc = range_enter(h, fn, h && info, r)) return rc;
  const int K = h->cfg.K, N = h->cfg.N, G = h->cfg.G;
  if (h->cfg.likelihood == BNMF_NORMAL)
    return fail(BNMF_EMODEL, "%s: the handle has the Normal likelihood; its refit is a different algorithm (least squares, not the KL update) and is out of scope", fn);
  std::vector<int> members;
  for (int g = 0; g < G; ++g) {
    if (include && include[g] != 0 && include[g] != 1) return fail(BNMF_EINVAL, "%s: include[%d] = %d is neither 0 nor 1", fn, g, (int)include[g]);
    if (!include || include[g]) members.push_back(g);
  }
  const int m = (int)members.size();
  if (n_steps < 1 || n_steps > 100000) return fail(BNMF_EINVAL, "%s: n_steps = %d is not in 1..100000", fn, n_steps);
  if (!std::isfinite(max_loss)) return fail(BNMF_EINVAL, "%s: max_loss = %g is not a finite number", fn, max_loss);
  std::vector<int> slots;
  if (int rc = range_slots(h, fn, r, used, true, slots)) return rc;
  const int S = (int)slots.size();
  if (S < 1) return fail(BNMF_ESIZE, "%s: no used sample", fn);
  if (m < 1) return fail(BNMF_ESIZE, "%s: no included tumour", fn);
  if (N > PR_MAX_N) return fail(BNMF_ESIZE, "%s: N = %d factors but at most BNMF_PRN_MAX_N = %d fit a lane's columns of the LDS", fn, N, PR_MAX_N);
  if (!h->arr[BNMF_P].ring || !h->arr[BNMF_E].ring || !h->arr[BNMF_A].ring) return fail(BNMF_ESTATE, "%s: nothing recorded yet", fn);
  if (int rc = post_sync(h)) return rc;
  bool reg = N <= PR_MAX_NT;
  if (const char* e = getenv("BNMF_PRN_FORM")) if (atoi(e) == 1) reg = false;                              // tests, tools: the LDS form at any N
  const int NS = prn_row_stride(N, reg);
  const size_t Nm = (size_t)N * m, KNS = (size_t)K * NS, lenP = (size_t)K * N;
  const size_t per = (((reg ? 1 : 2) + (exposures ? 1 : 0)) * Nm + (size_t)(PR_NVAL + 1) * m + KNS + N) * sizeof(double);   // scratch bytes of one sample
  long long want = (long long)std::max<size_t>(1, PRN_SCRATCH_CAP / per);
  if (const char* e = getenv("BNMF_PRN_BATCH")) { const long long v = atoll(e); if (v >= 1) want = v; }   // tests: the batch size
  const int Sb = (int)std::min<long long>({want, (long long)S, 65535LL});                                  // (a batch is the grid's y)
  const bool stage = !reg && prn_lds_bytes(K, N, false, true) <= LDS_CAP;
  const size_t lds = prn_lds_bytes(K, N, reg, stage);
  if (lds > LDS_CAP) return fail(BNMF_ESIZE, "%s: N = %d factors need %zu bytes of LDS", fn, N, lds);      // (unreachable for N <= BNMF_PRN_MAX_N)
  PrnArgs a{};
  double *cs, *dMt, *dmm, *dtt, *dxg, *dscr, *dvals, *dstate, *du, *dst, *dload, *dser, *dtst, *dtum, *dtser, *dexp; int *dslots, *dmem, *dnin, *didx;
  if (int rc = carve(h, [&](Carve& c) {
        cs = c.take<double>((size_t)S * N); dMt = c.take<double>((size_t)K * m); dmm = c.take<double>(m); dtt = c.take<double>(m);
        dxg = c.take<double>((size_t)Sb * KNS); dscr = c.take<double>((size_t)Sb * Nm); dvals = c.take<double>((size_t)Sb * PR_NVAL * m);
        dstate = reg ? nullptr : c.take<double>((size_t)Sb * Nm); du = c.take<double>((size_t)Sb * m);
        dst = c.take<double>(AT_NLOAD * Nm); dload = c.take<double>(AT_NLOAD * Nm); dser = c.take<double>((size_t)S * N);
        dtst = c.take<double>((size_t)PR_NTUM * m); dtum = c.take<double>((size_t)PR_NTUM * m); dtser = c.take<double>((size_t)PR_NSER * S);
        dexp = exposures ? c.take<double>((size_t)Sb * Nm) : nullptr;
        dslots = c.take<int>(S); dmem = c.take<int>(m); dnin = c.take<int>(Sb); didx = c.take<int>((size_t)Sb * N);
      })) return rc;
  HIPCHK(hipMemcpyAsync(dslots, slots.data(), (size_t)S * sizeof(int), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(dmem, members.data(), (size_t)m * sizeof(int), hipMemcpyHostToDevice, h->stream));
  const double *ringP = h->arr[BNMF_P].ring, *ringA = h->arr[BNMF_A].ring;
  hipLaunchKernelGGL(k_prn_data<PR_NTUM>, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, h->stream, (const int32_t*)h->dM, (const double*)h->dMf, (const int*)dmem, K,
                     m, dMt, dmm, dtt);
  hipLaunchKernelGGL(k_map_colsum, dim3(S, N), dim3(64), 0, h->stream, ringP, lenP, K, N, (const int*)dslots, cs);
  using PrnKernel = decltype(&k_prune<8, false>);
  const PrnKernel regk[5] = {nullptr, k_prune<8, false>, k_prune<16, false>, k_prune<24, false>, k_prune<32, false>};
  const PrnKernel kern = reg ? regk[NS / 8] : (stage ? k_prune<0, true> : k_prune<0, false>);
  if (int rc = opt_in_lds(kern, lds)) return rc;
  const int T = reg ? PR_T : PR_TL;
  a.xg = dxg; a.ringE = h->arr[BNMF_E].ring; a.Mt = dMt; a.mm = dmm; a.tt = dtt; a.nin = dnin; a.idx = didx; a.members = dmem; a.scr = dscr; a.vals = dvals;
  a.state = dstate; a.lenE = (size_t)N * G; a.K = K; a.N = N; a.G = G; a.m = m; a.n_steps = n_steps; a.max_loss = max_loss;
  const double tiny = 0x1p-1074;                                        // k_attr_stats counts a >= min_load: with the smallest positive double, a > 0
  std::vector<double> hexp(exposures ? (size_t)Sb * Nm : 0);
  if (exposures) std::fill(exposures, exposures + (size_t)S * N * G, std::nan(""));
  for (int s0 = 0; s0 < S; s0 += Sb) {
    const int nb = std::min(Sb, S - s0), last = s0 + nb == S ? 1 : 0;
    a.cs = cs + (size_t)s0 * N; a.slots = dslots + s0;
    hipLaunchKernelGGL(k_proj_x, dim3(nb), dim3(256), 0, h->stream, ringP, ringA, lenP, K, N, NS, (const int*)dslots + s0, (const double*)cs + (size_t)s0 * N, dxg, dnin,
                       didx);
    hipLaunchKernelGGL(kern, dim3((unsigned)((m + T - 1) / T), (unsigned)nb), dim3(T), lds, h->stream, a);
    const size_t nsm = (size_t)nb * m;
    hipLaunchKernelGGL(k_attr_share, dim3((unsigned)((nsm + 255) / 256)), dim3(256), 0, h->stream, (const double*)dscr, nb, N, m, du);
    hipLaunchKernelGGL(k_attr_stats, dim3((unsigned)((size_t)nb * N + (Nm + AT_TT - 1) / AT_TT)), dim3(AT_TT), 0, h->stream, (const double*)dscr, (const double*)du, nb,
                       N, m, S, s0, last, tiny, dst, dser, dload);
    hipLaunchKernelGGL(k_prn_stats<PR_NTUM>, dim3((unsigned)(2 * (size_t)nb + ((size_t)m + PR_TT - 1) / PR_TT)), dim3(PR_TT), 0, h->stream, (const double*)dvals,
                       (const double*)dmm, nb, m, S, s0, last, dtst, dtser, dtum);
    HIPCHK(hipGetLastError());
    if (exposures) {
      hipLaunchKernelGGL(k_proj_exposures, dim3((unsigned)(((size_t)nb * Nm + 255) / 256)), dim3(256), 0, h->stream, (const double*)dscr, nb, N, m, dexp);
      HIPCHK(hipGetLastError());
      HIPCHK(hipMemcpyAsync(hexp.data(), dexp, (size_t)nb * Nm * sizeof(double), hipMemcpyDeviceToHost, h->stream));
      HIPCHK(hipStreamSynchronize(h->stream));             // the next batch overwrites the scratch
      for (int s = 0; s < nb; ++s)
        for (int j = 0; j < m; ++j)
          std::memcpy(exposures + ((size_t)(s0 + s) * G + (size_t)members[j]) * N, hexp.data() + ((size_t)s * m + j) * N, (size_t)N * sizeof(double));
    }
  }
  std::vector<double> hl(AT_NLOAD * Nm), ht((size_t)PR_NTUM * m), htr(m), hs((size_t)PR_NSER * S), hm(m);
  HIPCHK(hipMemcpyAsync(hl.data(), dload, hl.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(ht.data(), dtum, ht.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(htr.data(), dtst + (size_t)6 * m, htr.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(hs.data(), dtser, hs.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(hm.data(), dmm, hm.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  std::memset(info, 0, sizeof *info);
  prune_finish(members.data(), m, G, N, S, hm.data(), hl.data(), ht.data(), htr.data(), hs.data(), load, tumour, signature, info);
  info->n_used = S; info->n_steps = n_steps; info->max_loss = max_loss;
  if (series) std::memcpy(series, hs.data(), hs.size() * sizeof(double));
  return 0;
}

// Cohort summary of signatures over the samples of r that used[] flags (summary.h): the member list, the aligned samples
// and their perm rows are made here; k_map_colsum runs once over the aligned samples; then per batch of samples (u is Sb m doubles and the
// general form's sorted chunks 2 Sb N nchunk chunk: the batch keeps the scratch under SUM_SCRATCH_CAP) k_sum_total, k_sum_scalar,
// k_sum_tail and the order statistics (k_sum_rank, or k_sum_sort + k_sum_select through sorted chunks) leave every value of the series;
// the statistics over the samples are summary_reduce's.
static_assert(SM_NSCAL == BNMF_SUM_NSCAL && SM_MAX_Q == BNMF_SUM_MAX_Q && SM_MAX_CHUNK == CO_MAX_CHUNK, "summary.h, coactivity.h and bnmf.h disagree");
static constexpr size_t SUM_SCRATCH_CAP = (size_t)256 << 20;    // bytes of u, sorted chunks and block partials per batch
static int summary_impl(bnmf_handle* h, const char* fn, Range r, const int32_t* used, const int32_t* include, const int32_t* perm, double min_load,
                        const double* probs, int L, double ci, double* stat, double* series, bnmf_summary_info* info) {
  if (int rc = range_enter(h, fn, h && info && probs, r)) return rc;
  const int K = h->cfg.K, N = h->cfg.N, G = h->cfg.G;
  std::vector<int> slots;
  if (int rc = range_slots(h, fn, r, used, true, slots)) return rc;
  std::vector<int> members;
  for (int g = 0; g < G; ++g) {
    if (include && include[g] != 0 && include[g] != 1) return fail(BNMF_EINVAL, "%s: include[%d] = %d is neither 0 nor 1", fn, g, (int)include[g]);
    if (!include || include[g]) members.push_back(g);
  }
  const int m = (int)members.size();
  // the aligned samples: rows[] is the row of the range of every used sample, place[] its row among the aligned ones (-1: left out)
  std::vector<int> rows, aslots, hperm, place;
  for (int s = 0; s < r.n; ++s) if (!used || used[s]) rows.push_back(s);
  const int S = (int)slots.size();
  for (int s = 0; s < S; ++s) {
    const int32_t* pr = perm ? perm + (size_t)rows[s] * N : nullptr;
    bool none = pr != nullptr;
    for (int n = 0; pr && n < N; ++n) none = none && pr[n] == -1;
    if (none) { place.push_back(-1); continue; }
    if (pr) {
      std::vector<char> seen(N, 0);
      for (int n = 0; n < N; ++n) {
        if (pr[n] < 0 || pr[n] >= N || seen[pr[n]])
          return fail(BNMF_EINVAL, "%s: perm[%d] is neither a permutation of 0..%d nor -1 throughout (sample %d of the range, factor %d: %d)", fn, rows[s], N - 1,
                      rows[s], n, (int)pr[n]);
        seen[pr[n]] = 1;
      }
    }
    place.push_back((int)aslots.size());
    aslots.push_back(slots[s]);
    for (int n = 0; n < N; ++n) hperm.push_back(pr ? pr[n] : n);
  }
  const int Sa = (int)aslots.size();
  if (!(min_load >= 0.0) || std::isinf(min_load)) return fail(BNMF_EINVAL, "%s: min_load = %g is not a finite number >= 0", fn, min_load);
  if (L < 1 || L > BNMF_SUM_MAX_Q) return fail(BNMF_EINVAL, "%s: L = %d levels, 1..%d are possible", fn, L, BNMF_SUM_MAX_Q);
  for (int l = 0; l < L; ++l) {
    if (!(probs[l] >= 0.0 && probs[l] <= 1.0)) return fail(BNMF_EINVAL, "%s: probs[%d] = %g is outside [0, 1]", fn, l, probs[l]);
    if (l > 0 && !(probs[l] > probs[l - 1])) return fail(BNMF_EINVAL, "%s: probs[%d] = %g is not above probs[%d] = %g", fn, l, probs[l], l - 1, probs[l - 1]);
  }
  if (!(ci < 1.0)) return fail(BNMF_EINVAL, "%s: credible_interval = %g must be below 1", fn, ci);
  if (S < 2) return fail(BNMF_ESIZE, "%s: %d used sample%s, the variance over the samples needs at least 2", fn, S, S == 1 ? "" : "s");
  if (Sa < 2) return fail(BNMF_ESIZE, "%s: %d aligned sample%s of %d used, the variance over the samples needs at least 2", fn, Sa, Sa == 1 ? "" : "s", S);
  if (m < 1) return fail(BNMF_ESIZE, "%s: no included tumour", fn);
  if (m > BNMF_COA_MAX_M) return fail(BNMF_ESIZE, "%s: %d included tumours, at most %d are taken", fn, m, BNMF_COA_MAX_M);
  if (!h->arr[BNMF_P].ring || !h->arr[BNMF_E].ring || !h->arr[BNMF_A].ring) return fail(BNMF_ESTATE, "%s: nothing recorded yet", fn);
  if (int rc = post_sync(h)) return rc;
  auto env_int = [](const char* name, long long dflt) { const char* e = getenv(name); const long long v = e ? atoll(e) : 0; return v >= 1 ? v : dflt; };
  int chunk = SM_MIN_CHUNK;                                                                                // a power of two in 64 .. 16,384
  { const long long want = std::min<long long>(env_int("BNMF_SUM_CHUNK", SM_MAX_CHUNK), SM_MAX_CHUNK); while ((long long)chunk * 2 <= want) chunk *= 2; }   // tests: the general form at a small m
  const int nchunk = (m + chunk - 1) / chunk;
  const bool general = nchunk > 1;
  int n2 = SM_MIN_CHUNK;                                                                                   // keys of the one-chunk form
  while (n2 < m) n2 *= 2;
  const int nb = (m + RG_BLOCK - 1) / RG_BLOCK, NSTAT = SM_NSCAL + 3 * L;
  const size_t per = (size_t)m * 8 + (general ? 2 * (size_t)N * nchunk * chunk * 8 : 0) + (size_t)nb * N * 20 + 4 * 256;
  const int Sb = (int)std::min<long long>({env_int("BNMF_SUM_BATCH", (long long)std::max<size_t>(1, SUM_SCRATCH_CAP / per)), (long long)Sa, 65535LL});   // tests: the batch
  const size_t nser = (size_t)NSTAT * Sa * N;
  SumArgs a{};
  double *cs, *dprobs; int *dslots, *dmem, *dperm;
  if (int rc = carve(h, [&](Carve& c) {
        cs = c.take<double>((size_t)Sa * N); a.ser = c.take<double>(nser); a.u = c.take<double>((size_t)Sb * m);
        a.part = c.take<double>((size_t)Sb * nb * N * 2); a.partC = c.take<int>((size_t)Sb * nb * N);
        a.sorted = general ? c.take<double>(2 * (size_t)Sb * N * nchunk * chunk) : nullptr;
        a.flag = c.take<int>((size_t)Sa * N); dprobs = c.take<double>(L);
        dslots = c.take<int>(Sa); dmem = c.take<int>(m); dperm = c.take<int>((size_t)Sa * N);
      })) return rc;
  HIPCHK(hipMemcpyAsync(dslots, aslots.data(), (size_t)Sa * sizeof(int), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(dmem, members.data(), (size_t)m * sizeof(int), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(dperm, hperm.data(), (size_t)Sa * N * sizeof(int), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(dprobs, probs, (size_t)L * sizeof(double), hipMemcpyHostToDevice, h->stream));
  if (general) HIPCHK(hipMemsetAsync(a.flag, 0, (size_t)Sa * N * sizeof(int), h->stream));
  hipLaunchKernelGGL(k_map_colsum, dim3(Sa, N), dim3(64), 0, h->stream, (const double*)h->arr[BNMF_P].ring, (size_t)K * N, K, N, (const int*)dslots, cs);
  a.ringE = h->arr[BNMF_E].ring; a.ringA = h->arr[BNMF_A].ring; a.cs = cs; a.slots = dslots; a.members = dmem; a.perm = dperm; a.probs = dprobs;
  a.lenE = (size_t)N * G; a.N = N; a.S = Sa; a.Sb = Sb; a.m = m; a.nb = nb; a.chunk = chunk; a.nchunk = nchunk; a.L = L; a.min_load = min_load;
  constexpr int T = 4;
  const int nt = (N + T - 1) / T;
  const size_t lds = (size_t)(general ? chunk : n2) * sizeof(double);
  if (int rc = general ? opt_in_lds(k_sum_sort<SM_WIDTH>, lds, lds) : opt_in_lds(k_sum_rank<SM_WIDTH>, lds, lds)) return rc;   // (the workgroup vote keeps a static word of its own: ask for the keys only)
  for (int s0 = 0; s0 < Sa; s0 += Sb) {
    const int ns = std::min(Sb, Sa - s0);
    a.s0 = s0;
    hipLaunchKernelGGL(k_sum_total<256>, dim3((unsigned)((m + 255) / 256), ns), dim3(256), 0, h->stream, a);
    hipLaunchKernelGGL(k_sum_scalar<T>, dim3(reg_units(nt, nb), ns), dim3(64), 0, h->stream, a);
    hipLaunchKernelGGL(k_sum_tail<SM_NSCAL>, dim3((unsigned)((ns + 63) / 64)), dim3(64), 0, h->stream, a, ns);
    if (!general) hipLaunchKernelGGL(k_sum_rank<SM_WIDTH>, dim3(N, ns), dim3(SM_WIDTH), lds, h->stream, a, n2);
    else {
      hipLaunchKernelGGL(k_sum_sort<SM_WIDTH>, dim3((unsigned)N * nchunk, ns, 2), dim3(SM_WIDTH), lds, h->stream, a);
      hipLaunchKernelGGL(k_sum_select<64>, dim3(N, ns), dim3(64), 0, h->stream, a);
    }
    HIPCHK(hipGetLastError());
  }
  std::vector<double> hs(nser);
  std::vector<int> hf((size_t)Sa * N);
  HIPCHK(hipMemcpyAsync(hs.data(), a.ser, nser * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(hf.data(), a.flag, hf.size() * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  // the series of the whole used range: a sample that perm leaves out is NaN throughout
  std::vector<double> full;
  const double* ser = hs.data();
  if (Sa < S) {
    full.assign((size_t)NSTAT * S * N, std::nan(""));
    for (int q = 0; q < NSTAT; ++q)
      for (int s = 0; s < S; ++s)
        if (place[s] >= 0) std::memcpy(full.data() + ((size_t)q * S + s) * N, hs.data() + ((size_t)q * Sa + place[s]) * N, (size_t)N * sizeof(double));
    ser = full.data();
  }
  if (series) std::memcpy(series, ser, (size_t)NSTAT * S * N * sizeof(double));
  if (stat) summary_reduce(ser, S, N, NSTAT, ci, stat);
  int64_t nbad = 0;
  for (int f : hf) nbad += f ? 1 : 0;
  std::memset(info, 0, sizeof *info);
  info->n_used = S; info->n_aligned = Sa; info->n_included = m; info->n_left_out = G - m; info->n_levels = L; info->n_blocks = nb; info->n_nonfinite = nbad;
  info->min_load = min_load; info->credible_interval = ci;
  return 0;
}

extern "C" {

int bnmf_map(bnmf_handle* h, int last_n, double ci, double* P_mean, double* E_mean, double* A_mode, double* top_A,
             double* P_lower, double* P_upper, double* E_lower, double* E_upper, int32_t* used, bnmf_map_info* info) {
  return map_impl(h, "bnmf_map", {false, 0, last_n}, ci, P_mean, E_mean, A_mode, top_A, P_lower, P_upper, E_lower, E_upper, used, info);
}
int bnmf_map_at(bnmf_handle* h, int end_iter, int n_samples, double ci, double* P_mean, double* E_mean, double* A_mode, double* top_A,
                double* P_lower, double* P_upper, double* E_lower, double* E_upper, int32_t* used, bnmf_map_info* info) {
  return map_impl(h, "bnmf_map_at", {true, end_iter, n_samples}, ci, P_mean, E_mean, A_mode, top_A, P_lower, P_upper, E_lower, E_upper, used, info);
}
int bnmf_waic(bnmf_handle* h, int last_n, const int32_t* used, double* col, double* cell, bnmf_waic_info* info) {
  return waic_impl(h, "bnmf_waic", {false, 0, last_n}, used, col, cell, info);
}
int bnmf_waic_at(bnmf_handle* h, int end_iter, int n_samples, const int32_t* used, double* col, double* cell, bnmf_waic_info* info) {
  return waic_impl(h, "bnmf_waic_at", {true, end_iter, n_samples}, used, col, cell, info);
}
int bnmf_ppc(bnmf_handle* h, int last_n, const int32_t* used, double* col, double* cell, double* series, bnmf_ppc_info* info) {
  return ppc_impl(h, "bnmf_ppc", {false, 0, last_n}, used, col, cell, series, info);
}
int bnmf_ppc_at(bnmf_handle* h, int end_iter, int n_samples, const int32_t* used, double* col, double* cell, double* series, bnmf_ppc_info* info) {
  return ppc_impl(h, "bnmf_ppc_at", {true, end_iter, n_samples}, used, col, cell, series, info);
}
int bnmf_attribution(bnmf_handle* h, int last_n, const int32_t* used, double min_load, double* load, double* prob, double* series, bnmf_attr_info* info) {
  return attr_impl(h, "bnmf_attribution", {false, 0, last_n}, used, min_load, load, prob, series, info);
}
int bnmf_attribution_at(bnmf_handle* h, int end_iter, int n_samples, const int32_t* used, double min_load, double* load, double* prob, double* series,
                        bnmf_attr_info* info) {
  return attr_impl(h, "bnmf_attribution_at", {true, end_iter, n_samples}, used, min_load, load, prob, series, info);
}
int bnmf_mixing(bnmf_handle* h, int last_n, const int32_t* used, const int32_t* keep, double* P_out, double* E_out, bnmf_mixing_info* info) {
  return mixing_impl(h, "bnmf_mixing", {false, 0, last_n}, used, keep, P_out, E_out, info);
}
int bnmf_mixing_at(bnmf_handle* h, int end_iter, int n_samples, const int32_t* used, const int32_t* keep, double* P_out, double* E_out,
                   bnmf_mixing_info* info) {
  return mixing_impl(h, "bnmf_mixing_at", {true, end_iter, n_samples}, used, keep, P_out, E_out, info);
}
int bnmf_assign(bnmf_handle* h, int last_n, const int32_t* used, const double* ref, int R, const int32_t* keep, const double* MAP_P,
                double ci, double* votes, int32_t* assigned, double* MAP_cosine, double* lower, double* upper) {
  return assign_impl(h, "bnmf_assign", {false, 0, last_n}, used, ref, R, keep, MAP_P, ci, votes, assigned, MAP_cosine, lower, upper);
}
int bnmf_assign_at(bnmf_handle* h, int end_iter, int n_samples, const int32_t* used, const double* ref, int R, const int32_t* keep, const double* MAP_P,
                   double ci, double* votes, int32_t* assigned, double* MAP_cosine, double* lower, double* upper) {
  return assign_impl(h, "bnmf_assign_at", {true, end_iter, n_samples}, used, ref, R, keep, MAP_P, ci, votes, assigned, MAP_cosine, lower, upper);
}
int bnmf_relabel(bnmf_handle* h, int last_n, const int32_t* used, const double* pivot_P, int max_rounds, int32_t* perm, double* cosine, int64_t* confusion,
                 double* P_out, double* E_out, double* aligned_P, double* aligned_E, bnmf_relabel_info* info) {
  return relabel_impl(h, "bnmf_relabel", {false, 0, last_n}, used, pivot_P, max_rounds, perm, cosine, confusion, P_out, E_out, aligned_P, aligned_E, info);
}
int bnmf_relabel_at(bnmf_handle* h, int end_iter, int n_samples, const int32_t* used, const double* pivot_P, int max_rounds, int32_t* perm, double* cosine,
                    int64_t* confusion, double* P_out, double* E_out, double* aligned_P, double* aligned_E, bnmf_relabel_info* info) {
  return relabel_impl(h, "bnmf_relabel_at", {true, end_iter, n_samples}, used, pivot_P, max_rounds, perm, cosine, confusion, P_out, E_out, aligned_P, aligned_E, info);
}

int bnmf_project(bnmf_handle* h, int last_n, const int32_t* used, const double* X, int J, int n_steps, double min_load, double* load, double* fit,
                 double* series, double* exposures, bnmf_project_info* info) {
  return project_impl(h, "bnmf_project", {false, 0, last_n}, used, X, J, n_steps, min_load, load, fit, series, exposures, info);
}
int bnmf_project_at(bnmf_handle* h, int end_iter, int n_samples, const int32_t* used, const double* X, int J, int n_steps, double min_load, double* load,
                    double* fit, double* series, double* exposures, bnmf_project_info* info) {
  return project_impl(h, "bnmf_project_at", {true, end_iter, n_samples}, used, X, J, n_steps, min_load, load, fit, series, exposures, info);
}

int bnmf_decompose(bnmf_handle* h, int last_n, const int32_t* used, const double* reference_P, int R, const int32_t* keep, int n_steps, double min_share,
                   double* weight, double* fit, int32_t* nactive, int32_t* included, double* weights, bnmf_decompose_info* info) {
  return decompose_impl(h, "bnmf_decompose", {false, 0, last_n}, used, reference_P, R, keep, n_steps, min_share, weight, fit, nactive, included, weights, info);
}
int bnmf_decompose_at(bnmf_handle* h, int end_iter, int n_samples, const int32_t* used, const double* reference_P, int R, const int32_t* keep, int n_steps,
                      double min_share, double* weight, double* fit, int32_t* nactive, int32_t* included, double* weights, bnmf_decompose_info* info) {
  return decompose_impl(h, "bnmf_decompose_at", {true, end_iter, n_samples}, used, reference_P, R, keep, n_steps, min_share, weight, fit, nactive, included,
                        weights, info);
}

int bnmf_contrast(bnmf_handle* h, int last_n, const int32_t* used, const int32_t* groups, double min_load, double credible_interval, double* group, double* pair,
                  double* series, int32_t* sizes, bnmf_contrast_info* info) {
  return contrast_impl(h, "bnmf_contrast", {false, 0, last_n}, used, groups, min_load, credible_interval, group, pair, series, sizes, info);
}
int bnmf_contrast_at(bnmf_handle* h, int end_iter, int n_samples, const int32_t* used, const int32_t* groups, double min_load, double credible_interval,
                     double* group, double* pair, double* series, int32_t* sizes, bnmf_contrast_info* info) {
  return contrast_impl(h, "bnmf_contrast_at", {true, end_iter, n_samples}, used, groups, min_load, credible_interval, group, pair, series, sizes, info);
}

int bnmf_regress(bnmf_handle* h, int last_n, const int32_t* used, const double* design, int Q, const int32_t* include, double credible_interval, double* coef,
                 double* fit, double* coef_series, double* r2_series, bnmf_regress_info* info) {
  return regress_impl(h, "bnmf_regress", {false, 0, last_n}, used, design, Q, include, credible_interval, coef, fit, coef_series, r2_series, info);
}
int bnmf_regress_at(bnmf_handle* h, int end_iter, int n_samples, const int32_t* used, const double* design, int Q, const int32_t* include,
                    double credible_interval, double* coef, double* fit, double* coef_series, double* r2_series, bnmf_regress_info* info) {
  return regress_impl(h, "bnmf_regress_at", {true, end_iter, n_samples}, used, design, Q, include, credible_interval, coef, fit, coef_series, r2_series, info);
}

int bnmf_coactivity(bnmf_handle* h, int last_n, const int32_t* used, const int32_t* include, double min_load, double credible_interval, double* pair,
                    double* series, bnmf_coactivity_info* info) {
  return coactivity_impl(h, "bnmf_coactivity", {false, 0, last_n}, used, include, min_load, credible_interval, pair, series, info);
}
int bnmf_coactivity_at(bnmf_handle* h, int end_iter, int n_samples, const int32_t* used, const int32_t* include, double min_load, double credible_interval,
                       double* pair, double* series, bnmf_coactivity_info* info) {
  return coactivity_impl(h, "bnmf_coactivity_at", {true, end_iter, n_samples}, used, include, min_load, credible_interval, pair, series, info);
}

int bnmf_stability(bnmf_handle* h, int last_n, const int32_t* used, const int32_t* labels, const double* extra_P, const int32_t* extra_label, int X,
                   double* point, double* factor, double* between, double* medoid, int64_t* medoid_at, bnmf_stability_info* info) {
  return stability_impl(h, "bnmf_stability", {false, 0, last_n}, used, labels, extra_P, extra_label, X, point, factor, between, medoid, medoid_at, info);
}
int bnmf_stability_at(bnmf_handle* h, int end_iter, int n_samples, const int32_t* used, const int32_t* labels, const double* extra_P,
                      const int32_t* extra_label, int X, double* point, double* factor, double* between, double* medoid, int64_t* medoid_at,
                      bnmf_stability_info* info) {
  return stability_impl(h, "bnmf_stability_at", {true, end_iter, n_samples}, used, labels, extra_P, extra_label, X, point, factor, between, medoid, medoid_at, info);
}

int bnmf_reconstruction(bnmf_handle* h, int last_n, const int32_t* used, double min_cosine, double min_drop, double* tumour, double* drop, double* series,
                        double* signature, bnmf_reconstruction_info* info) {
  return reconstruction_impl(h, "bnmf_reconstruction", {false, 0, last_n}, used, min_cosine, min_drop, tumour, drop, series, signature, info);
}
int bnmf_reconstruction_at(bnmf_handle* h, int end_iter, int n_samples, const int32_t* used, double min_cosine, double min_drop, double* tumour, double* drop,
                           double* series, double* signature, bnmf_reconstruction_info* info) {
  return reconstruction_impl(h, "bnmf_reconstruction_at", {true, end_iter, n_samples}, used, min_cosine, min_drop, tumour, drop, series, signature, info);
}

int bnmf_similarity(bnmf_handle* h, int last_n, const int32_t* used, const int32_t* include, const int32_t* query, int Q, int top_k, double min_cosine,
                    int32_t* neighbour_at, double* neighbour, double* dense, double* tumour, bnmf_similarity_info* info) {
  return similarity_impl(h, "bnmf_similarity", {false, 0, last_n}, used, include, query, Q, top_k, min_cosine, neighbour_at, neighbour, dense, tumour, info);
}
int bnmf_similarity_at(bnmf_handle* h, int end_iter, int n_samples, const int32_t* used, const int32_t* include, const int32_t* query, int Q, int top_k,
                       double min_cosine, int32_t* neighbour_at, double* neighbour, double* dense, double* tumour, bnmf_similarity_info* info) {
  return similarity_impl(h, "bnmf_similarity_at", {true, end_iter, n_samples}, used, include, query, Q, top_k, min_cosine, neighbour_at, neighbour, dense,
                         tumour, info);
}

int bnmf_subtypes(bnmf_handle* h, int last_n, const int32_t* used, const int32_t* include, const int32_t* perm, const double* centres0, int C, int n_steps,
                  const int32_t* query, int Q, double min_certainty, double* membership, int32_t* label, double* tumour, double* centre, double* size,
                  double* together, int32_t* labels, double* series, bnmf_subtypes_info* info) {
  return subtypes_impl(h, "bnmf_subtypes", {false, 0, last_n}, used, include, perm, centres0, C, n_steps, query, Q, min_certainty, membership, label, tumour, centre,
                       size, together, labels, series, info);
}
int bnmf_subtypes_at(bnmf_handle* h, int end_iter, int n_samples, const int32_t* used, const int32_t* include, const int32_t* perm, const double* centres0, int C,
                     int n_steps, const int32_t* query, int Q, double min_certainty, double* membership, int32_t* label, double* tumour, double* centre,
                     double* size, double* together, int32_t* labels, double* series, bnmf_subtypes_info* info) {
  return subtypes_impl(h, "bnmf_subtypes_at", {true, end_iter, n_samples}, used, include, perm, centres0, C, n_steps, query, Q, min_certainty, membership, label,
                       tumour, centre, size, together, labels, series, info);
}

int bnmf_residuals(bnmf_handle* h, int last_n, const int32_t* used, const int32_t* include, int n_steps, double max_dispersion, double* gram, double* type,
                   double* component, double* tumour, double* series, bnmf_residuals_info* info) {
  return residuals_impl(h, "bnmf_residuals", {false, 0, last_n}, used, include, n_steps, max_dispersion, gram, type, component, tumour, series, info);
}
int bnmf_residuals_at(bnmf_handle* h, int end_iter, int n_samples, const int32_t* used, const int32_t* include, int n_steps, double max_dispersion, double* gram,
                      double* type, double* component, double* tumour, double* series, bnmf_residuals_info* info) {
  return residuals_impl(h, "bnmf_residuals_at", {true, end_iter, n_samples}, used, include, n_steps, max_dispersion, gram, type, component, tumour, series, info);
}

int bnmf_tradeoff(bnmf_handle* h, int last_n, const int32_t* used, const int32_t* include, const int32_t* perm, const int32_t* sets, int C, const int32_t* query,
                  int Q, double min_corr, double* tumour, int32_t* pair_at, double* pair, double* dense, double* setstat, bnmf_tradeoff_info* info) {
  return tradeoff_impl(h, "bnmf_tradeoff", {false, 0, last_n}, used, include, perm, sets, C, query, Q, min_corr, tumour, pair_at, pair, dense, setstat, info);
}
int bnmf_tradeoff_at(bnmf_handle* h, int end_iter, int n_samples, const int32_t* used, const int32_t* include, const int32_t* perm, const int32_t* sets, int C,
                     const int32_t* query, int Q, double min_corr, double* tumour, int32_t* pair_at, double* pair, double* dense, double* setstat,
                     bnmf_tradeoff_info* info) {
  return tradeoff_impl(h, "bnmf_tradeoff_at", {true, end_iter, n_samples}, used, include, perm, sets, C, query, Q, min_corr, tumour, pair_at, pair, dense, setstat,
                       info);
}

int bnmf_prune(bnmf_handle* h, int last_n, const int32_t* used, const int32_t* include, int n_steps, double max_loss, double* load, double* tumour,
               double* series, double* signature, double* exposures, bnmf_prune_info* info) {
  return prune_impl(h, "bnmf_prune", Range{false, 0, last_n}, used, include, n_steps, max_loss, load, tumour, series, signature, exposures, info);
}
int bnmf_prune_at(bnmf_handle* h, int end_iter, int n_samples, const int32_t* used, const int32_t* include, int n_steps, double max_loss, double* load,
                  double* tumour, double* series, double* signature, double* exposures, bnmf_prune_info* info) {
  return prune_impl(h, "bnmf_prune_at", Range{true, end_iter, n_samples}, used, include, n_steps, max_loss, load, tumour, series, signature, exposures, info);
}

int bnmf_summary(bnmf_handle* h, int last_n, const int32_t* used, const int32_t* include, const int32_t* perm, double min_load, const double* probs, int L,
                 double credible_interval, double* stat, double* series, bnmf_summary_info* info) {
  return summary_impl(h, "bnmf_summary", Range{false, 0, last_n}, used, include, perm, min_load, probs, L, credible_interval, stat, series, info);
}
int bnmf_summary_at(bnmf_handle* h, int end_iter, int n_samples, const int32_t* used, const int32_t* include, const int32_t* perm, double min_load,
                    const double* probs, int L, double credible_interval, double* stat, double* series, bnmf_summary_info* info) {
  return summary_impl(h, "bnmf_summary_at", Range{true, end_iter, n_samples}, used, include, perm, min_load, probs, L, credible_interval, stat, series, info);
}

// plot_label_switching's per-sample hungarian_assignment(P_t, reference_P, keep_all_est = TRUE) diagonal (R/postprocessing_visualizations.R:
// 598-669) over the recorded iterations iters[]: k_label_switch, one wave per sample with the cosine matrix in the LDS; past the LDS,
// k_ref_cosine + k_hungarian (what bnmf_assign runs) over chunks of samples whose cosines stay within LS_CHUNK_BYTES, then k_label_gather.
int bnmf_label_switching(bnmf_handle* h, const int32_t* iters, int n_iters, const double* ref, int R, int32_t* assigned, double* cosine,
                         int32_t* included) {
  if (!h || !iters || !ref || !assigned || !cosine) return fail(BNMF_EINVAL, "bnmf_label_switching: null argument");
  if (int rc = check_recorded(h, "bnmf_label_switching")) return rc;
  if (!h->arr[BNMF_P].ring || !h->arr[BNMF_A].ring) return fail(BNMF_ESTATE, "bnmf_label_switching: nothing recorded yet");
  if (n_iters < 0) return fail(BNMF_EINVAL, "bnmf_label_switching: n_iters < 0");
  if (R < 1) return fail(BNMF_EINVAL, "bnmf_label_switching: empty reference");
  const int K = h->cfg.K, N = h->cfg.N;
  std::vector<int> slots(n_iters);
  for (int i = 0; i < n_iters; ++i) {
    if (int rc = check_kept(h, "bnmf_label_switching", iters[i], iters[i])) return rc;
    slots[i] = (int)((size_t)(iters[i] - 1) % (size_t)h->wcap);
  }
  if (n_iters == 0) return 0;
  if (int rc = post_sync(h)) return rc;
  const int tr = N > R ? 1 : 0, nrow = tr ? R : N, ncol = tr ? N : R;
  const size_t hung_lds = hungarian_lds_bytes(nrow, ncol);
  const size_t ls_lds = (size_t)N * R * sizeof(double) + hung_lds;
  const bool fused = ls_lds <= LDS_CAP;
  if (!fused && hung_lds > LDS_CAP) return fail(BNMF_ESIZE, "bnmf_label_switching: %d x %d assignment problem exceeds the LDS of one workgroup", nrow, ncol);
  const size_t per = (size_t)N * R * sizeof(double);
  const int chunk = fused ? 0 : (int)std::max<size_t>(1, std::min<size_t>((size_t)n_iters, LS_CHUNK_BYTES / per));
  const size_t out_n = (size_t)n_iters * N;
  double *dRef, *dN2, *dCs, *dCos; int *dSl, *dSig; int32_t *dAs, *dInc, *dCol;
  if (int rc = carve(h, [&](Carve& c) {
        dRef = c.take<double>((size_t)K * R); dN2 = c.take<double>(R); dSl = c.take<int>(n_iters);
        dAs = c.take<int32_t>(out_n); dCs = c.take<double>(out_n); dInc = c.take<int32_t>(out_n); dSig = c.take<int>(N);
        dCos = c.take<double>((size_t)chunk * N * R); dCol = c.take<int32_t>((size_t)chunk * nrow);
      })) return rc;
  std::vector<double> rn2;
  if (int rc = catalogue_upload(ref, K, R, dRef, dN2, rn2)) return rc;
  HIPCHK(hipMemcpy(dSl, slots.data(), (size_t)n_iters * sizeof(int), hipMemcpyHostToDevice));
  const double* ringP = h->arr[BNMF_P].ring;
  const double* ringA = h->arr[BNMF_A].ring;
  if (fused) {
    if (int rc = opt_in_lds(k_label_switch, ls_lds, ls_lds)) return rc;
    hipLaunchKernelGGL(k_label_switch, dim3(n_iters), dim3(64), ls_lds, h->stream, ringP, ringA, K, N, (const int*)dSl, (const double*)dRef,
                       (const double*)dN2, R, dAs, dCs, dInc);
    HIPCHK(hipGetLastError());
  } else {
    std::vector<int> sig(N);
    for (int n = 0; n < N; ++n) sig[n] = n;
    HIPCHK(hipMemcpy(dSig, sig.data(), (size_t)N * sizeof(int), hipMemcpyHostToDevice));
    if (int rc = opt_in_lds(k_hungarian, hung_lds, hung_lds)) return rc;
    for (int s0 = 0; s0 < n_iters; s0 += chunk) {
      const int ns = std::min(chunk, n_iters - s0);
      hipLaunchKernelGGL(k_ref_cosine, dim3(ns, N), dim3(128), 0, h->stream, ringP, (size_t)K * N, K, (const int*)dSl + s0, (const int*)dSig, N,
                         (const double*)dRef, (const double*)dN2, R, dCos);
      HIPCHK(hipMemsetAsync(dCol, 0xff, (size_t)ns * nrow * sizeof(int32_t), h->stream));
      hipLaunchKernelGGL(k_hungarian, dim3(ns), dim3(64), hung_lds, h->stream, (const double*)dCos, N, R, tr, dCol);
      hipLaunchKernelGGL(k_label_gather, dim3((ns + 63) / 64), dim3(64), 0, h->stream, (const double*)dCos, (const int32_t*)dCol, N, R, ns, ringA,
                         (const int*)dSl + s0, dAs + (size_t)s0 * N, dCs + (size_t)s0 * N, dInc + (size_t)s0 * N);
      HIPCHK(hipGetLastError());
    }
  }
  HIPCHK(hipMemcpyAsync(assigned, dAs, out_n * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(cosine, dCs, out_n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (included) HIPCHK(hipMemcpyAsync(included, dInc, out_n * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  for (int i = 0; i < n_iters; ++i)
    if (assigned[(size_t)i * N] == -2 && N > 0) return fail(BNMF_ESTATE, "bnmf_label_switching: iteration %d has no assignment (a cosine is not finite)", iters[i]);
  return 0;
}

}  // extern "C"
