/* r/bnmf_shim.c — thin `.Call` shim between R and the C ABI of libbnmf.so (include/bnmf.h).
 *
 * R API only (no Rcpp, no CUDA-compat headers); logic-free marshalling: every entry point is one C-ABI
 * call.  Must be called from the R main thread; never calls back into R; inputs are read-only SEXPs
 * (copied to the device by the library); outputs are freshly allocated and PROTECTed here; errors become
 * Rf_error() with bnmf_last_error().  Build inside an R package: src/bnmf_shim.c + PKG_LIBS = -lbnmf.
 * (Not compiled in this repository's container: there is no R installation / Rinternals.h.)
 */
#include <R.h>
#include <Rinternals.h>
#include <R_ext/Rdynload.h>
#include "bnmf.h"

static void chk(int rc) { if (rc != 0) Rf_error("%s", bnmf_last_error()); }

static void handle_finalizer(SEXP ptr) {
  bnmf_handle* h = (bnmf_handle*)R_ExternalPtrAddr(ptr);
  if (h) { bnmf_destroy(h); R_ClearExternalPtr(ptr); }
}
static bnmf_handle* get_handle(SEXP ptr) {
  bnmf_handle* h = (bnmf_handle*)R_ExternalPtrAddr(ptr);
  if (!h) Rf_error("bnmf: handle was destroyed");
  return h;
}

static bnmf_config make_config(SEXP dims, SEXP spec, SEXP temperature, SEXP seed, SEXP chain_id, SEXP device) {
  bnmf_config cfg;
  const int* d = INTEGER(dims); const int* s = INTEGER(spec);
  cfg.K = d[0]; cfg.G = d[1]; cfg.N = d[2];
  cfg.likelihood = s[0]; cfg.prior = s[1]; cfg.MH = s[2]; cfg.learning_rank = s[3];
  cfg.rank_method = s[4]; cfg.save_Z = s[5]; cfg.window = s[6];
  cfg.seed = (uint64_t)REAL(seed)[0]; cfg.chain_id = (uint32_t)INTEGER(chain_id)[0]; cfg.device = INTEGER(device)[0];
  cfg.temperature = REAL(temperature); cfg.n_temperature = (int64_t)XLENGTH(temperature);
  return cfg;
}
static SEXP wrap_handle(bnmf_handle* h) {
  SEXP ptr = PROTECT(R_MakeExternalPtr(h, R_NilValue, R_NilValue));
  R_RegisterCFinalizerEx(ptr, handle_finalizer, TRUE);
  UNPROTECT(1);
  return ptr;
}
/* C_bnmf_create(data (integer K x G), dims c(K,G,N), spec c(likelihood, prior, MH, learning_rank,
 *               rank_method, save_Z, window), temperature (double), seed (double), chain_id, device) */
SEXP C_bnmf_create(SEXP data, SEXP dims, SEXP spec, SEXP temperature, SEXP seed, SEXP chain_id, SEXP device) {
  const bnmf_config cfg = make_config(dims, spec, temperature, seed, chain_id, device);
  bnmf_handle* h = NULL;
  chk(bnmf_create(&cfg, INTEGER(data), &h));
  return wrap_handle(h);
}
/* C_bnmf_create_f64: the same arguments with data as a double K x G matrix (real-valued data of the Normal likelihood) */
SEXP C_bnmf_create_f64(SEXP data, SEXP dims, SEXP spec, SEXP temperature, SEXP seed, SEXP chain_id, SEXP device) {
  const bnmf_config cfg = make_config(dims, spec, temperature, seed, chain_id, device);
  bnmf_handle* h = NULL;
  chk(bnmf_create_f64(&cfg, REAL(data), &h));
  return wrap_handle(h);
}
SEXP C_bnmf_set_array(SEXP ptr, SEXP id, SEXP value) {
  chk(bnmf_set_array(get_handle(ptr), INTEGER(id)[0], REAL(value), (size_t)XLENGTH(value)));
  return R_NilValue;
}
SEXP C_bnmf_get_array(SEXP ptr, SEXP id, SEXP n) {
  const R_xlen_t len = (R_xlen_t)REAL(n)[0];
  SEXP out = PROTECT(Rf_allocVector(REALSXP, len));
  chk(bnmf_get_array(get_handle(ptr), INTEGER(id)[0], REAL(out), (size_t)len));
  UNPROTECT(1);
  return out;
}
/* hold columns of P fixed (bnmf_set_fixed): C_bnmf_set_fixed(ptr, id (.bnmf_ids[["P"]]), mask (integer 0 / 1, length N)), before
 * C_bnmf_init / C_bnmf_load_state; C_bnmf_get_fixed(ptr, id, n (= N)) -> the mask as an integer vector.  The arguments are checked
 * before the handle is touched */
SEXP C_bnmf_set_fixed(SEXP ptr, SEXP id, SEXP mask) {
  if (XLENGTH(id) != 1) Rf_error("bnmf: id must be one integer");
  const R_xlen_t n = XLENGTH(mask);
  if (n < 1) Rf_error("bnmf: the mask of fixed columns is empty");
  const int* m = INTEGER(mask);
  int32_t* f = (int32_t*)R_alloc((size_t)n, sizeof(int32_t));
  for (R_xlen_t i = 0; i < n; ++i) {
    if (m[i] == NA_INTEGER) Rf_error("bnmf: the mask of fixed columns holds NA (entry %ld)", (long)(i + 1));
    f[i] = (int32_t)m[i];
  }
  chk(bnmf_set_fixed(get_handle(ptr), INTEGER(id)[0], f, (size_t)n));
  return R_NilValue;
}
SEXP C_bnmf_get_fixed(SEXP ptr, SEXP id, SEXP n) {
  if (XLENGTH(id) != 1 || XLENGTH(n) != 1) Rf_error("bnmf: id and n must be one number each");
  const double len = REAL(n)[0];
  if (!(len >= 1.0) || len > 2147483647.0) Rf_error("bnmf: n = %g is not a number of columns", len);
  SEXP out = PROTECT(Rf_allocVector(INTSXP, (R_xlen_t)len));
  chk(bnmf_get_fixed(get_handle(ptr), INTEGER(id)[0], (int32_t*)INTEGER(out), (size_t)len));
  UNPROTECT(1);
  return out;
}
SEXP C_bnmf_init(SEXP ptr) {
  SEXP row = PROTECT(Rf_allocVector(REALSXP, BNMF_NMETRIC));
  chk(bnmf_init(get_handle(ptr), REAL(row)));
  UNPROTECT(1);
  return row;
}
/* returns a (BNMF_NMETRIC x n_iter) double matrix (column-major: one column per iteration) */
SEXP C_bnmf_run(SEXP ptr, SEXP n_iter, SEXP converged) {
  const int n = INTEGER(n_iter)[0];
  SEXP out = PROTECT(Rf_allocMatrix(REALSXP, BNMF_NMETRIC, n));
  chk(bnmf_run(get_handle(ptr), n, LOGICAL(converged)[0], REAL(out)));
  UNPROTECT(1);
  return out;
}
/* returns a (len x last_n) double matrix: one recorded sample per column, oldest first */
SEXP C_bnmf_window(SEXP ptr, SEXP id, SEXP last_n, SEXP len) {
  const int n = INTEGER(last_n)[0]; const R_xlen_t l = (R_xlen_t)REAL(len)[0];
  SEXP out = PROTECT(Rf_allocMatrix(REALSXP, (int)l, n));
  chk(bnmf_window(get_handle(ptr), INTEGER(id)[0], n, REAL(out)));
  UNPROTECT(1);
  return out;
}
SEXP C_bnmf_get_iter(SEXP ptr) {
  int it = 0;
  chk(bnmf_get_iter(get_handle(ptr), &it));
  return Rf_ScalarInteger(it);
}
static SEXP named_list(int n, const char** names) {
  SEXP out = PROTECT(Rf_allocVector(VECSXP, n)), nm = PROTECT(Rf_allocVector(STRSXP, n));
  for (int i = 0; i < n; ++i) SET_STRING_ELT(nm, i, Rf_mkChar(names[i]));
  Rf_setAttrib(out, R_NamesSymbol, nm);
  UNPROTECT(2);
  return out;
}
/* get_MAP_ on the device (R/utils.R:194-288): C_bnmf_map(ptr, last_n, credible_interval (<= 0: no bounds), dims c(K,G,N)) ->
 * list(P K x N, E N x G, A, top_A 5 x N (row i = i-th most frequent pattern), P_lower, P_upper, E_lower, E_upper, used (logical),
 *      n_used, n_patterns, top_counts, rmse, kl) */
/* the result list of C_bnmf_map / C_bnmf_map_at, its buffers allocated (elements 0-8: P, E, A, top_A (5 x N row-major until
 * map_finish), the four bounds or NULL, used (integer until map_finish)); returned unprotected */
static SEXP map_alloc(int n, int want, SEXP dims) {
  const int* d = INTEGER(dims); const int K = d[0], G = d[1], N = d[2];
  static const char* nms[] = {"P", "E", "A", "top_A", "P_lower", "P_upper", "E_lower", "E_upper", "used", "n_used", "n_patterns", "top_counts", "rmse", "kl"};
  SEXP out = PROTECT(named_list(14, nms));
  SET_VECTOR_ELT(out, 0, Rf_allocMatrix(REALSXP, K, N)); SET_VECTOR_ELT(out, 1, Rf_allocMatrix(REALSXP, N, G));
  SET_VECTOR_ELT(out, 2, Rf_allocMatrix(REALSXP, 1, N)); SET_VECTOR_ELT(out, 3, Rf_allocVector(REALSXP, 5 * (R_xlen_t)N));
  if (want) {
    SET_VECTOR_ELT(out, 4, Rf_allocMatrix(REALSXP, K, N)); SET_VECTOR_ELT(out, 5, Rf_allocMatrix(REALSXP, K, N));
    SET_VECTOR_ELT(out, 6, Rf_allocMatrix(REALSXP, N, G)); SET_VECTOR_ELT(out, 7, Rf_allocMatrix(REALSXP, N, G));
  }
  SET_VECTOR_ELT(out, 8, Rf_allocVector(INTSXP, n));
  UNPROTECT(1);
  return out;
}
static double* map_buf(SEXP out, int i) { SEXP x = VECTOR_ELT(out, i); return x == R_NilValue ? NULL : REAL(x); }
static void map_finish(SEXP out, int n, SEXP dims, const bnmf_map_info* info) {
  const int N = INTEGER(dims)[2];
  SEXP topm = PROTECT(Rf_allocMatrix(REALSXP, 5, N));                     /* row-major 5 x N -> R matrix */
  const double* top = REAL(VECTOR_ELT(out, 3));
  for (int i = 0; i < 5; ++i) for (int j = 0; j < N; ++j) REAL(topm)[i + 5 * j] = top[(size_t)i * N + j];
  SEXP usedl = PROTECT(Rf_allocVector(LGLSXP, n));
  const int* used = INTEGER(VECTOR_ELT(out, 8));
  for (int i = 0; i < n; ++i) LOGICAL(usedl)[i] = used[i] != 0;
  SEXP tc = PROTECT(Rf_allocVector(INTSXP, 5));
  for (int i = 0; i < 5; ++i) INTEGER(tc)[i] = info->top_counts[i];
  SET_VECTOR_ELT(out, 3, topm); SET_VECTOR_ELT(out, 8, usedl); SET_VECTOR_ELT(out, 11, tc);
  UNPROTECT(3);
  SET_VECTOR_ELT(out, 9, Rf_ScalarInteger(info->n_used)); SET_VECTOR_ELT(out, 10, Rf_ScalarInteger(info->n_patterns));
  SET_VECTOR_ELT(out, 12, Rf_ScalarReal(info->rmse)); SET_VECTOR_ELT(out, 13, Rf_ScalarReal(info->kl));
}
SEXP C_bnmf_map(SEXP ptr, SEXP last_n, SEXP ci, SEXP dims) {
  const int n = INTEGER(last_n)[0]; const double c = REAL(ci)[0];
  SEXP out = PROTECT(map_alloc(n, c > 0.0, dims));
  bnmf_map_info info;
  chk(bnmf_map(get_handle(ptr), n, c, map_buf(out, 0), map_buf(out, 1), map_buf(out, 2), map_buf(out, 3), map_buf(out, 4), map_buf(out, 5),
               map_buf(out, 6), map_buf(out, 7), INTEGER(VECTOR_ELT(out, 8)), &info));
  map_finish(out, n, dims, &info);
  UNPROTECT(1);
  return out;
}
/* get_MAP_(end_iter, n_samples) (R/utils.R:194-230): C_bnmf_map_at(ptr, end_iter, n_samples, credible_interval, dims) -> the list of
 * C_bnmf_map over iterations end_iter - n_samples + 1 ... end_iter */
SEXP C_bnmf_map_at(SEXP ptr, SEXP end_iter, SEXP n_samples, SEXP ci, SEXP dims) {
  const int n = INTEGER(n_samples)[0]; const double c = REAL(ci)[0];
  SEXP out = PROTECT(map_alloc(n, c > 0.0, dims));
  bnmf_map_info info;
  chk(bnmf_map_at(get_handle(ptr), INTEGER(end_iter)[0], n, c, map_buf(out, 0), map_buf(out, 1), map_buf(out, 2), map_buf(out, 3), map_buf(out, 4),
                  map_buf(out, 5), map_buf(out, 6), map_buf(out, 7), INTEGER(VECTOR_ELT(out, 8)), &info));
  map_finish(out, n, dims, &info);
  UNPROTECT(1);
  return out;
}
/* convergence control / state marshalling: cc_int = c(MAP_over, MAP_every, Ninarow_nochange, Ninarow_nobest, miniters, maxiters,
 * metric (0 loglikelihood, 1 logposterior, 2 RMSE, 3 KL, 4 BIC)); state = c(converged, why, best_iter, inarow_na, inarow_no_change,
 * inarow_no_best, have_prev, n_checks, prev_MAP_metric, best_MAP_metric, prev_percent_change) */
static void cc_in(SEXP cc_int, SEXP tol, bnmf_convergence_control* cc) {
  const int* c = INTEGER(cc_int);
  cc->MAP_over = c[0]; cc->MAP_every = c[1]; cc->Ninarow_nochange = c[2]; cc->Ninarow_nobest = c[3]; cc->miniters = c[4];
  cc->maxiters = c[5]; cc->metric = c[6]; cc->_pad = 0; cc->tol = REAL(tol)[0];
}
static void st_in(SEXP state, bnmf_convergence_state* st) {
  const double* v = REAL(state);
  st->converged = (int)v[0]; st->why = (int)v[1]; st->best_iter = (int)v[2]; st->inarow_na = (int)v[3]; st->inarow_no_change = (int)v[4];
  st->inarow_no_best = (int)v[5]; st->have_prev = (int)v[6]; st->n_checks = (int)v[7];
  st->prev_MAP_metric = v[8]; st->best_MAP_metric = v[9]; st->prev_percent_change = v[10];
}
static SEXP loop_out(const double* met, int n_rows, const double* maps, int n_checks, const bnmf_convergence_state* st) {
  static const char* nms[] = {"metrics", "map_rows", "state"};
  SEXP out = PROTECT(named_list(3, nms));
  SEXP m = PROTECT(Rf_allocMatrix(REALSXP, BNMF_NMETRIC, n_rows)), r = PROTECT(Rf_allocMatrix(REALSXP, BNMF_NMAPROW, n_checks));
  SEXP s = PROTECT(Rf_allocVector(REALSXP, 11));
  for (R_xlen_t i = 0; i < (R_xlen_t)BNMF_NMETRIC * n_rows; ++i) REAL(m)[i] = met[i];      /* one column per iteration */
  for (R_xlen_t i = 0; i < (R_xlen_t)BNMF_NMAPROW * n_checks; ++i) REAL(r)[i] = maps[i];   /* one column per MAP check */
  double* v = REAL(s);
  v[0] = st->converged; v[1] = st->why; v[2] = st->best_iter; v[3] = st->inarow_na; v[4] = st->inarow_no_change; v[5] = st->inarow_no_best;
  v[6] = st->have_prev; v[7] = st->n_checks; v[8] = st->prev_MAP_metric; v[9] = st->best_MAP_metric; v[10] = st->prev_percent_change;
  SET_VECTOR_ELT(out, 0, m); SET_VECTOR_ELT(out, 1, r); SET_VECTOR_ELT(out, 2, s);
  UNPROTECT(4);
  return out;
}
/* the warm-up loop to convergence in one call (R/bayesNMF_sampler.R:268-330) */
SEXP C_bnmf_run_until(SEXP ptr, SEXP cc_int, SEXP tol, SEXP state) {
  bnmf_convergence_control cc; bnmf_convergence_state st;
  cc_in(cc_int, tol, &cc); st_in(state, &st);
  int it = 0;
  chk(bnmf_get_iter(get_handle(ptr), &it));
  const int cap_rows = (cc.maxiters > it ? cc.maxiters - it : 0) + 1, cap_checks = cap_rows / cc.MAP_every + 2;
  double* met = (double*)R_alloc((size_t)cap_rows * BNMF_NMETRIC, sizeof(double));
  double* maps = (double*)R_alloc((size_t)cap_checks * BNMF_NMAPROW, sizeof(double));
  int n_rows = 0, n_checks = 0;
  chk(bnmf_run_until(get_handle(ptr), &cc, &st, met, cap_rows, &n_rows, maps, cap_checks, &n_checks));
  return loop_out(met, n_rows, maps, n_checks, &st);
}
/* the MH models' post-warm-up iterations in one call (R/bayesNMF_sampler.R:332-384) */
SEXP C_bnmf_run_post_warmup(SEXP ptr, SEXP cc_int, SEXP tol, SEXP state, SEXP post_warmup) {
  bnmf_convergence_control cc; bnmf_convergence_state st;
  cc_in(cc_int, tol, &cc); st_in(state, &st);
  const int pw = INTEGER(post_warmup)[0];
  const int cap_rows = pw + 1, cap_checks = cap_rows / cc.MAP_every + 3;
  double* met = (double*)R_alloc((size_t)cap_rows * BNMF_NMETRIC, sizeof(double));
  double* maps = (double*)R_alloc((size_t)cap_checks * BNMF_NMAPROW, sizeof(double));
  int n_rows = 0, n_checks = 0;
  chk(bnmf_run_post_warmup(get_handle(ptr), &cc, &st, pw, met, cap_rows, &n_rows, maps, cap_checks, &n_checks));
  return loop_out(met, n_rows, maps, n_checks, &st);
}
/* assign_signatures_ensemble_ (R/postprocessing.R:175-341): C_bnmf_assign(ptr, last_n, used (logical, or NULL = all), reference_P
 * (K x R), keep (logical length N, or NULL), MAP_P (K x N, or NULL), credible_interval, dims c(K,G,N)) ->
 * list(votes N x R, assigned (1-based column of reference_P, NA = not kept), MAP_cosine, lower, upper) */
/* the result list of C_bnmf_assign / C_bnmf_assign_at, its buffers allocated; returned unprotected */
static SEXP assign_alloc(int N, int R) {
  static const char* nms[] = {"votes", "assigned", "MAP_cosine", "lower", "upper"};
  SEXP out = PROTECT(named_list(5, nms));
  SET_VECTOR_ELT(out, 0, Rf_allocMatrix(REALSXP, N, R)); SET_VECTOR_ELT(out, 1, Rf_allocVector(INTSXP, N));
  for (int i = 2; i < 5; ++i) SET_VECTOR_ELT(out, i, Rf_allocVector(REALSXP, N));
  UNPROTECT(1);
  return out;
}
static int32_t* lgl_flags(SEXP x, int n) {                                /* logical (or NULL) -> 0/1 flags (NA counts as FALSE) */
  if (x == R_NilValue) return NULL;
  int32_t* f = (int32_t*)R_alloc(n, sizeof(int32_t));
  for (int i = 0; i < n; ++i) f[i] = LOGICAL(x)[i] == TRUE;
  return f;
}
static void assign_finish(SEXP out, int N) {                              /* 1-based columns of reference_P, NA = not kept */
  int* a = INTEGER(VECTOR_ELT(out, 1));
  for (int i = 0; i < N; ++i) a[i] = a[i] < 0 ? NA_INTEGER : a[i] + 1;
}
SEXP C_bnmf_assign(SEXP ptr, SEXP last_n, SEXP used, SEXP reference_P, SEXP keep, SEXP MAP_P, SEXP ci, SEXP dims) {
  const int n = INTEGER(last_n)[0], N = INTEGER(dims)[2], R = Rf_ncols(reference_P);
  int32_t* u = lgl_flags(used, n); int32_t* kp = lgl_flags(keep, N);
  SEXP out = PROTECT(assign_alloc(N, R));
  chk(bnmf_assign(get_handle(ptr), n, u, REAL(reference_P), R, kp, MAP_P == R_NilValue ? NULL : REAL(MAP_P), REAL(ci)[0], REAL(VECTOR_ELT(out, 0)),
                  INTEGER(VECTOR_ELT(out, 1)), REAL(VECTOR_ELT(out, 2)), REAL(VECTOR_ELT(out, 3)), REAL(VECTOR_ELT(out, 4))));
  assign_finish(out, N);
  UNPROTECT(1);
  return out;
}
/* C_bnmf_assign_at(ptr, end_iter, n_samples, used (logical length n_samples, or NULL = all), reference_P, keep, MAP_P, credible_interval,
 * dims) -> the list of C_bnmf_assign over iterations end_iter - n_samples + 1 ... end_iter */
SEXP C_bnmf_assign_at(SEXP ptr, SEXP end_iter, SEXP n_samples, SEXP used, SEXP reference_P, SEXP keep, SEXP MAP_P, SEXP ci, SEXP dims) {
  const int n = INTEGER(n_samples)[0], N = INTEGER(dims)[2], R = Rf_ncols(reference_P);
  int32_t* u = lgl_flags(used, n); int32_t* kp = lgl_flags(keep, N);
  SEXP out = PROTECT(assign_alloc(N, R));
  chk(bnmf_assign_at(get_handle(ptr), INTEGER(end_iter)[0], n, u, REAL(reference_P), R, kp, MAP_P == R_NilValue ? NULL : REAL(MAP_P), REAL(ci)[0],
                     REAL(VECTOR_ELT(out, 0)), INTEGER(VECTOR_ELT(out, 1)), REAL(VECTOR_ELT(out, 2)), REAL(VECTOR_ELT(out, 3)), REAL(VECTOR_ELT(out, 4))));
  assign_finish(out, N);
  UNPROTECT(1);
  return out;
}
/* WAIC over recorded samples on the device (bnmf_waic / bnmf_waic_at): C_bnmf_waic(ptr, end_iter (integer, or NULL = the current
 * iteration), n_samples, used (logical length n_samples, or NULL = all), want_col, want_cell (logical), dims c(K,G,N)) ->
 * list(n_used, n_high_var, lppd, p_waic, elpd_waic, waic, se_elpd, mean_loglik, col (G x 3: lppd, p_waic, mean_loglik per column, or
 * NULL), lppd_cell, p_waic_cell (K x G each, or NULL)) over iterations end_iter - n_samples + 1 ... end_iter.
 * C_bnmf_waic_at: the same with end_iter required */
/* the result list with col allocated if wanted, and the flags of used; returned unprotected */
static SEXP waic_alloc(SEXP n_samples, SEXP used, SEXP want_col, SEXP dims, int32_t** u) {
  const int n = INTEGER(n_samples)[0], G = INTEGER(dims)[1];
  if (used != R_NilValue && XLENGTH(used) != (R_xlen_t)n) Rf_error("bnmf: used has %ld entries for %d samples", (long)XLENGTH(used), n);
  *u = lgl_flags(used, n);
  static const char* nms[] = {"n_used", "n_high_var", "lppd", "p_waic", "elpd_waic", "waic", "se_elpd", "mean_loglik", "col", "lppd_cell", "p_waic_cell"};
  SEXP out = PROTECT(named_list(11, nms));
  if (LOGICAL(want_col)[0] == TRUE) SET_VECTOR_ELT(out, 8, Rf_allocMatrix(REALSXP, G, 3));
  UNPROTECT(1);
  return out;
}
static double* waic_cell_buf(SEXP want_cell, SEXP dims) {
  const int* d = INTEGER(dims);
  return LOGICAL(want_cell)[0] == TRUE ? (double*)R_alloc(2 * (size_t)d[0] * (size_t)d[1], sizeof(double)) : NULL;
}
static void waic_finish(SEXP out, const double* cell, SEXP dims, const bnmf_waic_info* info) {
  const int* d = INTEGER(dims); const int K = d[0], G = d[1];
  if (cell) {
    for (int i = 0; i < 2; ++i) {
      SEXP m = Rf_allocMatrix(REALSXP, K, G);
      SET_VECTOR_ELT(out, 9 + i, m);
      for (R_xlen_t j = 0; j < (R_xlen_t)K * G; ++j) REAL(m)[j] = cell[(size_t)i * K * G + (size_t)j];
    }
  }
  SET_VECTOR_ELT(out, 0, Rf_ScalarInteger(info->n_used)); SET_VECTOR_ELT(out, 1, Rf_ScalarInteger(info->n_high_var));
  const double v[6] = {info->lppd, info->p_waic, info->elpd_waic, info->waic, info->se_elpd, info->mean_loglik};
  for (int i = 0; i < 6; ++i) SET_VECTOR_ELT(out, 2 + i, Rf_ScalarReal(v[i]));
}
SEXP C_bnmf_waic(SEXP ptr, SEXP end_iter, SEXP n_samples, SEXP used, SEXP want_col, SEXP want_cell, SEXP dims) {
  int32_t* u = NULL;
  SEXP out = PROTECT(waic_alloc(n_samples, used, want_col, dims, &u));
  double* cell = waic_cell_buf(want_cell, dims);
  bnmf_waic_info info;
  if (end_iter == R_NilValue) chk(bnmf_waic(get_handle(ptr), INTEGER(n_samples)[0], u, map_buf(out, 8), cell, &info));
  else chk(bnmf_waic_at(get_handle(ptr), INTEGER(end_iter)[0], INTEGER(n_samples)[0], u, map_buf(out, 8), cell, &info));
  waic_finish(out, cell, dims, &info);
  UNPROTECT(1);
  return out;
}
SEXP C_bnmf_waic_at(SEXP ptr, SEXP end_iter, SEXP n_samples, SEXP used, SEXP want_col, SEXP want_cell, SEXP dims) {
  int32_t* u = NULL;
  SEXP out = PROTECT(waic_alloc(n_samples, used, want_col, dims, &u));
  double* cell = waic_cell_buf(want_cell, dims);
  bnmf_waic_info info;
  chk(bnmf_waic_at(get_handle(ptr), INTEGER(end_iter)[0], INTEGER(n_samples)[0], u, map_buf(out, 8), cell, &info));
  waic_finish(out, cell, dims, &info);
  UNPROTECT(1);
  return out;
}
/* Mixing diagnostics over recorded samples on the device (bnmf_mixing / bnmf_mixing_at): C_bnmf_mixing(ptr, end_iter (integer, or NULL =
 * the current iteration), n_samples, used (logical length n_samples, or NULL = all), keep (logical length N, or NULL = all), want_arrays
 * (logical), dims c(K,G,N)) -> list(n_used, n_half, n_const, n_ran_out, n_low_ess, n_high_rhat, min_ess_P, min_ess_E, max_rhat_P,
 * max_rhat_E, min_ess_P_at, min_ess_E_at, max_rhat_P_at, max_rhat_E_at (1-based positions in P / E as doubles, 0 = none), P (K N x 11), E (N G x 11):
 * one column per row of the C output — mean, var, ess, mcse, rhat, pairs, exit, mean_a, var_a, mean_b, var_b — or NULL) over iterations
 * end_iter - n_samples + 1 ... end_iter.  C_bnmf_mixing_at: the same with end_iter required */
/* the result list with P and E allocated if wanted, and the flags of used and keep; returned unprotected */
static SEXP mixing_alloc(SEXP n_samples, SEXP used, SEXP keep, SEXP want_arrays, SEXP dims, int32_t** u, int32_t** kp) {
  const int n = INTEGER(n_samples)[0];
  const int* d = INTEGER(dims);
  if (used != R_NilValue && XLENGTH(used) != (R_xlen_t)n) Rf_error("bnmf: used has %ld entries for %d samples", (long)XLENGTH(used), n);
  if (keep != R_NilValue && XLENGTH(keep) != (R_xlen_t)d[2]) Rf_error("bnmf: keep has %ld entries for %d factors", (long)XLENGTH(keep), d[2]);
  *u = lgl_flags(used, n); *kp = lgl_flags(keep, d[2]);
  static const char* nms[] = {"n_used", "n_half", "n_const", "n_ran_out", "n_low_ess", "n_high_rhat", "min_ess_P", "min_ess_E", "max_rhat_P", "max_rhat_E",
                              "min_ess_P_at", "min_ess_E_at", "max_rhat_P_at", "max_rhat_E_at", "P", "E"};
  SEXP out = PROTECT(named_list(16, nms));
  if (LOGICAL(want_arrays)[0] == TRUE) {
    SET_VECTOR_ELT(out, 14, Rf_allocMatrix(REALSXP, d[0] * d[2], BNMF_NMIX));
    SET_VECTOR_ELT(out, 15, Rf_allocMatrix(REALSXP, d[2] * d[1], BNMF_NMIX));
  }
  UNPROTECT(1);
  return out;
}
static void mixing_finish(SEXP out, const bnmf_mixing_info* info) {
  SET_VECTOR_ELT(out, 0, Rf_ScalarInteger(info->n_used)); SET_VECTOR_ELT(out, 1, Rf_ScalarInteger(info->n_half));
  const double v[12] = {(double)info->n_const, (double)info->n_ran_out, (double)info->n_low_ess, (double)info->n_high_rhat,
                        info->min_ess_P, info->min_ess_E, info->max_rhat_P, info->max_rhat_E,
                        (double)info->min_ess_P_at, (double)info->min_ess_E_at, (double)info->max_rhat_P_at, (double)info->max_rhat_E_at};
  for (int i = 0; i < 8; ++i) SET_VECTOR_ELT(out, 2 + i, Rf_ScalarReal(v[i]));
  for (int i = 8; i < 12; ++i) SET_VECTOR_ELT(out, 2 + i, Rf_ScalarReal(v[i] + 1.0)   /* 1-based; 0 = none */);
}
SEXP C_bnmf_mixing(SEXP ptr, SEXP end_iter, SEXP n_samples, SEXP used, SEXP keep, SEXP want_arrays, SEXP dims) {
  int32_t *u = NULL, *kp = NULL;
  SEXP out = PROTECT(mixing_alloc(n_samples, used, keep, want_arrays, dims, &u, &kp));
  bnmf_mixing_info info;
  if (end_iter == R_NilValue) chk(bnmf_mixing(get_handle(ptr), INTEGER(n_samples)[0], u, kp, map_buf(out, 14), map_buf(out, 15), &info));
  else chk(bnmf_mixing_at(get_handle(ptr), INTEGER(end_iter)[0], INTEGER(n_samples)[0], u, kp, map_buf(out, 14), map_buf(out, 15), &info));
  mixing_finish(out, &info);
  UNPROTECT(1);
  return out;
}
SEXP C_bnmf_mixing_at(SEXP ptr, SEXP end_iter, SEXP n_samples, SEXP used, SEXP keep, SEXP want_arrays, SEXP dims) {
  int32_t *u = NULL, *kp = NULL;
  SEXP out = PROTECT(mixing_alloc(n_samples, used, keep, want_arrays, dims, &u, &kp));
  bnmf_mixing_info info;
  chk(bnmf_mixing_at(get_handle(ptr), INTEGER(end_iter)[0], INTEGER(n_samples)[0], u, kp, map_buf(out, 14), map_buf(out, 15), &info));
  mixing_finish(out, &info);
  UNPROTECT(1);
  return out;
}
/* Posterior predictive checks over recorded samples on the device (bnmf_ppc / bnmf_ppc_at): C_bnmf_ppc(ptr, end_iter (integer, or NULL =
 * the current iteration), n_samples, used (logical length n_samples, or NULL = all), want_cell (logical), dims c(K,G,N)) ->
 * list(n_used, n_tail_cells, p_T1, p_T2, mean_T1_obs, mean_T1_rep, mean_T2_obs, mean_T2_rep, col (G x 6: T1_obs, T1_rep, p_T1, T2_obs,
 * T2_rep, p_T2 per column), series (S x 4: the whole-matrix T1_obs, T1_rep, T2_obs, T2_rep per used sample), mean_cell, var_cell,
 * p_less_cell, p_equal_cell (K x G each, or NULL)) over iterations end_iter - n_samples + 1 ... end_iter.
 * C_bnmf_ppc_at: the same with end_iter required */
/* the result list with col and series allocated, and the flags of used; returned unprotected */
static SEXP ppc_alloc(SEXP n_samples, SEXP used, SEXP dims, int32_t** u) {
  const int n = INTEGER(n_samples)[0], G = INTEGER(dims)[1];
  if (used != R_NilValue && XLENGTH(used) != (R_xlen_t)n) Rf_error("bnmf: used has %ld entries for %d samples", (long)XLENGTH(used), n);
  *u = lgl_flags(used, n);
  int S = n < 0 ? 0 : n;
  if (*u) { S = 0; for (int i = 0; i < n; ++i) S += (*u)[i]; }
  static const char* nms[] = {"n_used", "n_tail_cells", "p_T1", "p_T2", "mean_T1_obs", "mean_T1_rep", "mean_T2_obs", "mean_T2_rep", "col", "series",
                              "mean_cell", "var_cell", "p_less_cell", "p_equal_cell"};
  SEXP out = PROTECT(named_list(14, nms));
  SET_VECTOR_ELT(out, 8, Rf_allocMatrix(REALSXP, G, BNMF_PPC_NCOL));
  SET_VECTOR_ELT(out, 9, Rf_allocMatrix(REALSXP, S, 4));
  UNPROTECT(1);
  return out;
}
static double* ppc_cell_buf(SEXP want_cell, SEXP dims) {
  const int* d = INTEGER(dims);
  return LOGICAL(want_cell)[0] == TRUE ? (double*)R_alloc(4 * (size_t)d[0] * (size_t)d[1], sizeof(double)) : NULL;
}
static void ppc_finish(SEXP out, const double* cell, SEXP dims, const bnmf_ppc_info* info) {
  const int* d = INTEGER(dims); const int K = d[0], G = d[1];
  if (cell) {
    for (int i = 0; i < 4; ++i) {
      SEXP m = Rf_allocMatrix(REALSXP, K, G);
      SET_VECTOR_ELT(out, 10 + i, m);
      for (R_xlen_t j = 0; j < (R_xlen_t)K * G; ++j) REAL(m)[j] = cell[(size_t)i * K * G + (size_t)j];
    }
  }
  SET_VECTOR_ELT(out, 0, Rf_ScalarInteger(info->n_used)); SET_VECTOR_ELT(out, 1, Rf_ScalarReal((double)info->n_tail_cells));
  const double v[6] = {info->p_T1, info->p_T2, info->mean_T1_obs, info->mean_T1_rep, info->mean_T2_obs, info->mean_T2_rep};
  for (int i = 0; i < 6; ++i) SET_VECTOR_ELT(out, 2 + i, Rf_ScalarReal(v[i]));
}
SEXP C_bnmf_ppc(SEXP ptr, SEXP end_iter, SEXP n_samples, SEXP used, SEXP want_cell, SEXP dims) {
  int32_t* u = NULL;
  SEXP out = PROTECT(ppc_alloc(n_samples, used, dims, &u));
  double* cell = ppc_cell_buf(want_cell, dims);
  bnmf_ppc_info info;
  if (end_iter == R_NilValue) chk(bnmf_ppc(get_handle(ptr), INTEGER(n_samples)[0], u, map_buf(out, 8), cell, map_buf(out, 9), &info));
  else chk(bnmf_ppc_at(get_handle(ptr), INTEGER(end_iter)[0], INTEGER(n_samples)[0], u, map_buf(out, 8), cell, map_buf(out, 9), &info));
  ppc_finish(out, cell, dims, &info);
  UNPROTECT(1);
  return out;
}
SEXP C_bnmf_ppc_at(SEXP ptr, SEXP end_iter, SEXP n_samples, SEXP used, SEXP want_cell, SEXP dims) {
  int32_t* u = NULL;
  SEXP out = PROTECT(ppc_alloc(n_samples, used, dims, &u));
  double* cell = ppc_cell_buf(want_cell, dims);
  bnmf_ppc_info info;
  chk(bnmf_ppc_at(get_handle(ptr), INTEGER(end_iter)[0], INTEGER(n_samples)[0], u, map_buf(out, 8), cell, map_buf(out, 9), &info));
  ppc_finish(out, cell, dims, &info);
  UNPROTECT(1);
  return out;
}
/* Signature attribution over recorded samples on the device (bnmf_attribution / bnmf_attribution_at): C_bnmf_attribution(ptr, end_iter
 * (integer, or NULL = the current iteration), n_samples, used (logical length n_samples, or NULL = all), min_load, want_prob (logical),
 * dims c(K,G,N)) -> list(n_used, n_present, min_load, total, load (N G x 4: one column per row of the C output — mean, variance, mean
 * share, probability of presence — each laid out as E), series (N x S: the cohort's load of every signature per used sample), prob
 * (K N x G, laid out as Z: k + K (n + N g); or NULL)) over iterations end_iter - n_samples + 1 ... end_iter.
 * C_bnmf_attribution_at: the same with end_iter required */
/* the result list with load, series and (if wanted) prob allocated, and the flags of used; returned unprotected */
static SEXP attr_alloc(SEXP n_samples, SEXP used, SEXP want_prob, SEXP dims, int32_t** u) {
  const int n = INTEGER(n_samples)[0];
  const int* d = INTEGER(dims);
  if (used != R_NilValue && XLENGTH(used) != (R_xlen_t)n) Rf_error("bnmf: used has %ld entries for %d samples", (long)XLENGTH(used), n);
  *u = lgl_flags(used, n);
  int S = n < 0 ? 0 : n;
  if (*u) { S = 0; for (int i = 0; i < n; ++i) S += (*u)[i]; }
  static const char* nms[] = {"n_used", "n_present", "min_load", "total", "load", "series", "prob"};
  SEXP out = PROTECT(named_list(7, nms));
  SET_VECTOR_ELT(out, 4, Rf_allocMatrix(REALSXP, d[2] * d[1], BNMF_ATTR_NLOAD));
  SET_VECTOR_ELT(out, 5, Rf_allocMatrix(REALSXP, d[2], S));
  if (LOGICAL(want_prob)[0] == TRUE) SET_VECTOR_ELT(out, 6, Rf_allocMatrix(REALSXP, d[0] * d[2], d[1]));
  UNPROTECT(1);
  return out;
}
static void attr_finish(SEXP out, const bnmf_attr_info* info) {
  SET_VECTOR_ELT(out, 0, Rf_ScalarInteger(info->n_used)); SET_VECTOR_ELT(out, 1, Rf_ScalarReal((double)info->n_present));
  SET_VECTOR_ELT(out, 2, Rf_ScalarReal(info->min_load)); SET_VECTOR_ELT(out, 3, Rf_ScalarReal(info->total));
}
SEXP C_bnmf_attribution(SEXP ptr, SEXP end_iter, SEXP n_samples, SEXP used, SEXP min_load, SEXP want_prob, SEXP dims) {
  int32_t* u = NULL;
  SEXP out = PROTECT(attr_alloc(n_samples, used, want_prob, dims, &u));
  bnmf_attr_info info;
  if (end_iter == R_NilValue)
    chk(bnmf_attribution(get_handle(ptr), INTEGER(n_samples)[0], u, REAL(min_load)[0], map_buf(out, 4), map_buf(out, 6), map_buf(out, 5), &info));
  else
    chk(bnmf_attribution_at(get_handle(ptr), INTEGER(end_iter)[0], INTEGER(n_samples)[0], u, REAL(min_load)[0], map_buf(out, 4), map_buf(out, 6),
                            map_buf(out, 5), &info));
  attr_finish(out, &info);
  UNPROTECT(1);
  return out;
}
SEXP C_bnmf_attribution_at(SEXP ptr, SEXP end_iter, SEXP n_samples, SEXP used, SEXP min_load, SEXP want_prob, SEXP dims) {
  int32_t* u = NULL;
  SEXP out = PROTECT(attr_alloc(n_samples, used, want_prob, dims, &u));
  bnmf_attr_info info;
  chk(bnmf_attribution_at(get_handle(ptr), INTEGER(end_iter)[0], INTEGER(n_samples)[0], u, REAL(min_load)[0], map_buf(out, 4), map_buf(out, 6),
                          map_buf(out, 5), &info));
  attr_finish(out, &info);
  UNPROTECT(1);
  return out;
}
/* Reconstruction quality per tumour over recorded samples on the device (bnmf_reconstruction / bnmf_reconstruction_at):
 * C_bnmf_reconstruction(ptr, end_iter (integer, or NULL = the current iteration), n_samples, used (logical length n_samples, or NULL =
 * all), min_cosine, min_drop, dims c(K,G,N)) -> list(n_used, n_undefined, n_poor, n_needed, min_cosine, min_drop, worst_cosine, worst_at
 * (0-based tumour, -1 = none), tumour (G x 6: one column per row of the C output - mean cosine, its variance, smallest cosine, mean
 * relative L1 error, mean RMSE, share of samples with cosine >= min_cosine), drop (N G x 4: mean drop, its variance, mean leave-one-out
 * cosine, share of samples with drop >= min_drop - each laid out as E), series (S: the cohort's mean cosine per used sample), signature
 * (N x 3: tumours that need the signature, mean and largest mean drop)) over iterations end_iter - n_samples + 1 ... end_iter.
 * C_bnmf_reconstruction_at: the same with end_iter required */
/* the result list with its arrays allocated, and the flags of used; returned unprotected */
static SEXP rec_alloc(SEXP n_samples, SEXP used, SEXP dims, int32_t** u) {
  const int n = INTEGER(n_samples)[0];
  const int* d = INTEGER(dims);
  if (used != R_NilValue && XLENGTH(used) != (R_xlen_t)n) Rf_error("bnmf: used has %ld entries for %d samples", (long)XLENGTH(used), n);
  *u = lgl_flags(used, n);
  int S = n < 0 ? 0 : n;
  if (*u) { S = 0; for (int i = 0; i < n; ++i) S += (*u)[i]; }
  static const char* nms[] = {"n_used", "n_undefined", "n_poor", "n_needed", "min_cosine", "min_drop", "worst_cosine", "worst_at", "tumour", "drop",
                              "series", "signature"};
  SEXP out = PROTECT(named_list(12, nms));
  SET_VECTOR_ELT(out, 8, Rf_allocMatrix(REALSXP, d[1], BNMF_REC_NTUM));
  SET_VECTOR_ELT(out, 9, Rf_allocMatrix(REALSXP, d[2] * d[1], BNMF_REC_NDROP));
  SET_VECTOR_ELT(out, 10, Rf_allocVector(REALSXP, S));
  SET_VECTOR_ELT(out, 11, Rf_allocMatrix(REALSXP, d[2], BNMF_REC_NSIG));
  UNPROTECT(1);
  return out;
}
static void rec_finish(SEXP out, const bnmf_reconstruction_info* info) {
  SET_VECTOR_ELT(out, 0, Rf_ScalarInteger(info->n_used)); SET_VECTOR_ELT(out, 1, Rf_ScalarInteger(info->n_undefined));
  SET_VECTOR_ELT(out, 2, Rf_ScalarReal((double)info->n_poor)); SET_VECTOR_ELT(out, 3, Rf_ScalarReal((double)info->n_needed));
  SET_VECTOR_ELT(out, 4, Rf_ScalarReal(info->min_cosine)); SET_VECTOR_ELT(out, 5, Rf_ScalarReal(info->min_drop));
  SET_VECTOR_ELT(out, 6, Rf_ScalarReal(info->worst_cosine)); SET_VECTOR_ELT(out, 7, Rf_ScalarReal((double)info->worst_at));
}
SEXP C_bnmf_reconstruction(SEXP ptr, SEXP end_iter, SEXP n_samples, SEXP used, SEXP min_cosine, SEXP min_drop, SEXP dims) {
  int32_t* u = NULL;
  SEXP out = PROTECT(rec_alloc(n_samples, used, dims, &u));
  bnmf_reconstruction_info info;
  if (end_iter == R_NilValue)
    chk(bnmf_reconstruction(get_handle(ptr), INTEGER(n_samples)[0], u, REAL(min_cosine)[0], REAL(min_drop)[0], map_buf(out, 8), map_buf(out, 9), map_buf(out, 10),
                            map_buf(out, 11), &info));
  else
    chk(bnmf_reconstruction_at(get_handle(ptr), INTEGER(end_iter)[0], INTEGER(n_samples)[0], u, REAL(min_cosine)[0], REAL(min_drop)[0], map_buf(out, 8),
                               map_buf(out, 9), map_buf(out, 10), map_buf(out, 11), &info));
  rec_finish(out, &info);
  UNPROTECT(1);
  return out;
}
SEXP C_bnmf_reconstruction_at(SEXP ptr, SEXP end_iter, SEXP n_samples, SEXP used, SEXP min_cosine, SEXP min_drop, SEXP dims) {
  int32_t* u = NULL;
  SEXP out = PROTECT(rec_alloc(n_samples, used, dims, &u));
  bnmf_reconstruction_info info;
  chk(bnmf_reconstruction_at(get_handle(ptr), INTEGER(end_iter)[0], INTEGER(n_samples)[0], u, REAL(min_cosine)[0], REAL(min_drop)[0], map_buf(out, 8),
                             map_buf(out, 9), map_buf(out, 10), map_buf(out, 11), &info));
  rec_finish(out, &info);
  UNPROTECT(1);
  return out;
}
/* Group contrasts of exposures over recorded samples on the device (bnmf_contrast / bnmf_contrast_at): C_bnmf_contrast(ptr, end_iter
 * (integer, or NULL = the current iteration), n_samples, used (logical length n_samples, or NULL = all), groups (integer length G: the
 * 0-based label of every tumour, -1 or NA = left out), min_load, credible_interval (<= 0: no interval), want_series (logical),
 * dims c(K,G,N)) -> list(n_used, n_groups, n_pairs, n_left_out, n_credible (3: load, share, prevalence), min_load, credible_interval,
 * sizes (C), group (N C x 12: column 4 q + i = row i — mean, variance, lower, upper — of statistic q, each laid out n + N c), pair
 * (N NP x 18: column 6 q + i = row i — mean, variance, lower, upper, p_greater, p_less — of statistic q, each laid out n + N p; NULL
 * with one group), series (N C x 3 S: column S q + s; or NULL)) over iterations end_iter - n_samples + 1 ... end_iter.
 * C_bnmf_contrast_at: the same with end_iter required */
/* the result list with sizes, group, pair and (if wanted) series allocated, the flags of used and the labels; returned unprotected */
static SEXP con_alloc(SEXP n_samples, SEXP used, SEXP groups, SEXP want_series, SEXP dims, int32_t** u, int32_t** lab) {
  const int n = INTEGER(n_samples)[0];
  const int* d = INTEGER(dims);
  const int G = d[1], N = d[2];
  if (used != R_NilValue && XLENGTH(used) != (R_xlen_t)n) Rf_error("bnmf: used has %ld entries for %d samples", (long)XLENGTH(used), n);
  if (XLENGTH(groups) != (R_xlen_t)G) Rf_error("bnmf: groups has %ld labels for %d tumours", (long)XLENGTH(groups), G);
  *u = lgl_flags(used, n);
  int S = n < 0 ? 0 : n;
  if (*u) { S = 0; for (int i = 0; i < n; ++i) S += (*u)[i]; }
  int32_t* l = (int32_t*)R_alloc(G, sizeof(int32_t));
  int C = 1;                                                              /* (a label the library refuses sizes nothing) */
  for (int g = 0; g < G; ++g) {
    const int v = INTEGER(groups)[g];
    l[g] = v == NA_INTEGER ? -1 : v;
    if (l[g] >= C && l[g] < BNMF_CON_MAX_GROUPS) C = l[g] + 1;
  }
  *lab = l;
  const int NP = C * (C - 1) / 2;
  static const char* nms[] = {"n_used", "n_groups", "n_pairs", "n_left_out", "n_credible", "min_load", "credible_interval", "sizes", "group", "pair", "series"};
  SEXP out = PROTECT(named_list(11, nms));
  SET_VECTOR_ELT(out, 7, Rf_allocVector(INTSXP, C));
  SET_VECTOR_ELT(out, 8, Rf_allocMatrix(REALSXP, N * C, BNMF_CON_NSTAT * BNMF_CON_NGROW));
  if (NP > 0) SET_VECTOR_ELT(out, 9, Rf_allocMatrix(REALSXP, N * NP, BNMF_CON_NSTAT * BNMF_CON_NPROW));
  if (LOGICAL(want_series)[0] == TRUE) SET_VECTOR_ELT(out, 10, Rf_allocMatrix(REALSXP, N * C, BNMF_CON_NSTAT * S));
  UNPROTECT(1);
  return out;
}
static void con_finish(SEXP out, const bnmf_contrast_info* info) {
  SET_VECTOR_ELT(out, 0, Rf_ScalarInteger(info->n_used)); SET_VECTOR_ELT(out, 1, Rf_ScalarInteger(info->n_groups));
  SET_VECTOR_ELT(out, 2, Rf_ScalarInteger(info->n_pairs)); SET_VECTOR_ELT(out, 3, Rf_ScalarInteger(info->n_left_out));
  SEXP nc = PROTECT(Rf_allocVector(REALSXP, BNMF_CON_NSTAT));
  for (int q = 0; q < BNMF_CON_NSTAT; ++q) REAL(nc)[q] = (double)info->n_credible[q];
  SET_VECTOR_ELT(out, 4, nc);
  UNPROTECT(1);
  SET_VECTOR_ELT(out, 5, Rf_ScalarReal(info->min_load)); SET_VECTOR_ELT(out, 6, Rf_ScalarReal(info->credible_interval));
}
SEXP C_bnmf_contrast(SEXP ptr, SEXP end_iter, SEXP n_samples, SEXP used, SEXP groups, SEXP min_load, SEXP ci, SEXP want_series, SEXP dims) {
  int32_t *u = NULL, *lab = NULL;
  SEXP out = PROTECT(con_alloc(n_samples, used, groups, want_series, dims, &u, &lab));
  bnmf_contrast_info info;
  if (end_iter == R_NilValue)
    chk(bnmf_contrast(get_handle(ptr), INTEGER(n_samples)[0], u, lab, REAL(min_load)[0], REAL(ci)[0], map_buf(out, 8), map_buf(out, 9), map_buf(out, 10),
                      INTEGER(VECTOR_ELT(out, 7)), &info));
  else
    chk(bnmf_contrast_at(get_handle(ptr), INTEGER(end_iter)[0], INTEGER(n_samples)[0], u, lab, REAL(min_load)[0], REAL(ci)[0], map_buf(out, 8),
                         map_buf(out, 9), map_buf(out, 10), INTEGER(VECTOR_ELT(out, 7)), &info));
  con_finish(out, &info);
  UNPROTECT(1);
  return out;
}
SEXP C_bnmf_contrast_at(SEXP ptr, SEXP end_iter, SEXP n_samples, SEXP used, SEXP groups, SEXP min_load, SEXP ci, SEXP want_series, SEXP dims) {
  int32_t *u = NULL, *lab = NULL;
  SEXP out = PROTECT(con_alloc(n_samples, used, groups, want_series, dims, &u, &lab));
  bnmf_contrast_info info;
  chk(bnmf_contrast_at(get_handle(ptr), INTEGER(end_iter)[0], INTEGER(n_samples)[0], u, lab, REAL(min_load)[0], REAL(ci)[0], map_buf(out, 8),
                       map_buf(out, 9), map_buf(out, 10), INTEGER(VECTOR_ELT(out, 7)), &info));
  con_finish(out, &info);
  UNPROTECT(1);
  return out;
}
/* Regression of exposures on tumour covariates over recorded samples on the device (bnmf_regress / bnmf_regress_at): C_bnmf_regress(ptr,
 * end_iter (integer, or NULL = the current iteration), n_samples, used (logical length n_samples, or NULL = all), design (G x Q real
 * matrix, taken as given: the caller supplies the column of ones), include (logical length G, or NULL = all), credible_interval (<= 0: no
 * interval), want_series (logical), dims c(K,G,N)) -> list(n_used, Q, n_included, n_left_out, n_blocks, min_pivot_at (0-based column),
 * n_credible (Q x 3: column q = response q), credible_interval, min_pivot_ratio, coef (N Q x 18: column 6 q + i = row i — mean, variance,
 * lower, upper, p_greater, p_less — of response q, each laid out n + N j), fit (N x 15: column 5 q + i = row i — mean r2, lower r2, upper
 * r2, samples with an r2, mean sigma2), coef_series (N Q x 3 S: column S q + s; or NULL), r2_series (N x 3 S; or NULL)) over iterations
 * end_iter - n_samples + 1 ... end_iter.  C_bnmf_regress_at: the same with end_iter required */
/* the result list with coef, fit and (if wanted) the series allocated, the flags of used and include; returned unprotected */
static SEXP reg_alloc(SEXP n_samples, SEXP used, SEXP design, SEXP include, SEXP want_series, SEXP dims, int32_t** u, int32_t** inc, int* Q) {
  const int n = INTEGER(n_samples)[0];
  const int* d = INTEGER(dims);
  const int G = d[1], N = d[2];
  if (used != R_NilValue && XLENGTH(used) != (R_xlen_t)n) Rf_error("bnmf: used has %ld entries for %d samples", (long)XLENGTH(used), n);
  if (Rf_nrows(design) != G) Rf_error("bnmf: design has %d rows for %d tumours", Rf_nrows(design), G);
  if (include != R_NilValue && XLENGTH(include) != (R_xlen_t)G) Rf_error("bnmf: include has %ld flags for %d tumours", (long)XLENGTH(include), G);
  *u = lgl_flags(used, n);
  *inc = lgl_flags(include, G);
  *Q = Rf_ncols(design);
  int S = n < 0 ? 0 : n;
  if (*u) { S = 0; for (int i = 0; i < n; ++i) S += (*u)[i]; }
  static const char* nms[] = {"n_used", "Q", "n_included", "n_left_out", "n_blocks", "min_pivot_at", "n_credible", "credible_interval", "min_pivot_ratio",
                              "coef", "fit", "coef_series", "r2_series"};
  SEXP out = PROTECT(named_list(13, nms));
  SET_VECTOR_ELT(out, 9, Rf_allocMatrix(REALSXP, N * *Q, BNMF_REG_NSTAT * BNMF_REG_NCROW));
  SET_VECTOR_ELT(out, 10, Rf_allocMatrix(REALSXP, N, BNMF_REG_NSTAT * BNMF_REG_NFIT));
  if (LOGICAL(want_series)[0] == TRUE) {
    SET_VECTOR_ELT(out, 11, Rf_allocMatrix(REALSXP, N * *Q, BNMF_REG_NSTAT * S));
    SET_VECTOR_ELT(out, 12, Rf_allocMatrix(REALSXP, N, BNMF_REG_NSTAT * S));
  }
  UNPROTECT(1);
  return out;
}
static void reg_finish(SEXP out, const bnmf_regress_info* info) {
  SET_VECTOR_ELT(out, 0, Rf_ScalarInteger(info->n_used)); SET_VECTOR_ELT(out, 1, Rf_ScalarInteger(info->Q));
  SET_VECTOR_ELT(out, 2, Rf_ScalarInteger(info->n_included)); SET_VECTOR_ELT(out, 3, Rf_ScalarInteger(info->n_left_out));
  SET_VECTOR_ELT(out, 4, Rf_ScalarInteger(info->n_blocks)); SET_VECTOR_ELT(out, 5, Rf_ScalarInteger(info->min_pivot_at));
  SEXP nc = PROTECT(Rf_allocMatrix(REALSXP, info->Q, BNMF_REG_NSTAT));
  for (int q = 0; q < BNMF_REG_NSTAT; ++q) for (int j = 0; j < info->Q; ++j) REAL(nc)[j + info->Q * q] = (double)info->n_credible[q][j];
  SET_VECTOR_ELT(out, 6, nc);
  UNPROTECT(1);
  SET_VECTOR_ELT(out, 7, Rf_ScalarReal(info->credible_interval)); SET_VECTOR_ELT(out, 8, Rf_ScalarReal(info->min_pivot_ratio));
}
SEXP C_bnmf_regress(SEXP ptr, SEXP end_iter, SEXP n_samples, SEXP used, SEXP design, SEXP include, SEXP ci, SEXP want_series, SEXP dims) {
  int32_t *u = NULL, *inc = NULL; int Q = 0;
  SEXP out = PROTECT(reg_alloc(n_samples, used, design, include, want_series, dims, &u, &inc, &Q));
  bnmf_regress_info info;
  if (end_iter == R_NilValue)
    chk(bnmf_regress(get_handle(ptr), INTEGER(n_samples)[0], u, REAL(design), Q, inc, REAL(ci)[0], map_buf(out, 9), map_buf(out, 10), map_buf(out, 11),
                     map_buf(out, 12), &info));
  else
    chk(bnmf_regress_at(get_handle(ptr), INTEGER(end_iter)[0], INTEGER(n_samples)[0], u, REAL(design), Q, inc, REAL(ci)[0], map_buf(out, 9),
                        map_buf(out, 10), map_buf(out, 11), map_buf(out, 12), &info));
  reg_finish(out, &info);
  UNPROTECT(1);
  return out;
}
SEXP C_bnmf_regress_at(SEXP ptr, SEXP end_iter, SEXP n_samples, SEXP used, SEXP design, SEXP include, SEXP ci, SEXP want_series, SEXP dims) {
  int32_t *u = NULL, *inc = NULL; int Q = 0;
  SEXP out = PROTECT(reg_alloc(n_samples, used, design, include, want_series, dims, &u, &inc, &Q));
  bnmf_regress_info info;
  chk(bnmf_regress_at(get_handle(ptr), INTEGER(end_iter)[0], INTEGER(n_samples)[0], u, REAL(design), Q, inc, REAL(ci)[0], map_buf(out, 9),
                      map_buf(out, 10), map_buf(out, 11), map_buf(out, 12), &info));
  reg_finish(out, &info);
  UNPROTECT(1);
  return out;
}
/* Co-activity of signatures over recorded samples on the device (bnmf_coactivity / bnmf_coactivity_at): C_bnmf_coactivity(ptr, end_iter
 * (integer, or NULL = the current iteration), n_samples, used (logical length n_samples, or NULL = all), include (logical length G, or
 * NULL = all), min_load, credible_interval (<= 0: no interval), want_series (logical), dims c(K,G,N)) -> list(n_used, n_included,
 * n_left_out, n_pairs, n_blocks, n_credible (3: pearson, spearman, co-presence), max_cosine_at (0-based pair, -1 = none), max_cosine,
 * min_load, credible_interval, pair (NP x 28: column 7 q + i = row i — mean, variance, lower, upper, p_greater, p_less, n_valid — of
 * statistic q; the pairs a < b numbered with a ascending, then b), series (NP x 4 S: column S q + s; or NULL)) over iterations
 * end_iter - n_samples + 1 ... end_iter.  C_bnmf_coactivity_at: the same with end_iter required */
/* the result list with pair and (if wanted) series allocated, the flags of used and include; returned unprotected */
static SEXP coa_alloc(SEXP n_samples, SEXP used, SEXP include, SEXP want_series, SEXP dims, int32_t** u, int32_t** inc) {
  const int n = INTEGER(n_samples)[0];
  const int* d = INTEGER(dims);
  const int G = d[1], N = d[2], NP = N * (N - 1) / 2;
  if (used != R_NilValue && XLENGTH(used) != (R_xlen_t)n) Rf_error("bnmf: used has %ld entries for %d samples", (long)XLENGTH(used), n);
  if (include != R_NilValue && XLENGTH(include) != (R_xlen_t)G) Rf_error("bnmf: include has %ld flags for %d tumours", (long)XLENGTH(include), G);
  *u = lgl_flags(used, n);
  *inc = lgl_flags(include, G);
  int S = n < 0 ? 0 : n;
  if (*u) { S = 0; for (int i = 0; i < n; ++i) S += (*u)[i]; }
  static const char* nms[] = {"n_used", "n_included", "n_left_out", "n_pairs", "n_blocks", "n_credible", "max_cosine_at", "max_cosine", "min_load",
                              "credible_interval", "pair", "series"};
  SEXP out = PROTECT(named_list(12, nms));
  SET_VECTOR_ELT(out, 10, Rf_allocMatrix(REALSXP, NP, BNMF_COA_NSTAT * BNMF_COA_NPROW));
  if (LOGICAL(want_series)[0] == TRUE) SET_VECTOR_ELT(out, 11, Rf_allocMatrix(REALSXP, NP, BNMF_COA_NSTAT * S));
  UNPROTECT(1);
  return out;
}
static void coa_finish(SEXP out, const bnmf_coactivity_info* info) {
  SET_VECTOR_ELT(out, 0, Rf_ScalarInteger(info->n_used)); SET_VECTOR_ELT(out, 1, Rf_ScalarInteger(info->n_included));
  SET_VECTOR_ELT(out, 2, Rf_ScalarInteger(info->n_left_out)); SET_VECTOR_ELT(out, 3, Rf_ScalarInteger(info->n_pairs));
  SET_VECTOR_ELT(out, 4, Rf_ScalarInteger(info->n_blocks));
  SEXP nc = PROTECT(Rf_allocVector(REALSXP, 3));
  for (int q = 0; q < 3; ++q) REAL(nc)[q] = (double)info->n_credible[q];
  SET_VECTOR_ELT(out, 5, nc);
  UNPROTECT(1);
  SET_VECTOR_ELT(out, 6, Rf_ScalarInteger((int)info->max_cosine_at)); SET_VECTOR_ELT(out, 7, Rf_ScalarReal(info->max_cosine));
  SET_VECTOR_ELT(out, 8, Rf_ScalarReal(info->min_load)); SET_VECTOR_ELT(out, 9, Rf_ScalarReal(info->credible_interval));
}
SEXP C_bnmf_coactivity(SEXP ptr, SEXP end_iter, SEXP n_samples, SEXP used, SEXP include, SEXP min_load, SEXP ci, SEXP want_series, SEXP dims) {
  int32_t *u = NULL, *inc = NULL;
  SEXP out = PROTECT(coa_alloc(n_samples, used, include, want_series, dims, &u, &inc));
  bnmf_coactivity_info info;
  if (end_iter == R_NilValue)
    chk(bnmf_coactivity(get_handle(ptr), INTEGER(n_samples)[0], u, inc, REAL(min_load)[0], REAL(ci)[0], map_buf(out, 10), map_buf(out, 11), &info));
  else
    chk(bnmf_coactivity_at(get_handle(ptr), INTEGER(end_iter)[0], INTEGER(n_samples)[0], u, inc, REAL(min_load)[0], REAL(ci)[0], map_buf(out, 10),
                           map_buf(out, 11), &info));
  coa_finish(out, &info);
  UNPROTECT(1);
  return out;
}
SEXP C_bnmf_coactivity_at(SEXP ptr, SEXP end_iter, SEXP n_samples, SEXP used, SEXP include, SEXP min_load, SEXP ci, SEXP want_series, SEXP dims) {
  int32_t *u = NULL, *inc = NULL;
  SEXP out = PROTECT(coa_alloc(n_samples, used, include, want_series, dims, &u, &inc));
  bnmf_coactivity_info info;
  chk(bnmf_coactivity_at(get_handle(ptr), INTEGER(end_iter)[0], INTEGER(n_samples)[0], u, inc, REAL(min_load)[0], REAL(ci)[0], map_buf(out, 10),
                         map_buf(out, 11), &info));
  coa_finish(out, &info);
  UNPROTECT(1);
  return out;
}
/* Similarity of tumours over recorded samples on the device (bnmf_similarity / bnmf_similarity_at): C_bnmf_similarity(ptr, end_iter
 * (integer, or NULL = the current iteration), n_samples, used (logical length n_samples, or NULL = all), include (logical length G, or
 * NULL = all), query (integer, 0-based tumours; or NULL), opts (integer c(top_k, want_tumour 0 / 1)), min_cosine, dims c(K,G,N)) -> list(n_used,
 * n_included, n_left_out, top_k, n_query, n_pairs, n_similar_pairs, n_isolated, least_typical_at (0-based tumour, -1 = none),
 * mean_similarity, least_typical, min_cosine, neighbour_at (top_k x G integer: column g holds the 0-based neighbours of tumour g, -1 =
 * none; NULL with top_k = 0), neighbour (top_k G x 3: one column per row of the C output - mean, variance, p_similar - each laid out as
 * neighbour_at; or NULL), dense (G Q x 3: column r laid out as a G x Q matrix, one column per query; NULL without a query), tumour (G x 3:
 * typicality, the first neighbour's mean, degree; NULL unless want_tumour is 1)) over iterations end_iter - n_samples + 1 ... end_iter.  With
 * opts = c(0, 0) and a query only the queries' rows are computed.  C_bnmf_similarity_at: the same with end_iter required */
/* the result list with its arrays allocated, the flags of used and include, the queries; returned unprotected */
static SEXP sim_alloc(SEXP n_samples, SEXP used, SEXP include, SEXP query, SEXP opts, SEXP dims, int32_t** u, int32_t** inc,
                      int32_t** q, int* Q) {
  const int n = INTEGER(n_samples)[0], G = INTEGER(dims)[1];
  if (XLENGTH(opts) != 2) Rf_error("bnmf: opts has %ld entries, c(top_k, want_tumour) is needed", (long)XLENGTH(opts));
  int k = INTEGER(opts)[0];
  if (used != R_NilValue && XLENGTH(used) != (R_xlen_t)n) Rf_error("bnmf: used has %ld entries for %d samples", (long)XLENGTH(used), n);
  if (include != R_NilValue && XLENGTH(include) != (R_xlen_t)G) Rf_error("bnmf: include has %ld flags for %d tumours", (long)XLENGTH(include), G);
  *u = lgl_flags(used, n);
  *inc = lgl_flags(include, G);
  *Q = query == R_NilValue ? 0 : (int)XLENGTH(query);
  *q = *Q > 0 ? (int32_t*)INTEGER(query) : NULL;
  if (k < 0 || k > BNMF_SIM_MAX_K) k = 0;                                  /* (the library refuses it: nothing to allocate) */
  static const char* nms[] = {"n_used", "n_included", "n_left_out", "top_k", "n_query", "n_pairs", "n_similar_pairs", "n_isolated", "least_typical_at",
                              "mean_similarity", "least_typical", "min_cosine", "neighbour_at", "neighbour", "dense", "tumour"};
  SEXP out = PROTECT(named_list(16, nms));
  if (k > 0) {
    SET_VECTOR_ELT(out, 12, Rf_allocMatrix(INTSXP, k, G));
    SET_VECTOR_ELT(out, 13, Rf_allocMatrix(REALSXP, k * G, BNMF_SIM_NNROW));
  }
  if (*Q > 0) SET_VECTOR_ELT(out, 14, Rf_allocMatrix(REALSXP, G * *Q, BNMF_SIM_NDROW));
  if (INTEGER(opts)[1] == 1) SET_VECTOR_ELT(out, 15, Rf_allocMatrix(REALSXP, G, BNMF_SIM_NTUM));
  UNPROTECT(1);
  return out;
}
static int32_t* sim_at_buf(SEXP out) { SEXP x = VECTOR_ELT(out, 12); return x == R_NilValue ? NULL : (int32_t*)INTEGER(x); }
static void sim_finish(SEXP out, const bnmf_similarity_info* info) {
  SET_VECTOR_ELT(out, 0, Rf_ScalarInteger(info->n_used)); SET_VECTOR_ELT(out, 1, Rf_ScalarInteger(info->n_included));
  SET_VECTOR_ELT(out, 2, Rf_ScalarInteger(info->n_left_out)); SET_VECTOR_ELT(out, 3, Rf_ScalarInteger(info->top_k));
  SET_VECTOR_ELT(out, 4, Rf_ScalarInteger(info->n_query)); SET_VECTOR_ELT(out, 5, Rf_ScalarReal((double)info->n_pairs));
  SET_VECTOR_ELT(out, 6, Rf_ScalarReal((double)info->n_similar_pairs)); SET_VECTOR_ELT(out, 7, Rf_ScalarReal((double)info->n_isolated));
  SET_VECTOR_ELT(out, 8, Rf_ScalarReal((double)info->least_typical_at)); SET_VECTOR_ELT(out, 9, Rf_ScalarReal(info->mean_similarity));
  SET_VECTOR_ELT(out, 10, Rf_ScalarReal(info->least_typical)); SET_VECTOR_ELT(out, 11, Rf_ScalarReal(info->min_cosine));
}
SEXP C_bnmf_similarity(SEXP ptr, SEXP end_iter, SEXP n_samples, SEXP used, SEXP include, SEXP query, SEXP opts, SEXP min_cosine, SEXP dims) {
  int32_t *u = NULL, *inc = NULL, *q = NULL; int Q = 0;
  SEXP out = PROTECT(sim_alloc(n_samples, used, include, query, opts, dims, &u, &inc, &q, &Q));
  bnmf_similarity_info info;
  if (end_iter == R_NilValue)
    chk(bnmf_similarity(get_handle(ptr), INTEGER(n_samples)[0], u, inc, q, Q, INTEGER(opts)[0], REAL(min_cosine)[0], sim_at_buf(out), map_buf(out, 13),
                        map_buf(out, 14), map_buf(out, 15), &info));
  else
    chk(bnmf_similarity_at(get_handle(ptr), INTEGER(end_iter)[0], INTEGER(n_samples)[0], u, inc, q, Q, INTEGER(opts)[0], REAL(min_cosine)[0], sim_at_buf(out),
                           map_buf(out, 13), map_buf(out, 14), map_buf(out, 15), &info));
  sim_finish(out, &info);
  UNPROTECT(1);
  return out;
}
SEXP C_bnmf_similarity_at(SEXP ptr, SEXP end_iter, SEXP n_samples, SEXP used, SEXP include, SEXP query, SEXP opts, SEXP min_cosine, SEXP dims) {
  int32_t *u = NULL, *inc = NULL, *q = NULL; int Q = 0;
  SEXP out = PROTECT(sim_alloc(n_samples, used, include, query, opts, dims, &u, &inc, &q, &Q));
  bnmf_similarity_info info;
  chk(bnmf_similarity_at(get_handle(ptr), INTEGER(end_iter)[0], INTEGER(n_samples)[0], u, inc, q, Q, INTEGER(opts)[0], REAL(min_cosine)[0], sim_at_buf(out),
                         map_buf(out, 13), map_buf(out, 14), map_buf(out, 15), &info));
  sim_finish(out, &info);
  UNPROTECT(1);
  return out;
}
/* Subtypes of tumours over recorded samples on the device (bnmf_subtypes / bnmf_subtypes_at): C_bnmf_subtypes(ptr, end_iter (integer, or
 * NULL = the current iteration), n_samples, used (logical length n_samples, or NULL = all), include (logical length G, or NULL = all),
 * perm (integer n_samples x N matrix of 0-based places, a row of -1 / NA = the sample is unmatched; or NULL = identity), centres0 (N x C
 * real matrix), query (integer, 0-based tumours; or NULL), opts (real c(n_steps, min_certainty, want_labels 0 / 1, K, G, N))) ->
 * list(n_used, n_matched, n_unmatched, n_included, n_left_out, C, n_steps, n_query, n_not_converged, n_certain, n_never_assigned,
 * smallest_subtype_at (0-based), least_certain_at (0-based tumour, -1 = none), mean_certainty, least_certain, smallest_subtype,
 * min_certainty, membership (G x C), label (integer G, 0-based, -1 = none), tumour (G x 3: certainty, share of samples assigned,
 * runner-up), centre (N C x 4: mean, variance, lower, upper at 0.95, row j + N c), size (C x 4), together (G x Q; NULL without a
 * query), labels (G x S integer, -1 unassigned, -2 left out or unmatched; NULL unless want_labels is 1), series (S x 3: inertia, steps,
 * assigned tumours)) over iterations end_iter - n_samples + 1 ... end_iter.  C_bnmf_subtypes_at: the same with end_iter required */
/* the result list with its arrays allocated and the inputs converted; returned unprotected */
typedef struct { int32_t *u, *inc, *perm, *q; int Q, C, n_steps; double min_certainty; } sub_in;
static SEXP sub_alloc(SEXP n_samples, SEXP used, SEXP include, SEXP perm, SEXP centres0, SEXP query, SEXP opts, sub_in* in) {
  const int n = INTEGER(n_samples)[0];
  if (XLENGTH(opts) != 6) Rf_error("bnmf: opts has %ld entries, c(n_steps, min_certainty, want_labels, K, G, N) is needed", (long)XLENGTH(opts));
  const double* o = REAL(opts);
  const int G = (int)o[4], N = (int)o[5];
  if (used != R_NilValue && XLENGTH(used) != (R_xlen_t)n) Rf_error("bnmf: used has %ld entries for %d samples", (long)XLENGTH(used), n);
  if (include != R_NilValue && XLENGTH(include) != (R_xlen_t)G) Rf_error("bnmf: include has %ld flags for %d tumours", (long)XLENGTH(include), G);
  if (perm != R_NilValue && XLENGTH(perm) != (R_xlen_t)n * N) Rf_error("bnmf: perm has %ld entries for %d samples of %d factors", (long)XLENGTH(perm), n, N);
  if (N < 1 || XLENGTH(centres0) < (R_xlen_t)N || XLENGTH(centres0) % N != 0)
    Rf_error("bnmf: centres0 has %ld entries, whole columns of N = %d are needed", (long)XLENGTH(centres0), N);
  in->u = lgl_flags(used, n);
  in->inc = lgl_flags(include, G);
  in->perm = NULL;
  if (perm != R_NilValue) {                                                /* the R matrix is column-major: row s of the ABI is its row s */
    in->perm = (int32_t*)R_alloc((size_t)n * N, sizeof(int32_t));
    for (int s = 0; s < n; ++s) for (int j = 0; j < N; ++j) { const int v = INTEGER(perm)[s + (size_t)n * j]; in->perm[(size_t)s * N + j] = v == NA_INTEGER ? -1 : v; }
  }
  in->Q = query == R_NilValue ? 0 : (int)XLENGTH(query);
  in->q = in->Q > 0 ? (int32_t*)INTEGER(query) : NULL;
  in->C = (int)(XLENGTH(centres0) / N); in->n_steps = (int)o[0]; in->min_certainty = o[1];
  int S = n < 0 ? 0 : n;
  if (in->u) { S = 0; for (int i = 0; i < n; ++i) S += in->u[i]; }
  const int Cb = in->C > BNMF_SUB_MAX_C ? BNMF_SUB_MAX_C : in->C;          /* (the library refuses a larger C: the buffers only have to exist) */
  static const char* nms[] = {"n_used", "n_matched", "n_unmatched", "n_included", "n_left_out", "C", "n_steps", "n_query", "n_not_converged", "n_certain",
                              "n_never_assigned", "smallest_subtype_at", "least_certain_at", "mean_certainty", "least_certain", "smallest_subtype",
                              "min_certainty", "membership", "label", "tumour", "centre", "size", "together", "labels", "series"};
  SEXP out = PROTECT(named_list(25, nms));
  SET_VECTOR_ELT(out, 17, Rf_allocMatrix(REALSXP, G, Cb));
  SET_VECTOR_ELT(out, 18, Rf_allocVector(INTSXP, G));
  SET_VECTOR_ELT(out, 19, Rf_allocMatrix(REALSXP, G, BNMF_SUB_NTUM));
  SET_VECTOR_ELT(out, 20, Rf_allocMatrix(REALSXP, N * Cb, BNMF_SUB_NCROW));
  SET_VECTOR_ELT(out, 21, Rf_allocMatrix(REALSXP, Cb, BNMF_SUB_NCROW));
  if (in->Q > 0) SET_VECTOR_ELT(out, 22, Rf_allocMatrix(REALSXP, G, in->Q));
  if (o[2] == 1.0) SET_VECTOR_ELT(out, 23, Rf_allocMatrix(INTSXP, G, S));
  SET_VECTOR_ELT(out, 24, Rf_allocMatrix(REALSXP, S, BNMF_SUB_NSER));
  UNPROTECT(1);
  return out;
}
static int32_t* sub_int_buf(SEXP out, int i) { SEXP x = VECTOR_ELT(out, i); return x == R_NilValue ? NULL : (int32_t*)INTEGER(x); }
static void sub_finish(SEXP out, const bnmf_subtypes_info* info) {
  const int32_t v[12] = {info->n_used, info->n_matched, info->n_unmatched, info->n_included, info->n_left_out, info->C, info->n_steps, info->n_query,
                         info->n_not_converged, info->n_certain, info->n_never_assigned, info->smallest_subtype_at};
  for (int i = 0; i < 12; ++i) SET_VECTOR_ELT(out, i, Rf_ScalarInteger(v[i]));
  SET_VECTOR_ELT(out, 12, Rf_ScalarReal((double)info->least_certain_at)); SET_VECTOR_ELT(out, 13, Rf_ScalarReal(info->mean_certainty));
  SET_VECTOR_ELT(out, 14, Rf_ScalarReal(info->least_certain)); SET_VECTOR_ELT(out, 15, Rf_ScalarReal(info->smallest_subtype));
  SET_VECTOR_ELT(out, 16, Rf_ScalarReal(info->min_certainty));
}
SEXP C_bnmf_subtypes(SEXP ptr, SEXP end_iter, SEXP n_samples, SEXP used, SEXP include, SEXP perm, SEXP centres0, SEXP query, SEXP opts) {
  sub_in in;
  SEXP out = PROTECT(sub_alloc(n_samples, used, include, perm, centres0, query, opts, &in));
  bnmf_subtypes_info info;
  if (end_iter == R_NilValue)
    chk(bnmf_subtypes(get_handle(ptr), INTEGER(n_samples)[0], in.u, in.inc, in.perm, REAL(centres0), in.C, in.n_steps, in.q, in.Q, in.min_certainty,
                      map_buf(out, 17), sub_int_buf(out, 18), map_buf(out, 19), map_buf(out, 20), map_buf(out, 21), map_buf(out, 22), sub_int_buf(out, 23),
                      map_buf(out, 24), &info));
  else
    chk(bnmf_subtypes_at(get_handle(ptr), INTEGER(end_iter)[0], INTEGER(n_samples)[0], in.u, in.inc, in.perm, REAL(centres0), in.C, in.n_steps, in.q, in.Q,
                         in.min_certainty, map_buf(out, 17), sub_int_buf(out, 18), map_buf(out, 19), map_buf(out, 20), map_buf(out, 21), map_buf(out, 22),
                         sub_int_buf(out, 23), map_buf(out, 24), &info));
  sub_finish(out, &info);
  UNPROTECT(1);
  return out;
}
SEXP C_bnmf_subtypes_at(SEXP ptr, SEXP end_iter, SEXP n_samples, SEXP used, SEXP include, SEXP perm, SEXP centres0, SEXP query, SEXP opts) {
  sub_in in;
  SEXP out = PROTECT(sub_alloc(n_samples, used, include, perm, centres0, query, opts, &in));
  bnmf_subtypes_info info;
  chk(bnmf_subtypes_at(get_handle(ptr), INTEGER(end_iter)[0], INTEGER(n_samples)[0], in.u, in.inc, in.perm, REAL(centres0), in.C, in.n_steps, in.q, in.Q,
                       in.min_certainty, map_buf(out, 17), sub_int_buf(out, 18), map_buf(out, 19), map_buf(out, 20), map_buf(out, 21), map_buf(out, 22),
                       sub_int_buf(out, 23), map_buf(out, 24), &info));
  sub_finish(out, &info);
  UNPROTECT(1);
  return out;
}
/* Residual structure of recorded samples on the device (bnmf_residuals / bnmf_residuals_at): C_bnmf_residuals(ptr, end_iter (integer, or
 * NULL = the current iteration), n_samples, used (logical length n_samples, or NULL = all), include (logical length G, or NULL = all),
 * opts (real c(n_steps, max_dispersion, K, G))) -> list(n_used, n_flat, n_included, n_left_out, n_steps, n_biased, n_overdispersed,
 * worst_type_at (0-based), min_agreement_at (0-based used sample, -1 = none), lambda, share, move, mean_share, min_agreement, worst_type,
 * max_dispersion, gram (K x K), type (K x 5: mean and variance of b, share of b > 0, mean and variance of q), component (K x 4: vbar,
 * mean, variance and share > 0 of the aligned v_s), tumour (G x 3: mean and variance of the aligned score, mean chi), series (S x 5:
 * trace, lambda, share, move, agreement)) over iterations end_iter - n_samples + 1 ... end_iter.  C_bnmf_residuals_at: the same with
 * end_iter required */
/* the result list with its arrays allocated and the flags converted; returned unprotected */
static SEXP res_alloc(SEXP n_samples, SEXP used, SEXP include, SEXP opts, int32_t** u, int32_t** inc) {
  const int n = INTEGER(n_samples)[0];
  if (XLENGTH(opts) != 4) Rf_error("bnmf: opts has %ld entries, c(n_steps, max_dispersion, K, G) is needed", (long)XLENGTH(opts));
  const int K = (int)REAL(opts)[2], G = (int)REAL(opts)[3];
  if (used != R_NilValue && XLENGTH(used) != (R_xlen_t)n) Rf_error("bnmf: used has %ld entries for %d samples", (long)XLENGTH(used), n);
  if (include != R_NilValue && XLENGTH(include) != (R_xlen_t)G) Rf_error("bnmf: include has %ld flags for %d tumours", (long)XLENGTH(include), G);
  *u = lgl_flags(used, n);
  *inc = lgl_flags(include, G);
  int S = n < 0 ? 0 : n;
  if (*u) { S = 0; for (int i = 0; i < n; ++i) S += (*u)[i]; }
  static const char* nms[] = {"n_used", "n_flat", "n_included", "n_left_out", "n_steps", "n_biased", "n_overdispersed", "worst_type_at", "min_agreement_at",
                              "lambda", "share", "move", "mean_share", "min_agreement", "worst_type", "max_dispersion", "gram", "type", "component", "tumour",
                              "series"};
  SEXP out = PROTECT(named_list(21, nms));
  SET_VECTOR_ELT(out, 16, Rf_allocMatrix(REALSXP, K, K));
  SET_VECTOR_ELT(out, 17, Rf_allocMatrix(REALSXP, K, BNMF_RES_NTYPE));
  SET_VECTOR_ELT(out, 18, Rf_allocMatrix(REALSXP, K, BNMF_RES_NCOMP));
  SET_VECTOR_ELT(out, 19, Rf_allocMatrix(REALSXP, G, BNMF_RES_NTUM));
  SET_VECTOR_ELT(out, 20, Rf_allocMatrix(REALSXP, S, BNMF_RES_NSER));
  UNPROTECT(1);
  return out;
}
static void res_finish(SEXP out, const bnmf_residuals_info* info) {
  const int32_t v[9] = {info->n_used, info->n_flat, info->n_included, info->n_left_out, info->n_steps, info->n_biased, info->n_overdispersed,
                        info->worst_type_at, info->min_agreement_at};
  for (int i = 0; i < 9; ++i) SET_VECTOR_ELT(out, i, Rf_ScalarInteger(v[i]));
  const double d[7] = {info->lambda, info->share, info->move, info->mean_share, info->min_agreement, info->worst_type, info->max_dispersion};
  for (int i = 0; i < 7; ++i) SET_VECTOR_ELT(out, 9 + i, Rf_ScalarReal(d[i]));
}
SEXP C_bnmf_residuals(SEXP ptr, SEXP end_iter, SEXP n_samples, SEXP used, SEXP include, SEXP opts) {
  int32_t *u = NULL, *inc = NULL;
  SEXP out = PROTECT(res_alloc(n_samples, used, include, opts, &u, &inc));
  bnmf_residuals_info info;
  if (end_iter == R_NilValue)
    chk(bnmf_residuals(get_handle(ptr), INTEGER(n_samples)[0], u, inc, (int)REAL(opts)[0], REAL(opts)[1], map_buf(out, 16), map_buf(out, 17), map_buf(out, 18),
                       map_buf(out, 19), map_buf(out, 20), &info));
  else
    chk(bnmf_residuals_at(get_handle(ptr), INTEGER(end_iter)[0], INTEGER(n_samples)[0], u, inc, (int)REAL(opts)[0], REAL(opts)[1], map_buf(out, 16),
                          map_buf(out, 17), map_buf(out, 18), map_buf(out, 19), map_buf(out, 20), &info));
  res_finish(out, &info);
  UNPROTECT(1);
  return out;
}
SEXP C_bnmf_residuals_at(SEXP ptr, SEXP end_iter, SEXP n_samples, SEXP used, SEXP include, SEXP opts) {
  int32_t *u = NULL, *inc = NULL;
  SEXP out = PROTECT(res_alloc(n_samples, used, include, opts, &u, &inc));
  bnmf_residuals_info info;
  chk(bnmf_residuals_at(get_handle(ptr), INTEGER(end_iter)[0], INTEGER(n_samples)[0], u, inc, (int)REAL(opts)[0], REAL(opts)[1], map_buf(out, 16),
                        map_buf(out, 17), map_buf(out, 18), map_buf(out, 19), map_buf(out, 20), &info));
  res_finish(out, &info);
  UNPROTECT(1);
  return out;
}
/* Trade-offs between signatures within a tumour on the device (bnmf_tradeoff / bnmf_tradeoff_at): C_bnmf_tradeoff(ptr, end_iter (integer,
 * or NULL = the current iteration), n_samples, used (logical length n_samples, or NULL = all), include (logical length G, or NULL = all),
 * perm (integer n_samples x N matrix of 0-based places, a row of -1 / NA = the sample is unmatched; or NULL = identity), sets (integer N
 * of 0-based sets, -1 / NA = in no set; or NULL), query (integer, 0-based tumours; or NULL), opts (real c(min_corr, C, G, N))) ->
 * list(n_used, n_matched, n_unmatched, n_included, n_left_out, n_sets, n_query, n_traded, strongest_pair_at (0-based j * N + l, -1 =
 * none), strongest_pair, mean_ratio, min_corr, tumour (G x 3: smallest correlation, defined pairs, variance ratio of the total), pair_at
 * (integer G, 0-based j * N + l, -1 = none), pair (N N x 5: mean r, n_def, share r <= -min_corr, share r >= min_corr, mean covariance;
 * row l + N j, symmetric), dense (N N x 2 x Q: covariance, correlation; NULL without a query), setstat (G x C x 4; NULL without sets))
 * over iterations end_iter - n_samples + 1 ... end_iter.  C_bnmf_tradeoff_at: the same with end_iter required */
typedef struct { int32_t *u, *inc, *perm, *sets, *q; int Q, C; double min_corr; } trd_in;
static SEXP trd_alloc(SEXP n_samples, SEXP used, SEXP include, SEXP perm, SEXP sets, SEXP query, SEXP opts, trd_in* in) {
  const int n = INTEGER(n_samples)[0];
  if (XLENGTH(opts) != 4) Rf_error("bnmf: opts has %ld entries, c(min_corr, C, G, N) is needed", (long)XLENGTH(opts));
  const double* o = REAL(opts);
  const int G = (int)o[2], N = (int)o[3];
  if (used != R_NilValue && XLENGTH(used) != (R_xlen_t)n) Rf_error("bnmf: used has %ld entries for %d samples", (long)XLENGTH(used), n);
  if (include != R_NilValue && XLENGTH(include) != (R_xlen_t)G) Rf_error("bnmf: include has %ld flags for %d tumours", (long)XLENGTH(include), G);
  if (perm != R_NilValue && XLENGTH(perm) != (R_xlen_t)n * N) Rf_error("bnmf: perm has %ld entries for %d samples of %d factors", (long)XLENGTH(perm), n, N);
  if (sets != R_NilValue && XLENGTH(sets) != (R_xlen_t)N) Rf_error("bnmf: sets has %ld labels for %d factors", (long)XLENGTH(sets), N);
  in->u = lgl_flags(used, n);
  in->inc = lgl_flags(include, G);
  in->perm = NULL;
  if (perm != R_NilValue) {                                                /* the R matrix is column-major: row s of the ABI is its row s */
    in->perm = (int32_t*)R_alloc((size_t)n * N, sizeof(int32_t));
    for (int s = 0; s < n; ++s) for (int j = 0; j < N; ++j) { const int v = INTEGER(perm)[s + (size_t)n * j]; in->perm[(size_t)s * N + j] = v == NA_INTEGER ? -1 : v; }
  }
  in->sets = NULL;
  if (sets != R_NilValue) {
    in->sets = (int32_t*)R_alloc((size_t)N, sizeof(int32_t));
    for (int j = 0; j < N; ++j) { const int v = INTEGER(sets)[j]; in->sets[j] = v == NA_INTEGER ? -1 : v; }
  }
  in->Q = query == R_NilValue ? 0 : (int)XLENGTH(query);
  in->q = in->Q > 0 ? (int32_t*)INTEGER(query) : NULL;
  in->min_corr = o[0]; in->C = (int)o[1];
  const int Cb = in->C > BNMF_TRD_MAX_C ? BNMF_TRD_MAX_C : in->C;          /* (the library refuses a larger C: the buffers only have to exist) */
  static const char* nms[] = {"n_used", "n_matched", "n_unmatched", "n_included", "n_left_out", "n_sets", "n_query", "n_traded", "strongest_pair_at",
                              "strongest_pair", "mean_ratio", "min_corr", "tumour", "pair_at", "pair", "dense", "setstat"};
  SEXP out = PROTECT(named_list(17, nms));
  SET_VECTOR_ELT(out, 12, Rf_allocMatrix(REALSXP, G, BNMF_TRD_NTUM));
  SET_VECTOR_ELT(out, 13, Rf_allocVector(INTSXP, G));
  SET_VECTOR_ELT(out, 14, Rf_allocMatrix(REALSXP, N * N, BNMF_TRD_NPAIR));
  if (in->Q > 0) SET_VECTOR_ELT(out, 15, Rf_allocVector(REALSXP, (R_xlen_t)N * N * 2 * in->Q));
  if (Cb > 0) SET_VECTOR_ELT(out, 16, Rf_allocVector(REALSXP, (R_xlen_t)G * Cb * BNMF_TRD_NSET));
  UNPROTECT(1);
  return out;
}
static int32_t* trd_int_buf(SEXP out, int i) { SEXP x = VECTOR_ELT(out, i); return x == R_NilValue ? NULL : (int32_t*)INTEGER(x); }
static void trd_finish(SEXP out, const bnmf_tradeoff_info* info) {
  const int32_t v[9] = {info->n_used, info->n_matched, info->n_unmatched, info->n_included, info->n_left_out, info->n_sets, info->n_query, info->n_traded,
                        info->strongest_pair_at};
  for (int i = 0; i < 9; ++i) SET_VECTOR_ELT(out, i, Rf_ScalarInteger(v[i]));
  SET_VECTOR_ELT(out, 9, Rf_ScalarReal(info->strongest_pair)); SET_VECTOR_ELT(out, 10, Rf_ScalarReal(info->mean_ratio));
  SET_VECTOR_ELT(out, 11, Rf_ScalarReal(info->min_corr));
}
SEXP C_bnmf_tradeoff(SEXP ptr, SEXP end_iter, SEXP n_samples, SEXP used, SEXP include, SEXP perm, SEXP sets, SEXP query, SEXP opts) {
  trd_in in;
  SEXP out = PROTECT(trd_alloc(n_samples, used, include, perm, sets, query, opts, &in));
  bnmf_tradeoff_info info;
  if (end_iter == R_NilValue)
    chk(bnmf_tradeoff(get_handle(ptr), INTEGER(n_samples)[0], in.u, in.inc, in.perm, in.sets, in.C, in.q, in.Q, in.min_corr, map_buf(out, 12), trd_int_buf(out, 13),
                      map_buf(out, 14), map_buf(out, 15), map_buf(out, 16), &info));
  else
    chk(bnmf_tradeoff_at(get_handle(ptr), INTEGER(end_iter)[0], INTEGER(n_samples)[0], in.u, in.inc, in.perm, in.sets, in.C, in.q, in.Q, in.min_corr,
                         map_buf(out, 12), trd_int_buf(out, 13), map_buf(out, 14), map_buf(out, 15), map_buf(out, 16), &info));
  trd_finish(out, &info);
  UNPROTECT(1);
  return out;
}
SEXP C_bnmf_tradeoff_at(SEXP ptr, SEXP end_iter, SEXP n_samples, SEXP used, SEXP include, SEXP perm, SEXP sets, SEXP query, SEXP opts) {
  trd_in in;
  SEXP out = PROTECT(trd_alloc(n_samples, used, include, perm, sets, query, opts, &in));
  bnmf_tradeoff_info info;
  chk(bnmf_tradeoff_at(get_handle(ptr), INTEGER(end_iter)[0], INTEGER(n_samples)[0], in.u, in.inc, in.perm, in.sets, in.C, in.q, in.Q, in.min_corr,
                       map_buf(out, 12), trd_int_buf(out, 13), map_buf(out, 14), map_buf(out, 15), map_buf(out, 16), &info));
  trd_finish(out, &info);
  UNPROTECT(1);
  return out;
}
/* Cohort summary of signatures over recorded samples on the device (bnmf_summary / bnmf_summary_at): C_bnmf_summary(ptr, end_iter (integer,
 * or NULL = the current iteration), n_samples, used (logical length n_samples, or NULL = all), include (logical length G, or NULL = all),
 * perm (integer n_samples x N matrix of 0-based places, a row of -1 / NA = the sample is left out; or NULL = identity), probs (real, the
 * L levels), opts (real c(min_load, credible_interval, want_series 0 / 1, G, N))) -> list(n_used, n_aligned, n_included, n_left_out,
 * n_levels, n_blocks, n_nonfinite, min_load, credible_interval, stat (N x 5 NSTAT: column 5 q + i = row i — mean, variance, lower, upper,
 * n_valid — of statistic q; NSTAT = 4 + 3 L: prevalence, total, fraction, mean_present, then L of load_all, load_present, share_all),
 * series (N x NSTAT S: column S q + s; or NULL)) over iterations end_iter - n_samples + 1 ... end_iter.  C_bnmf_summary_at: the same with
 * end_iter required */
typedef struct { int32_t *u, *inc, *perm; int L; double min_load, ci; } sum_in;
static SEXP sum_alloc(SEXP n_samples, SEXP used, SEXP include, SEXP perm, SEXP probs, SEXP opts, sum_in* in) {
  const int n = INTEGER(n_samples)[0];
  if (XLENGTH(opts) != 5) Rf_error("bnmf: opts has %ld entries, c(min_load, credible_interval, want_series, G, N) is needed", (long)XLENGTH(opts));
  const double* o = REAL(opts);
  const int G = (int)o[3], N = (int)o[4];
  if (used != R_NilValue && XLENGTH(used) != (R_xlen_t)n) Rf_error("bnmf: used has %ld entries for %d samples", (long)XLENGTH(used), n);
  if (include != R_NilValue && XLENGTH(include) != (R_xlen_t)G) Rf_error("bnmf: include has %ld flags for %d tumours", (long)XLENGTH(include), G);
  if (perm != R_NilValue && XLENGTH(perm) != (R_xlen_t)n * N) Rf_error("bnmf: perm has %ld entries for %d samples of %d factors", (long)XLENGTH(perm), n, N);
  in->u = lgl_flags(used, n);
  in->inc = lgl_flags(include, G);
  in->perm = NULL;
  if (perm != R_NilValue) {                                                /* the R matrix is column-major: row s of the ABI is its row s */
    in->perm = (int32_t*)R_alloc((size_t)n * N, sizeof(int32_t));
    for (int s = 0; s < n; ++s) for (int j = 0; j < N; ++j) { const int v = INTEGER(perm)[s + (size_t)n * j]; in->perm[(size_t)s * N + j] = v == NA_INTEGER ? -1 : v; }
  }
  in->L = (int)XLENGTH(probs); in->min_load = o[0]; in->ci = o[1];
  const int Lb = in->L > BNMF_SUM_MAX_Q ? BNMF_SUM_MAX_Q : in->L;          /* (the library refuses more levels: the buffers only have to exist) */
  const int nstat = BNMF_SUM_NSCAL + 3 * Lb;
  int S = n < 0 ? 0 : n;
  if (in->u) { S = 0; for (int i = 0; i < n; ++i) S += in->u[i]; }
  static const char* nms[] = {"n_used", "n_aligned", "n_included", "n_left_out", "n_levels", "n_blocks", "n_nonfinite", "min_load", "credible_interval",
                              "stat", "series"};
  SEXP out = PROTECT(named_list(11, nms));
  SET_VECTOR_ELT(out, 9, Rf_allocMatrix(REALSXP, N, BNMF_SUM_NROW * nstat));
  if (o[2] != 0.0) SET_VECTOR_ELT(out, 10, Rf_allocMatrix(REALSXP, N, nstat * S));
  UNPROTECT(1);
  return out;
}
static void sum_finish(SEXP out, const bnmf_summary_info* info) {
  const int32_t v[6] = {info->n_used, info->n_aligned, info->n_included, info->n_left_out, info->n_levels, info->n_blocks};
  for (int i = 0; i < 6; ++i) SET_VECTOR_ELT(out, i, Rf_ScalarInteger(v[i]));
  SET_VECTOR_ELT(out, 6, Rf_ScalarReal((double)info->n_nonfinite)); SET_VECTOR_ELT(out, 7, Rf_ScalarReal(info->min_load));
  SET_VECTOR_ELT(out, 8, Rf_ScalarReal(info->credible_interval));
}
SEXP C_bnmf_summary(SEXP ptr, SEXP end_iter, SEXP n_samples, SEXP used, SEXP include, SEXP perm, SEXP probs, SEXP opts) {
  sum_in in;
  SEXP out = PROTECT(sum_alloc(n_samples, used, include, perm, probs, opts, &in));
  bnmf_summary_info info;
  if (end_iter == R_NilValue)
    chk(bnmf_summary(get_handle(ptr), INTEGER(n_samples)[0], in.u, in.inc, in.perm, in.min_load, REAL(probs), in.L, in.ci, map_buf(out, 9), map_buf(out, 10), &info));
  else
    chk(bnmf_summary_at(get_handle(ptr), INTEGER(end_iter)[0], INTEGER(n_samples)[0], in.u, in.inc, in.perm, in.min_load, REAL(probs), in.L, in.ci, map_buf(out, 9),
                        map_buf(out, 10), &info));
  sum_finish(out, &info);
  UNPROTECT(1);
  return out;
}
SEXP C_bnmf_summary_at(SEXP ptr, SEXP end_iter, SEXP n_samples, SEXP used, SEXP include, SEXP perm, SEXP probs, SEXP opts) {
  sum_in in;
  SEXP out = PROTECT(sum_alloc(n_samples, used, include, perm, probs, opts, &in));
  bnmf_summary_info info;
  chk(bnmf_summary_at(get_handle(ptr), INTEGER(end_iter)[0], INTEGER(n_samples)[0], in.u, in.inc, in.perm, in.min_load, REAL(probs), in.L, in.ci, map_buf(out, 9),
                      map_buf(out, 10), &info));
  sum_finish(out, &info);
  UNPROTECT(1);
  return out;
}
/* Sparse per-tumour assignment with refit on the device (bnmf_prune / bnmf_prune_at): C_bnmf_prune(ptr, end_iter (integer, or NULL = the
 * current iteration), n_samples, used (logical length n_samples, or NULL = all), include (logical length G, or NULL = all), opts (real
 * c(n_steps, max_loss, want_exposures 0 / 1, G, N))) -> list(n_used, n_included, n_undefined, n_single, n_steps, trials, max_change,
 * max_loss, load (N G x 4: mean sparse exposure, its variance, mean share, p_kept - each laid out as E), tumour (G x 7: mean cos_0, mean
 * cos_f, mean / smallest / largest n_kept, largest change, mean trials), series (S x 2: mean n_kept, mean cos_f per used sample), signature
 * (N x 3: tumours with p_kept >= 0.5, mean p_kept, sum of the mean loads), exposures (N G x S, or NULL)) over iterations
 * end_iter - n_samples + 1 ... end_iter.  C_bnmf_prune_at: the same with end_iter required */
typedef struct { int32_t *u, *inc; int n_steps; double max_loss; } prn_in;
static SEXP prn_alloc(SEXP n_samples, SEXP used, SEXP include, SEXP opts, prn_in* in) {
  const int n = INTEGER(n_samples)[0];
  if (XLENGTH(opts) != 5) Rf_error("bnmf: opts has %ld entries, c(n_steps, max_loss, want_exposures, G, N) is needed", (long)XLENGTH(opts));
  const double* o = REAL(opts);
  const int G = (int)o[3], N = (int)o[4];
  if (used != R_NilValue && XLENGTH(used) != (R_xlen_t)n) Rf_error("bnmf: used has %ld entries for %d samples", (long)XLENGTH(used), n);
  if (include != R_NilValue && XLENGTH(include) != (R_xlen_t)G) Rf_error("bnmf: include has %ld flags for %d tumours", (long)XLENGTH(include), G);
  in->u = lgl_flags(used, n);
  in->inc = lgl_flags(include, G);
  in->n_steps = (int)o[0]; in->max_loss = o[1];
  int S = n < 0 ? 0 : n;
  if (in->u) { S = 0; for (int i = 0; i < n; ++i) S += in->u[i]; }
  static const char* nms[] = {"n_used", "n_included", "n_undefined", "n_single", "n_steps", "trials", "max_change", "max_loss", "load", "tumour", "series",
                              "signature", "exposures"};
  SEXP out = PROTECT(named_list(13, nms));
  SET_VECTOR_ELT(out, 8, Rf_allocMatrix(REALSXP, N * G, BNMF_PRN_NLOAD));
  SET_VECTOR_ELT(out, 9, Rf_allocMatrix(REALSXP, G, BNMF_PRN_NTUM));
  SET_VECTOR_ELT(out, 10, Rf_allocMatrix(REALSXP, S, BNMF_PRN_NSER));
  SET_VECTOR_ELT(out, 11, Rf_allocMatrix(REALSXP, N, BNMF_PRN_NSIG));
  if (o[2] != 0.0) SET_VECTOR_ELT(out, 12, Rf_allocMatrix(REALSXP, N * G, S));
  UNPROTECT(1);
  return out;
}
static void prn_finish(SEXP out, const bnmf_prune_info* info) {
  const int32_t v[5] = {info->n_used, info->n_included, info->n_undefined, info->n_single, info->n_steps};
  for (int i = 0; i < 5; ++i) SET_VECTOR_ELT(out, i, Rf_ScalarInteger(v[i]));
  SET_VECTOR_ELT(out, 5, Rf_ScalarReal((double)info->trials)); SET_VECTOR_ELT(out, 6, Rf_ScalarReal(info->max_change));
  SET_VECTOR_ELT(out, 7, Rf_ScalarReal(info->max_loss));
}
SEXP C_bnmf_prune(SEXP ptr, SEXP end_iter, SEXP n_samples, SEXP used, SEXP include, SEXP opts) {
  prn_in in;
  SEXP out = PROTECT(prn_alloc(n_samples, used, include, opts, &in));
  bnmf_prune_info info;
  if (end_iter == R_NilValue)
    chk(bnmf_prune(get_handle(ptr), INTEGER(n_samples)[0], in.u, in.inc, in.n_steps, in.max_loss, map_buf(out, 8), map_buf(out, 9), map_buf(out, 10), map_buf(out, 11),
                   map_buf(out, 12), &info));
  else
    chk(bnmf_prune_at(get_handle(ptr), INTEGER(end_iter)[0], INTEGER(n_samples)[0], in.u, in.inc, in.n_steps, in.max_loss, map_buf(out, 8), map_buf(out, 9),
                      map_buf(out, 10), map_buf(out, 11), map_buf(out, 12), &info));
  prn_finish(out, &info);
  UNPROTECT(1);
  return out;
}
SEXP C_bnmf_prune_at(SEXP ptr, SEXP end_iter, SEXP n_samples, SEXP used, SEXP include, SEXP opts) {
  prn_in in;
  SEXP out = PROTECT(prn_alloc(n_samples, used, include, opts, &in));
  bnmf_prune_info info;
  chk(bnmf_prune_at(get_handle(ptr), INTEGER(end_iter)[0], INTEGER(n_samples)[0], in.u, in.inc, in.n_steps, in.max_loss, map_buf(out, 8), map_buf(out, 9),
                    map_buf(out, 10), map_buf(out, 11), map_buf(out, 12), &info));
  prn_finish(out, &info);
  UNPROTECT(1);
  return out;
}
/* Silhouette stability of the recorded signatures on the device (bnmf_stability / bnmf_stability_at): C_bnmf_stability(ptr, end_iter
 * (integer, or NULL = the current iteration), n_samples, used (logical length n_samples, or NULL = all), labels (integer n_samples x N
 * matrix of 0-based clusters, -1 / NA = left out; or NULL = the factor), extra_P (K x X real matrix, or NULL), extra_label (integer X,
 * 0-based; or NULL), dims c(K,G,N)) -> list(n_used, n_points, n_extra, n_left_out, n_clusters, min_stability_at (0-based label, -1 =
 * none), n_negative, mean_silhouette, min_stability, point ((S N + X) x 4: silhouette, a, b, nearest (0-based, -1 = none); row s N + n
 * is factor n of used sample s, then the extras), factor (N x 6: members, stability, min silhouette, mean a, mean b, share negative),
 * between (N x N, column a = the distances from cluster a), medoid (K x N), medoid_at (N 0-based points, -1 = empty)) over iterations
 * end_iter - n_samples + 1 ... end_iter.  C_bnmf_stability_at: the same with end_iter required */
/* the result list with its arrays allocated, the flags of used, the labels row-major and X; returned unprotected */
static SEXP stab_alloc(SEXP n_samples, SEXP used, SEXP labels, SEXP extra_P, SEXP extra_label, SEXP dims, int32_t** u, int32_t** lab, int* X) {
  const int n = INTEGER(n_samples)[0];
  const int* d = INTEGER(dims);
  const int K = d[0], N = d[2];
  if (used != R_NilValue && XLENGTH(used) != (R_xlen_t)n) Rf_error("bnmf: used has %ld entries for %d samples", (long)XLENGTH(used), n);
  if (labels != R_NilValue && XLENGTH(labels) != (R_xlen_t)n * N) Rf_error("bnmf: labels has %ld entries for %d samples of %d factors", (long)XLENGTH(labels), n, N);
  *X = 0;
  if (extra_P != R_NilValue) {
    if (K < 1 || XLENGTH(extra_P) % (R_xlen_t)K != 0) Rf_error("bnmf: extra_P has %ld values, not a multiple of K = %d rows", (long)XLENGTH(extra_P), K);
    *X = (int)(XLENGTH(extra_P) / (R_xlen_t)K);
    if (extra_label == R_NilValue || XLENGTH(extra_label) != (R_xlen_t)*X) Rf_error("bnmf: extra_label must hold one label per extra column (%d)", *X);
  }
  *u = lgl_flags(used, n);
  *lab = NULL;
  if (labels != R_NilValue) {                                             /* column-major n x N -> row-major, NA = left out */
    *lab = (int32_t*)R_alloc((size_t)n * N, sizeof(int32_t));
    for (int s = 0; s < n; ++s) for (int f = 0; f < N; ++f) { const int v = INTEGER(labels)[s + (size_t)n * f]; (*lab)[(size_t)s * N + f] = v == NA_INTEGER ? -1 : v; }
  }
  int S = n < 0 ? 0 : n;
  if (*u) { S = 0; for (int i = 0; i < n; ++i) S += (*u)[i]; }
  static const char* nms[] = {"n_used", "n_points", "n_extra", "n_left_out", "n_clusters", "min_stability_at", "n_negative", "mean_silhouette",
                              "min_stability", "point", "factor", "between", "medoid", "medoid_at"};
  SEXP out = PROTECT(named_list(14, nms));
  SET_VECTOR_ELT(out, 9, Rf_allocMatrix(REALSXP, S * N + *X, BNMF_STAB_NPOINT));
  SET_VECTOR_ELT(out, 10, Rf_allocMatrix(REALSXP, N, BNMF_STAB_NFROW));
  SET_VECTOR_ELT(out, 11, Rf_allocMatrix(REALSXP, N, N));
  SET_VECTOR_ELT(out, 12, Rf_allocMatrix(REALSXP, K, N));
  SET_VECTOR_ELT(out, 13, Rf_allocVector(REALSXP, N));
  UNPROTECT(1);
  return out;
}
static void stab_finish(SEXP out, const bnmf_stability_info* info, const int64_t* at, int N) {
  SET_VECTOR_ELT(out, 0, Rf_ScalarInteger(info->n_used)); SET_VECTOR_ELT(out, 1, Rf_ScalarInteger(info->n_points));
  SET_VECTOR_ELT(out, 2, Rf_ScalarInteger(info->n_extra)); SET_VECTOR_ELT(out, 3, Rf_ScalarInteger(info->n_left_out));
  SET_VECTOR_ELT(out, 4, Rf_ScalarInteger(info->n_clusters)); SET_VECTOR_ELT(out, 5, Rf_ScalarInteger(info->min_stability_at));
  SET_VECTOR_ELT(out, 6, Rf_ScalarReal((double)info->n_negative)); SET_VECTOR_ELT(out, 7, Rf_ScalarReal(info->mean_silhouette));
  SET_VECTOR_ELT(out, 8, Rf_ScalarReal(info->min_stability));
  for (int j = 0; j < N; ++j) REAL(VECTOR_ELT(out, 13))[j] = (double)at[j];
}
SEXP C_bnmf_stability(SEXP ptr, SEXP end_iter, SEXP n_samples, SEXP used, SEXP labels, SEXP extra_P, SEXP extra_label, SEXP dims) {
  int32_t *u = NULL, *lab = NULL; int X = 0;
  const int N = INTEGER(dims)[2];
  SEXP out = PROTECT(stab_alloc(n_samples, used, labels, extra_P, extra_label, dims, &u, &lab, &X));
  int64_t* at = (int64_t*)R_alloc((size_t)(N > 0 ? N : 1), sizeof(int64_t));
  const double* ex = X > 0 ? REAL(extra_P) : NULL;
  const int32_t* el = X > 0 ? (const int32_t*)INTEGER(extra_label) : NULL;
  bnmf_stability_info info;
  if (end_iter == R_NilValue)
    chk(bnmf_stability(get_handle(ptr), INTEGER(n_samples)[0], u, lab, ex, el, X, map_buf(out, 9), map_buf(out, 10), map_buf(out, 11), map_buf(out, 12), at, &info));
  else
    chk(bnmf_stability_at(get_handle(ptr), INTEGER(end_iter)[0], INTEGER(n_samples)[0], u, lab, ex, el, X, map_buf(out, 9), map_buf(out, 10), map_buf(out, 11),
                          map_buf(out, 12), at, &info));
  stab_finish(out, &info, at, N);
  UNPROTECT(1);
  return out;
}
SEXP C_bnmf_stability_at(SEXP ptr, SEXP end_iter, SEXP n_samples, SEXP used, SEXP labels, SEXP extra_P, SEXP extra_label, SEXP dims) {
  int32_t *u = NULL, *lab = NULL; int X = 0;
  const int N = INTEGER(dims)[2];
  SEXP out = PROTECT(stab_alloc(n_samples, used, labels, extra_P, extra_label, dims, &u, &lab, &X));
  int64_t* at = (int64_t*)R_alloc((size_t)(N > 0 ? N : 1), sizeof(int64_t));
  bnmf_stability_info info;
  chk(bnmf_stability_at(get_handle(ptr), INTEGER(end_iter)[0], INTEGER(n_samples)[0], u, lab, X > 0 ? REAL(extra_P) : NULL,
                        X > 0 ? (const int32_t*)INTEGER(extra_label) : NULL, X, map_buf(out, 9), map_buf(out, 10), map_buf(out, 11), map_buf(out, 12), at, &info));
  stab_finish(out, &info, at, N);
  UNPROTECT(1);
  return out;
}
/* Exposures of new tumours under the recorded signatures on the device (bnmf_project / bnmf_project_at): C_bnmf_project(ptr, end_iter
 * (integer, or NULL = the current iteration), n_samples, used (logical length n_samples, or NULL = all), X (K x J real matrix, not
 * negative), n_steps, min_load, want_exposures (logical), dims c(K,G,N)) -> list(n_used, n_steps, n_present, min_load, total,
 * max_rel_change, min_cosine, min_cosine_at (0-based j; -1 if none), load (N J x 4: one column per row of the C output — mean, variance,
 * mean share, probability of presence — each laid out as E), fit (J x 3: mean cosine, mean relative L1 error, largest last-step
 * change), series (N x S), exposures (N J x S: one column per used sample, laid out as E; or NULL)) over iterations
 * end_iter - n_samples + 1 ... end_iter.
 * C_bnmf_project_at: the same with end_iter required */
/* the result list with load, fit, series and (if wanted) exposures allocated, the flags of used and J; returned unprotected */
static SEXP project_alloc(SEXP n_samples, SEXP used, SEXP X, SEXP want_exposures, SEXP dims, int32_t** u, int* J) {
  const int n = INTEGER(n_samples)[0];
  const int* d = INTEGER(dims);
  if (d[0] < 1 || XLENGTH(X) % (R_xlen_t)d[0] != 0) Rf_error("bnmf: X has %ld values, not a multiple of K = %d rows", (long)XLENGTH(X), d[0]);
  *J = (int)(XLENGTH(X) / (R_xlen_t)d[0]);
  if (used != R_NilValue && XLENGTH(used) != (R_xlen_t)n) Rf_error("bnmf: used has %ld entries for %d samples", (long)XLENGTH(used), n);
  *u = lgl_flags(used, n);
  int S = n < 0 ? 0 : n;
  if (*u) { S = 0; for (int i = 0; i < n; ++i) S += (*u)[i]; }
  static const char* nms[] = {"n_used", "n_steps", "n_present", "min_load", "total", "max_rel_change", "min_cosine", "min_cosine_at", "load", "fit",
                              "series", "exposures"};
  SEXP out = PROTECT(named_list(12, nms));
  SET_VECTOR_ELT(out, 8, Rf_allocMatrix(REALSXP, d[2] * *J, BNMF_PROJ_NLOAD));
  SET_VECTOR_ELT(out, 9, Rf_allocMatrix(REALSXP, *J, BNMF_PROJ_NFIT));
  SET_VECTOR_ELT(out, 10, Rf_allocMatrix(REALSXP, d[2], S));
  if (LOGICAL(want_exposures)[0] == TRUE) SET_VECTOR_ELT(out, 11, Rf_allocMatrix(REALSXP, d[2] * *J, S));
  UNPROTECT(1);
  return out;
}
static void project_finish(SEXP out, const bnmf_project_info* info) {
  SET_VECTOR_ELT(out, 0, Rf_ScalarInteger(info->n_used)); SET_VECTOR_ELT(out, 1, Rf_ScalarInteger(info->n_steps));
  SET_VECTOR_ELT(out, 2, Rf_ScalarReal((double)info->n_present)); SET_VECTOR_ELT(out, 3, Rf_ScalarReal(info->min_load));
  SET_VECTOR_ELT(out, 4, Rf_ScalarReal(info->total)); SET_VECTOR_ELT(out, 5, Rf_ScalarReal(info->max_rel_change));
  SET_VECTOR_ELT(out, 6, Rf_ScalarReal(info->min_cosine)); SET_VECTOR_ELT(out, 7, Rf_ScalarReal((double)info->min_cosine_at));
}
SEXP C_bnmf_project(SEXP ptr, SEXP end_iter, SEXP n_samples, SEXP used, SEXP X, SEXP n_steps, SEXP min_load, SEXP want_exposures, SEXP dims) {
  int32_t* u = NULL; int J = 0;
  SEXP out = PROTECT(project_alloc(n_samples, used, X, want_exposures, dims, &u, &J));
  bnmf_project_info info;
  if (end_iter == R_NilValue)
    chk(bnmf_project(get_handle(ptr), INTEGER(n_samples)[0], u, REAL(X), J, INTEGER(n_steps)[0], REAL(min_load)[0], map_buf(out, 8), map_buf(out, 9),
                     map_buf(out, 10), map_buf(out, 11), &info));
  else
    chk(bnmf_project_at(get_handle(ptr), INTEGER(end_iter)[0], INTEGER(n_samples)[0], u, REAL(X), J, INTEGER(n_steps)[0], REAL(min_load)[0],
                        map_buf(out, 8), map_buf(out, 9), map_buf(out, 10), map_buf(out, 11), &info));
  project_finish(out, &info);
  UNPROTECT(1);
  return out;
}
SEXP C_bnmf_project_at(SEXP ptr, SEXP end_iter, SEXP n_samples, SEXP used, SEXP X, SEXP n_steps, SEXP min_load, SEXP want_exposures, SEXP dims) {
  int32_t* u = NULL; int J = 0;
  SEXP out = PROTECT(project_alloc(n_samples, used, X, want_exposures, dims, &u, &J));
  bnmf_project_info info;
  chk(bnmf_project_at(get_handle(ptr), INTEGER(end_iter)[0], INTEGER(n_samples)[0], u, REAL(X), J, INTEGER(n_steps)[0], REAL(min_load)[0],
                      map_buf(out, 8), map_buf(out, 9), map_buf(out, 10), map_buf(out, 11), &info));
  project_finish(out, &info);
  UNPROTECT(1);
  return out;
}
/* Decomposition of the recorded signatures into a reference catalogue on the device (bnmf_decompose / bnmf_decompose_at):
 * C_bnmf_decompose(ptr, end_iter (integer, or NULL = the current iteration), n_samples, used (logical length n_samples, or NULL = all),
 * reference_P (K x R real matrix, not negative, no all-zero column), keep (logical length N, or NULL = all), min_share, opts (integer
 * c(n_steps, want_weights as 0 / 1): .Call routines here take at most 9 arguments), dims c(K,G,N)) -> list(n_used, n_steps, R, n_present, min_share, max_rel_change, min_cosine, min_cosine_at
 * (0-based n; -1 if none), weight (R N x 4: one column per row of the C output — mean, variance, mean share, probability of presence —
 * each laid out r + R n), fit (N x 3: mean cosine, mean relative L1 error, largest last-step change), nactive (N x S integer), included
 * (N integer), weights (R N x S: one column per used sample, laid out r + R n; or NULL)) over iterations
 * end_iter - n_samples + 1 ... end_iter.
 * C_bnmf_decompose_at: the same with end_iter required */
/* the result list with weight, fit, nactive, included and (if wanted) weights allocated, the flags of used and keep, and R; returned
 * unprotected */
static SEXP decompose_alloc(SEXP n_samples, SEXP used, SEXP ref, SEXP keep, SEXP opts, SEXP dims, int32_t** u, int32_t** kp, int* R) {
  const int n = INTEGER(n_samples)[0];
  const int* d = INTEGER(dims);
  if (XLENGTH(opts) != 2) Rf_error("bnmf: opts has %ld entries, c(n_steps, want_weights) is needed", (long)XLENGTH(opts));
  if (d[0] < 1 || XLENGTH(ref) % (R_xlen_t)d[0] != 0) Rf_error("bnmf: reference_P has %ld values, not a multiple of K = %d rows", (long)XLENGTH(ref), d[0]);
  *R = (int)(XLENGTH(ref) / (R_xlen_t)d[0]);
  if (used != R_NilValue && XLENGTH(used) != (R_xlen_t)n) Rf_error("bnmf: used has %ld entries for %d samples", (long)XLENGTH(used), n);
  if (keep != R_NilValue && XLENGTH(keep) != (R_xlen_t)d[2]) Rf_error("bnmf: keep has %ld entries for %d factors", (long)XLENGTH(keep), d[2]);
  *u = lgl_flags(used, n);
  *kp = lgl_flags(keep, d[2]);
  int S = n < 0 ? 0 : n;
  if (*u) { S = 0; for (int i = 0; i < n; ++i) S += (*u)[i]; }
  static const char* nms[] = {"n_used", "n_steps", "R", "n_present", "min_share", "max_rel_change", "min_cosine", "min_cosine_at", "weight", "fit",
                              "nactive", "included", "weights"};
  SEXP out = PROTECT(named_list(13, nms));
  SET_VECTOR_ELT(out, 8, Rf_allocMatrix(REALSXP, *R * d[2], BNMF_DEC_NW));
  SET_VECTOR_ELT(out, 9, Rf_allocMatrix(REALSXP, d[2], BNMF_DEC_NFIT));
  SET_VECTOR_ELT(out, 10, Rf_allocMatrix(INTSXP, d[2], S));
  SET_VECTOR_ELT(out, 11, Rf_allocVector(INTSXP, d[2]));
  if (INTEGER(opts)[1] != 0) SET_VECTOR_ELT(out, 12, Rf_allocMatrix(REALSXP, *R * d[2], S));
  UNPROTECT(1);
  return out;
}
static void decompose_finish(SEXP out, const bnmf_decompose_info* info) {
  SET_VECTOR_ELT(out, 0, Rf_ScalarInteger(info->n_used)); SET_VECTOR_ELT(out, 1, Rf_ScalarInteger(info->n_steps));
  SET_VECTOR_ELT(out, 2, Rf_ScalarInteger(info->R)); SET_VECTOR_ELT(out, 3, Rf_ScalarReal((double)info->n_present));
  SET_VECTOR_ELT(out, 4, Rf_ScalarReal(info->min_share)); SET_VECTOR_ELT(out, 5, Rf_ScalarReal(info->max_rel_change));
  SET_VECTOR_ELT(out, 6, Rf_ScalarReal(info->min_cosine)); SET_VECTOR_ELT(out, 7, Rf_ScalarReal((double)info->min_cosine_at));
}
SEXP C_bnmf_decompose(SEXP ptr, SEXP end_iter, SEXP n_samples, SEXP used, SEXP ref, SEXP keep, SEXP min_share, SEXP opts, SEXP dims) {
  int32_t *u = NULL, *kp = NULL; int R = 0;
  SEXP out = PROTECT(decompose_alloc(n_samples, used, ref, keep, opts, dims, &u, &kp, &R));
  bnmf_decompose_info info;
  if (end_iter == R_NilValue)
    chk(bnmf_decompose(get_handle(ptr), INTEGER(n_samples)[0], u, REAL(ref), R, kp, INTEGER(opts)[0], REAL(min_share)[0], map_buf(out, 8),
                       map_buf(out, 9), (int32_t*)INTEGER(VECTOR_ELT(out, 10)), (int32_t*)INTEGER(VECTOR_ELT(out, 11)), map_buf(out, 12), &info));
  else
    chk(bnmf_decompose_at(get_handle(ptr), INTEGER(end_iter)[0], INTEGER(n_samples)[0], u, REAL(ref), R, kp, INTEGER(opts)[0], REAL(min_share)[0],
                          map_buf(out, 8), map_buf(out, 9), (int32_t*)INTEGER(VECTOR_ELT(out, 10)), (int32_t*)INTEGER(VECTOR_ELT(out, 11)),
                          map_buf(out, 12), &info));
  decompose_finish(out, &info);
  UNPROTECT(1);
  return out;
}
SEXP C_bnmf_decompose_at(SEXP ptr, SEXP end_iter, SEXP n_samples, SEXP used, SEXP ref, SEXP keep, SEXP min_share, SEXP opts, SEXP dims) {
  int32_t *u = NULL, *kp = NULL; int R = 0;
  SEXP out = PROTECT(decompose_alloc(n_samples, used, ref, keep, opts, dims, &u, &kp, &R));
  bnmf_decompose_info info;
  chk(bnmf_decompose_at(get_handle(ptr), INTEGER(end_iter)[0], INTEGER(n_samples)[0], u, REAL(ref), R, kp, INTEGER(opts)[0], REAL(min_share)[0],
                        map_buf(out, 8), map_buf(out, 9), (int32_t*)INTEGER(VECTOR_ELT(out, 10)), (int32_t*)INTEGER(VECTOR_ELT(out, 11)),
                        map_buf(out, 12), &info));
  decompose_finish(out, &info);
  UNPROTECT(1);
  return out;
}
/* Label-switching correction over recorded samples on the device (bnmf_relabel / bnmf_relabel_at): C_bnmf_relabel(ptr, end_iter (integer,
 * or NULL = the current iteration), n_samples, used (logical length n_samples, or NULL = all), pivot_P (K x N, or NULL = the newest used
 * sample's P), max_rounds, want_aligned (logical), dims c(K,G,N)) -> list(n_used, n_aligned, n_unmatched, rounds, converged, n_switched,
 * n_changed_last, mean_cosine, min_cosine, min_cosine_at (1-based position in perm as a double, 0 = none), perm (N x S: one column per used
 * sample, the 1-based label of every factor, NA for a sample without an assignment), cosine (N x S), confusion (N x N: samples in which
 * factor [row] received label [column]), P (K N x 2) and E (N G x 2): mean and variance of the aligned samples, each column laid out as P /
 * E, aligned_P (K N x S) and aligned_E (N G x S) or NULL) over iterations end_iter - n_samples + 1 ... end_iter.
 * C_bnmf_relabel_at: the same with end_iter required */
/* the result list with its buffers allocated, the flags of used and the pivot; returned unprotected */
static SEXP relabel_alloc(SEXP n_samples, SEXP used, SEXP pivot_P, SEXP want_aligned, SEXP dims, int32_t** u, const double** piv) {
  const int n = INTEGER(n_samples)[0];
  const int* d = INTEGER(dims);
  if (used != R_NilValue && XLENGTH(used) != (R_xlen_t)n) Rf_error("bnmf: used has %ld entries for %d samples", (long)XLENGTH(used), n);
  if (pivot_P != R_NilValue && XLENGTH(pivot_P) != (R_xlen_t)d[0] * d[2])
    Rf_error("bnmf: pivot_P has %ld entries, K x N = %d x %d are needed", (long)XLENGTH(pivot_P), d[0], d[2]);
  *u = lgl_flags(used, n);
  *piv = pivot_P == R_NilValue ? NULL : REAL(pivot_P);
  int S = n < 0 ? 0 : n;
  if (*u) { S = 0; for (int i = 0; i < n; ++i) S += (*u)[i]; }
  static const char* nms[] = {"n_used", "n_aligned", "n_unmatched", "rounds", "converged", "n_switched", "n_changed_last", "mean_cosine",
                              "min_cosine", "min_cosine_at", "perm", "cosine", "confusion", "P", "E", "aligned_P", "aligned_E"};
  SEXP out = PROTECT(named_list(17, nms));
  SET_VECTOR_ELT(out, 10, Rf_allocMatrix(INTSXP, d[2], S));
  SET_VECTOR_ELT(out, 11, Rf_allocMatrix(REALSXP, d[2], S));
  SET_VECTOR_ELT(out, 12, Rf_allocMatrix(REALSXP, d[2], d[2]));
  SET_VECTOR_ELT(out, 13, Rf_allocMatrix(REALSXP, d[0] * d[2], BNMF_NREL));
  SET_VECTOR_ELT(out, 14, Rf_allocMatrix(REALSXP, d[2] * d[1], BNMF_NREL));
  if (LOGICAL(want_aligned)[0] == TRUE) {
    SET_VECTOR_ELT(out, 15, Rf_allocMatrix(REALSXP, d[0] * d[2], S));
    SET_VECTOR_ELT(out, 16, Rf_allocMatrix(REALSXP, d[2] * d[1], S));
  }
  UNPROTECT(1);
  return out;
}
static void relabel_finish(SEXP out, const int64_t* conf, SEXP dims, const bnmf_relabel_info* info) {
  const int N = INTEGER(dims)[2];
  const int v[7] = {info->n_used, info->n_aligned, info->n_unmatched, info->rounds, info->converged, info->n_switched, info->n_changed_last};
  for (int i = 0; i < 7; ++i) SET_VECTOR_ELT(out, i, Rf_ScalarInteger(v[i]));
  SET_VECTOR_ELT(out, 7, Rf_ScalarReal(info->mean_cosine)); SET_VECTOR_ELT(out, 8, Rf_ScalarReal(info->min_cosine));
  SET_VECTOR_ELT(out, 9, Rf_ScalarReal((double)info->min_cosine_at + 1.0));   /* 1-based; 0 = none */
  SEXP pm = VECTOR_ELT(out, 10);
  int* a = INTEGER(pm);
  for (R_xlen_t i = 0; i < XLENGTH(pm); ++i) a[i] = a[i] < 0 ? NA_INTEGER : a[i] + 1;
  double* c = REAL(VECTOR_ELT(out, 12));
  for (int n = 0; n < N; ++n) for (int j = 0; j < N; ++j) c[n + (size_t)N * j] = (double)conf[(size_t)n * N + j];
}
SEXP C_bnmf_relabel(SEXP ptr, SEXP end_iter, SEXP n_samples, SEXP used, SEXP pivot_P, SEXP max_rounds, SEXP want_aligned, SEXP dims) {
  int32_t* u = NULL;
  const double* piv = NULL;
  SEXP out = PROTECT(relabel_alloc(n_samples, used, pivot_P, want_aligned, dims, &u, &piv));
  const int N = INTEGER(dims)[2];
  int64_t* conf = (int64_t*)R_alloc((size_t)N * N, sizeof(int64_t));
  bnmf_relabel_info info;
  if (end_iter == R_NilValue)
    chk(bnmf_relabel(get_handle(ptr), INTEGER(n_samples)[0], u, piv, INTEGER(max_rounds)[0], INTEGER(VECTOR_ELT(out, 10)), map_buf(out, 11), conf,
                     map_buf(out, 13), map_buf(out, 14), map_buf(out, 15), map_buf(out, 16), &info));
  else
    chk(bnmf_relabel_at(get_handle(ptr), INTEGER(end_iter)[0], INTEGER(n_samples)[0], u, piv, INTEGER(max_rounds)[0], INTEGER(VECTOR_ELT(out, 10)),
                        map_buf(out, 11), conf, map_buf(out, 13), map_buf(out, 14), map_buf(out, 15), map_buf(out, 16), &info));
  relabel_finish(out, conf, dims, &info);
  UNPROTECT(1);
  return out;
}
SEXP C_bnmf_relabel_at(SEXP ptr, SEXP end_iter, SEXP n_samples, SEXP used, SEXP pivot_P, SEXP max_rounds, SEXP want_aligned, SEXP dims) {
  int32_t* u = NULL;
  const double* piv = NULL;
  SEXP out = PROTECT(relabel_alloc(n_samples, used, pivot_P, want_aligned, dims, &u, &piv));
  const int N = INTEGER(dims)[2];
  int64_t* conf = (int64_t*)R_alloc((size_t)N * N, sizeof(int64_t));
  bnmf_relabel_info info;
  chk(bnmf_relabel_at(get_handle(ptr), INTEGER(end_iter)[0], INTEGER(n_samples)[0], u, piv, INTEGER(max_rounds)[0], INTEGER(VECTOR_ELT(out, 10)),
                      map_buf(out, 11), conf, map_buf(out, 13), map_buf(out, 14), map_buf(out, 15), map_buf(out, 16), &info));
  relabel_finish(out, conf, dims, &info);
  UNPROTECT(1);
  return out;
}
/* plot_label_switching's per-sample hungarian_assignment diagonal (R/postprocessing_visualizations.R:598-669):
 * C_bnmf_label_switching(ptr, iters (integer iteration numbers), reference_P (K x R), dims c(K,G,N)) ->
 * list(assigned N x n_iters (1-based column of reference_P, NA = "None"), cosine N x n_iters, included N x n_iters logical):
 * one column per iteration, factor k in row k */
SEXP C_bnmf_label_switching(SEXP ptr, SEXP iters, SEXP reference_P, SEXP dims) {
  const int n = (int)XLENGTH(iters), N = INTEGER(dims)[2], R = Rf_ncols(reference_P);
  static const char* nms[] = {"assigned", "cosine", "included"};
  SEXP out = PROTECT(named_list(3, nms));
  SEXP asg = PROTECT(Rf_allocMatrix(INTSXP, N, n)), cs = PROTECT(Rf_allocMatrix(REALSXP, N, n)), inc = PROTECT(Rf_allocMatrix(LGLSXP, N, n));
  chk(bnmf_label_switching(get_handle(ptr), INTEGER(iters), n, REAL(reference_P), R, INTEGER(asg), REAL(cs), LOGICAL(inc)));
  for (R_xlen_t i = 0; i < (R_xlen_t)N * n; ++i) INTEGER(asg)[i] = INTEGER(asg)[i] < 0 ? NA_INTEGER : INTEGER(asg)[i] + 1;
  SET_VECTOR_ELT(out, 0, asg); SET_VECTOR_ELT(out, 1, cs); SET_VECTOR_ELT(out, 2, inc);
  UNPROTECT(4);
  return out;
}
/* a chain's state in a file and back (bnmf_save_state / bnmf_load_state / bnmf_state_info): path is a character string */
static const char* path_arg(SEXP path) {
  if (XLENGTH(path) != 1) Rf_error("bnmf: path must be one character string");
  return CHAR(STRING_ELT(path, 0));
}
/* C_bnmf_save_state(ptr, path, since_iter): 0 = a full record (file created), S > 0 = a delta on a file that ends at iteration S;
 * returns the bytes written (double) */
SEXP C_bnmf_save_state(SEXP ptr, SEXP path, SEXP since_iter) {
  size_t bytes = 0;
  chk(bnmf_save_state(get_handle(ptr), path_arg(path), INTEGER(since_iter)[0], &bytes));
  return Rf_ScalarReal((double)bytes);
}
/* C_bnmf_load_state(ptr, path): into a handle fresh from C_bnmf_create / C_bnmf_create_f64 (instead of C_bnmf_init); returns the
 * iteration the handle is then at */
SEXP C_bnmf_load_state(SEXP ptr, SEXP path) {
  int it = 0;
  chk(bnmf_load_state(get_handle(ptr), path_arg(path), &it));
  return Rf_ScalarInteger(it);
}
/* C_bnmf_state_info(path) -> list(dims c(K,G,N), spec c(likelihood, prior, MH, learning_rank, rank_method, save_Z, window), seed,
 * chain_id, format_version, first_iter, last_iter, n_records, bytes) — no handle, no device */
SEXP C_bnmf_state_info(SEXP path) {
  bnmf_state_desc d;
  chk(bnmf_state_info(path_arg(path), &d));
  static const char* nms[] = {"dims", "spec", "seed", "chain_id", "format_version", "first_iter", "last_iter", "n_records", "bytes"};
  SEXP out = PROTECT(named_list(9, nms));
  SEXP dims = Rf_allocVector(INTSXP, 3);
  SET_VECTOR_ELT(out, 0, dims);
  INTEGER(dims)[0] = d.K; INTEGER(dims)[1] = d.G; INTEGER(dims)[2] = d.N;
  SEXP spec = Rf_allocVector(INTSXP, 7);
  SET_VECTOR_ELT(out, 1, spec);
  const int sv[7] = {d.likelihood, d.prior, d.MH, d.learning_rank, d.rank_method, d.save_Z, d.window};
  for (int i = 0; i < 7; ++i) INTEGER(spec)[i] = sv[i];
  SET_VECTOR_ELT(out, 2, Rf_ScalarReal((double)d.seed));
  SET_VECTOR_ELT(out, 3, Rf_ScalarInteger((int)d.chain_id));
  SET_VECTOR_ELT(out, 4, Rf_ScalarInteger(d.format_version));
  SET_VECTOR_ELT(out, 5, Rf_ScalarInteger(d.first_iter));
  SET_VECTOR_ELT(out, 6, Rf_ScalarInteger(d.last_iter));
  SET_VECTOR_ELT(out, 7, Rf_ScalarInteger(d.n_records));
  SET_VECTOR_ELT(out, 8, Rf_ScalarReal((double)d.bytes));
  UNPROTECT(1);
  return out;
}
SEXP C_bnmf_destroy(SEXP ptr) { handle_finalizer(ptr); return R_NilValue; }
SEXP C_bnmf_device_info(SEXP device) {
  char buf[512];
  chk(bnmf_device_info(INTEGER(device)[0], buf, sizeof buf));
  return Rf_mkString(buf);
}

static const R_CallMethodDef call_methods[] = {
  {"C_bnmf_create", (DL_FUNC)&C_bnmf_create, 7}, {"C_bnmf_create_f64", (DL_FUNC)&C_bnmf_create_f64, 7},
  {"C_bnmf_set_array", (DL_FUNC)&C_bnmf_set_array, 3},
  {"C_bnmf_get_array", (DL_FUNC)&C_bnmf_get_array, 3}, {"C_bnmf_init", (DL_FUNC)&C_bnmf_init, 1},
  {"C_bnmf_run", (DL_FUNC)&C_bnmf_run, 3}, {"C_bnmf_window", (DL_FUNC)&C_bnmf_window, 4},
  {"C_bnmf_get_iter", (DL_FUNC)&C_bnmf_get_iter, 1}, {"C_bnmf_map", (DL_FUNC)&C_bnmf_map, 4},
  {"C_bnmf_run_until", (DL_FUNC)&C_bnmf_run_until, 4}, {"C_bnmf_run_post_warmup", (DL_FUNC)&C_bnmf_run_post_warmup, 5},
  {"C_bnmf_assign", (DL_FUNC)&C_bnmf_assign, 8}, {"C_bnmf_map_at", (DL_FUNC)&C_bnmf_map_at, 5},
  {"C_bnmf_assign_at", (DL_FUNC)&C_bnmf_assign_at, 9}, {"C_bnmf_label_switching", (DL_FUNC)&C_bnmf_label_switching, 4},
  {"C_bnmf_destroy", (DL_FUNC)&C_bnmf_destroy, 1}, {"C_bnmf_device_info", (DL_FUNC)&C_bnmf_device_info, 1},
  {"C_bnmf_save_state", (DL_FUNC)&C_bnmf_save_state, 3}, {"C_bnmf_load_state", (DL_FUNC)&C_bnmf_load_state, 2},
  {"C_bnmf_state_info", (DL_FUNC)&C_bnmf_state_info, 1},
  {"C_bnmf_set_fixed", (DL_FUNC)&C_bnmf_set_fixed, 3}, {"C_bnmf_get_fixed", (DL_FUNC)&C_bnmf_get_fixed, 3},
  {"C_bnmf_waic", (DL_FUNC)&C_bnmf_waic, 7}, {"C_bnmf_waic_at", (DL_FUNC)&C_bnmf_waic_at, 7},
  {"C_bnmf_mixing", (DL_FUNC)&C_bnmf_mixing, 7}, {"C_bnmf_mixing_at", (DL_FUNC)&C_bnmf_mixing_at, 7},
  {"C_bnmf_ppc", (DL_FUNC)&C_bnmf_ppc, 6}, {"C_bnmf_ppc_at", (DL_FUNC)&C_bnmf_ppc_at, 6},
  {"C_bnmf_attribution", (DL_FUNC)&C_bnmf_attribution, 7}, {"C_bnmf_attribution_at", (DL_FUNC)&C_bnmf_attribution_at, 7},
  {"C_bnmf_project", (DL_FUNC)&C_bnmf_project, 9}, {"C_bnmf_project_at", (DL_FUNC)&C_bnmf_project_at, 9},
  {"C_bnmf_decompose", (DL_FUNC)&C_bnmf_decompose, 9}, {"C_bnmf_decompose_at", (DL_FUNC)&C_bnmf_decompose_at, 9},
  {"C_bnmf_relabel", (DL_FUNC)&C_bnmf_relabel, 8}, {"C_bnmf_relabel_at", (DL_FUNC)&C_bnmf_relabel_at, 8},
  {"C_bnmf_contrast", (DL_FUNC)&C_bnmf_contrast, 9}, {"C_bnmf_contrast_at", (DL_FUNC)&C_bnmf_contrast_at, 9},
  {"C_bnmf_regress", (DL_FUNC)&C_bnmf_regress, 9}, {"C_bnmf_regress_at", (DL_FUNC)&C_bnmf_regress_at, 9},
  {"C_bnmf_coactivity", (DL_FUNC)&C_bnmf_coactivity, 9}, {"C_bnmf_coactivity_at", (DL_FUNC)&C_bnmf_coactivity_at, 9},
  {"C_bnmf_stability", (DL_FUNC)&C_bnmf_stability, 8}, {"C_bnmf_stability_at", (DL_FUNC)&C_bnmf_stability_at, 8},
  {"C_bnmf_reconstruction", (DL_FUNC)&C_bnmf_reconstruction, 7}, {"C_bnmf_reconstruction_at", (DL_FUNC)&C_bnmf_reconstruction_at, 7},
  {"C_bnmf_similarity", (DL_FUNC)&C_bnmf_similarity, 9}, {"C_bnmf_similarity_at", (DL_FUNC)&C_bnmf_similarity_at, 9},
  {"C_bnmf_subtypes", (DL_FUNC)&C_bnmf_subtypes, 9}, {"C_bnmf_subtypes_at", (DL_FUNC)&C_bnmf_subtypes_at, 9},
  {"C_bnmf_residuals", (DL_FUNC)&C_bnmf_residuals, 6}, {"C_bnmf_residuals_at", (DL_FUNC)&C_bnmf_residuals_at, 6},
  {"C_bnmf_tradeoff", (DL_FUNC)&C_bnmf_tradeoff, 9}, {"C_bnmf_tradeoff_at", (DL_FUNC)&C_bnmf_tradeoff_at, 9},
  {"C_bnmf_prune", (DL_FUNC)&C_bnmf_prune, 6}, {"C_bnmf_prune_at", (DL_FUNC)&C_bnmf_prune_at, 6},
  {"C_bnmf_summary", (DL_FUNC)&C_bnmf_summary, 8}, {"C_bnmf_summary_at", (DL_FUNC)&C_bnmf_summary_at, 8},
  {NULL, NULL, 0}};
void R_init_bayesNMFhip(DllInfo* dll) {
  R_registerRoutines(dll, NULL, call_methods, NULL, NULL);
  R_useDynamicSymbols(dll, FALSE);
}
