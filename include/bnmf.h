/* include/bnmf.h — C ABI of libbnmf.so, the MI355X (gfx950) Gibbs engine for Bayesian NMF.
 *
 * This is the drop-in boundary.  The reference (jennalandy/bayesNMF, pure R) has no FFI;
 * the seam this library replaces is the body of the sampling loop
 *   R/bayesNMF_sampler.R:273-285  (sample_prior_params -> sample_params -> record_sample ->
 *                                  update_sample_metrics)
 * and the constructor's prior draws (R/bayesNMF_sampler.R:232-257).  An R `.Call` shim
 * (r/bnmf_shim.c) or Python ctypes (bayesnmf_amd/engine.py) binds exactly these symbols.
 *
 * Conventions
 *  - plain C types only; every matrix is column-major double exactly as R stores it:
 *    M[k+K*g], P[k+K*n], E[n+N*g], Z[k+K*(n+N*g)]; A is length N; R one value.
 *  - every function returns 0 on success, a negative BNMF_E* code otherwise; the message is
 *    available from bnmf_last_error() (thread-local).  No exceptions cross the boundary.
 *  - the caller owns every buffer it passes; the handle owns all device memory and one HIP
 *    stream.  One handle = one chain = one device.  Handles are independent.
 *  - there is NO CPU fallback: bnmf_create fails with BNMF_ENODEVICE when no gfx950 GPU is
 *    visible.
 */
#ifndef BNMF_H
#define BNMF_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define BNMF_VERSION 100
#define BNMF_NMETRIC 11   /* iter,RMSE,KL,loglikelihood,logposterior,n_params,BIC,rank,temp,
                             P_mean_acceptance_rate,E_mean_acceptance_rate
                             (state$sample_metrics columns, R/bayesNMF_sampler.R:190-207) */

enum { BNMF_OK = 0, BNMF_EINVAL = -1, BNMF_ESIZE = -2, BNMF_EUNSET = -3, BNMF_ENODEVICE = -4,
       BNMF_EHIP = -5, BNMF_EMODEL = -6, BNMF_ESTATE = -7 };

enum { BNMF_POISSON = 0, BNMF_NORMAL = 1 };                       /* likelihood */
enum { BNMF_TRUNCNORMAL = 0, BNMF_EXPONENTIAL = 1, BNMF_GAMMA = 2 }; /* prior */
enum { BNMF_SBFI = 0, BNMF_BFI = 1 };                             /* rank_method */

/* array ids for bnmf_set_array / bnmf_get_array / bnmf_window */
enum {
  BNMF_P = 0, BNMF_E = 1, BNMF_A = 2, BNMF_R = 3, BNMF_Z = 4, BNMF_ZSUMK = 5, BNMF_ZSUMG = 6,
  BNMF_SIGMASQ = 7,
  BNMF_ALPHA_P = 10, BNMF_BETA_P = 11, BNMF_ALPHA_E = 12, BNMF_BETA_E = 13,
  BNMF_MU_P = 14, BNMF_SIGMASQ_P = 15, BNMF_MU_E = 16, BNMF_SIGMASQ_E = 17,
  BNMF_LAMBDA_P = 18, BNMF_LAMBDA_E = 19, BNMF_ALPHA = 20, BNMF_BETA = 21,
  /* hyper-prior matrices (R/setup.R:15-88); n==1 means a scalar broadcast */
  BNMF_HA_P = 30, BNMF_HB_P = 31, BNMF_HC_P = 32, BNMF_HD_P = 33, BNMF_HM_P = 34, BNMF_HS_P = 35,
  BNMF_HA_E = 40, BNMF_HB_E = 41, BNMF_HC_E = 42, BNMF_HD_E = 43, BNMF_HM_E = 44, BNMF_HS_E = 45,
  BNMF_ACC_P = 50, BNMF_ACC_E = 51, BNMF_MHAT = 60, BNMF_ID_MAX = 64
};

/* Philox variable ids (counter word 3 of the stream spec) */
enum { BNMF_V_Z = 1, BNMF_V_P = 2, BNMF_V_E = 3, BNMF_V_BETA_P = 4, BNMF_V_ALPHA_P = 5,
       BNMF_V_BETA_E = 6, BNMF_V_ALPHA_E = 7, BNMF_V_MU_P = 8, BNMF_V_SIGSQ_P = 9,
       BNMF_V_MU_E = 10, BNMF_V_SIGSQ_E = 11, BNMF_V_LAMBDA_P = 12, BNMF_V_LAMBDA_E = 13,
       BNMF_V_A = 14, BNMF_V_R = 15, BNMF_V_MHU_P = 16, BNMF_V_MHU_E = 17, BNMF_V_SIGMASQ = 18,
       BNMF_V_YREP = 19 /* the replicates of bnmf_ppc: no draw of the chain */ };

typedef struct bnmf_handle bnmf_handle;

typedef struct {
  int32_t K, G, N;          /* dims (R/bayesNMF_sampler.R:141-145) */
  int32_t likelihood;       /* BNMF_POISSON | BNMF_NORMAL */
  int32_t prior;            /* BNMF_TRUNCNORMAL | BNMF_EXPONENTIAL | BNMF_GAMMA */
  int32_t MH;               /* Metropolis-Hastings within Gibbs (Poisson only) */
  int32_t learning_rank;    /* rank given as a range -> A, R sampled */
  int32_t rank_method;      /* BNMF_SBFI | BNMF_BFI */
  int32_t save_Z;           /* materialise Z (K x N x G int32) every iteration ("full mode") */
  int32_t window;           /* samples kept on device for bnmf_window (MAP_over, or all) */
  uint64_t seed;            /* Philox key = (seed_lo, seed_hi ^ chain_id) */
  uint32_t chain_id;
  int32_t device;           /* HIP device ordinal */
  const double* temperature;/* temperature_schedule, length n_temperature (may be NULL = all 1) */
  int64_t n_temperature;
} bnmf_config;

/* create: copies M (int32, column-major K x G) to the device.  Replaces the data/dims part of
 * bayesNMF_sampler$new (R/bayesNMF_sampler.R:140-145). */
int bnmf_create(const bnmf_config* cfg, const int32_t* M_colmajor, bnmf_handle** out);
/* create from real-valued data (double, column-major K x G), every cell checked on the host before any device call:
 *  BNMF_NORMAL   any finite value, negative ones included (NaN / +-Inf: BNMF_EINVAL naming the first bad cell [k, g]);
 *  BNMF_POISSON  whole numbers in [0, 2^31 - 1] only (anything else: BNMF_EINVAL, "non-integer count"), converted exactly,
 *                then as bnmf_create.
 * A Normal handle holds its data on the device as fp64 whichever entry point created it: integer data give the same chain, bit
 * for bit, through either. */
int bnmf_create_f64(const bnmf_config* cfg, const double* M_colmajor, bnmf_handle** out);
int bnmf_destroy(bnmf_handle* h);

/* set/get any array by id (column-major doubles; integer arrays are converted).  Hyper-prior
 * ids accept n==1 (scalar) — fill_matrix_ R/setup.R:102-113.  State arrays given before
 * bnmf_init are kept verbatim (init_prior_params / init_params, R/sample_priors.R:15-141,
 * R/sample_params.R:16-41); NaN entries mark "missing" and make that column n be re-drawn. */
int bnmf_set_array(bnmf_handle* h, int id, const double* colmajor, size_t n);
int bnmf_get_array(bnmf_handle* h, int id, double* colmajor_out, size_t n);
int bnmf_get_array_i32(bnmf_handle* h, int id, int32_t* out, size_t n);   /* Z, ZsumK, ZsumG */

/* Hold chosen columns of P fixed (refit to a known catalogue).  id must be BNMF_P, fixed[N] holds 0 / 1.  Iteration t of
 * a chain with a mask is the loop body with sample_Pn skipped for every n with fixed[n] = 1, nothing else changed: P[, n] keeps, bit for
 * bit, the value bnmf_set_array(BNMF_P) gave it (also while A[n] == 0: no prior redraw); every other draw keeps its Philox stream —
 * the P-side prior parameters of a fixed column go on being drawn, from the fixed P; Psum, the recorded samples, the log-prior and the
 * metrics are produced as always.  n_params stays sum(A) * (G + K): it is NOT reduced for fixed columns.  The BNMF_ACC_P entries of a
 * fixed column are never written: they stay as bnmf_init left them (no value, NaN), and P_mean_acceptance_rate averages them as before.
 * A mask of zeros, or no call, is the chain without the feature, bit for bit.  Call before bnmf_init / bnmf_load_state.
 *   bnmf_set_fixed refuses: id != BNMF_P with BNMF_EMODEL (fixing rows of E is out of scope), n != N with BNMF_ESIZE, a value other than
 *   0 / 1 with BNMF_EINVAL, a handle that has been initialised, loaded or run with BNMF_ESTATE (the column or value named).
 *   bnmf_init then refuses, on the host and before its first device write: a fixed column whose P[, n] was not set or holds NaN with
 *   BNMF_EUNSET; one with a negative or infinite entry or a column sum of 0 with BNMF_EINVAL.  Columns that are NOT fixed and carry a NaN
 *   in the supplied P are drawn from the prior at bnmf_init (without a mask a supplied P is kept whole, as before).
 *   bnmf_save_state writes the mask into the base record (only if a column is fixed: other chains write the bytes they always wrote);
 *   bnmf_load_state applies it, and refuses a handle that was given another mask with BNMF_ESTATE, the column named.
 * bnmf_get_fixed returns the mask (zeros if none was set); bnmf_get_stat(h, 8) the number of fixed columns. */
int bnmf_set_fixed(bnmf_handle* h, int id, const int32_t* fixed, size_t n);
int bnmf_get_fixed(bnmf_handle* h, int id, int32_t* out, size_t n);

/* constructor draws: prior params from hyper-priors unless supplied, then
 * sample_params(from_prior=TRUE), record iteration 1 and its metrics row
 * (R/bayesNMF_sampler.R:232-257).  metrics_row1 may be NULL. */
int bnmf_init(bnmf_handle* h, double* metrics_row1 /* BNMF_NMETRIC */);

/* n_iter iterations of the loop body (R/bayesNMF_sampler.R:273-285).  `converged` is
 * state$converged: it only matters for MH (accept-all before, true accept/reject after,
 * R/sample_Pn.R:199-204).  metrics_rowmajor: n_iter x BNMF_NMETRIC doubles (may be NULL). */
int bnmf_run(bnmf_handle* h, int n_iter, int converged, double* metrics_rowmajor);

/* last `last_n` recorded samples (<= window) of array `id`, oldest first:
 * out[last_n][len(id)] (record_sample, R/bayesNMF_sampler.R:651-672). */
int bnmf_window(bnmf_handle* h, int id, int last_n, double* out);

/* MAP estimate over the last `last_n` recorded samples, computed on the device (get_MAP_, R/utils.R:194-288;
 * get_mode / renormalize, R/helpers.R:35-79): mode of A over the window (ties: alphabetically first pattern, as
 * sort(table(.), decreasing = TRUE) gives); over the samples whose A equals the mode, P / colSums(P) and
 * E * colSums(P) are averaged element-wise (P_mean K x N, E_mean N x G, every factor; `final = TRUE` of the
 * reference is the caller dropping the factors with A_mode == 0); credible_interval in (0,1) also returns the
 * quantile(., type 7) bounds at (1 -+ credible_interval) / 2 (any of the four pointers may be NULL; <= 0: none);
 * used[last_n] flags the samples that entered (oldest first); top_A (5 x N, row-major) the most frequent patterns.
 * info.rmse / info.kl are compute_metrics_(P = MAP$P, A = MAP$A, E = MAP$E, MAP = TRUE) (R/utils.R:412-455). */
typedef struct {
  int32_t n_used;          /* samples whose A equals the mode */
  int32_t n_patterns;      /* distinct A patterns in the window */
  int32_t top_counts[5];   /* counts of the (up to) five most frequent patterns, descending */
  int32_t _pad;
  double rmse, kl;
} bnmf_map_info;
int bnmf_map(bnmf_handle* h, int last_n, double credible_interval, double* P_mean, double* E_mean,
             double* A_mode, double* top_A, double* P_lower, double* P_upper, double* E_lower,
             double* E_upper, int32_t* used, bnmf_map_info* info);
/* bnmf_map over any kept range (get_MAP_(end_iter, n_samples), R/utils.R:194-230): the n_samples recorded samples that end at
 * iteration end_iter, i.e. iterations end_iter - n_samples + 1 ... end_iter (used[n_samples], oldest first).  Every one must lie in
 * [max(1, iter - window + 1), iter], else BNMF_ESIZE.  bnmf_map(h, n, ...) is bnmf_map_at(h, iter, n, ...). */
int bnmf_map_at(bnmf_handle* h, int end_iter, int n_samples, double credible_interval, double* P_mean, double* E_mean,
                double* A_mode, double* top_A, double* P_lower, double* P_upper, double* E_lower, double* E_upper,
                int32_t* used, bnmf_map_info* info);

/* The sampling loop up to convergence as ONE call (run_gibbs_sampler, R/bayesNMF_sampler.R:268-330, warm-up part):
 * blocks of iterations up to the next MAP check; at a check get_MAP_ over the last MAP_over samples on the device,
 * update_MAP_metrics_ (R/utils.R:356-397) and check_convergence_ (R/convergence.R:60-154).
 *   metrics  [cap_rows][BNMF_NMETRIC]   one row per iteration run (n_rows returned)
 *   map_rows [cap_checks][BNMF_NMAPROW] one row per check: iter, RMSE, KL, loglikelihood, logposterior, n_params, BIC,
 *            rank, MAP_A_counts, mean_temp, P/E_mean_acceptance_rate (state$MAP_metrics columns), then percent change,
 *            inarow_no_change, inarow_no_best, inarow_na, converged after that check.
 * `st` carries state$prev_MAP_metric ... between calls (zero-initialise it for a fresh chain). */
#define BNMF_NMAPROW 17
typedef struct {
  int32_t MAP_over, MAP_every, Ninarow_nochange, Ninarow_nobest, miniters, maxiters;
  int32_t metric;                /* 0 loglikelihood, 1 logposterior, 2 RMSE, 3 KL, 4 BIC */
  int32_t _pad;
  double tol;
} bnmf_convergence_control;
typedef struct {
  int32_t converged, why /* 0 -, 1 "no change", 2 "no best", 3 "max iters" */, best_iter, inarow_na, inarow_no_change,
          inarow_no_best, have_prev, n_checks;
  double prev_MAP_metric, best_MAP_metric, prev_percent_change;
} bnmf_convergence_state;
int bnmf_run_until(bnmf_handle* h, const bnmf_convergence_control* cc, bnmf_convergence_state* st,
                   double* metrics_rowmajor, int cap_rows, int* n_rows, double* map_rows, int cap_checks,
                   int* n_checks);

/* The post-warm-up tail of the MH models as ONE call (R/bayesNMF_sampler.R:332-384): post_warmup more iterations with
 * state$converged = TRUE, i.e. true accept / reject in MH_Pn_poisson / MH_En_poisson (R/sample_Pn.R:199-248), a MAP check
 * (rows as in bnmf_run_until) whenever iter is a multiple of MAP_every and after the last iteration. */
int bnmf_run_post_warmup(bnmf_handle* h, const bnmf_convergence_control* cc, bnmf_convergence_state* st,
                         int post_warmup, double* metrics_rowmajor, int cap_rows, int* n_rows, double* map_rows,
                         int cap_checks, int* n_checks);

/* Posterior reference assignment (assign_signatures_ensemble_, R/postprocessing.R:175-341; hungarian_assignment,
 * pairwise_sim, R/helpers.R:218-398) over the recorded samples flagged in used[last_n] (MAP$idx; NULL = all):
 * cosine similarities of every sample's included signatures (keep[N] flags; NULL = all) with the reference catalogue
 * reference_P (K x R, column-major) and one Hungarian assignment per sample maximising the total cosine, both on the device,
 * votes[n + N*j] = sum over samples of the cosine of the pairs (n, j) chosen; assigned_ref[n] = which.max of the votes
 * (-1 for a signature that is not kept); MAP_P (K x N, may be NULL) -> MAP_cosine[n]; lower/upper_cosine[n] =
 * quantile(type 7) of the per-sample cosine between signature n and its assigned reference. */
int bnmf_assign(bnmf_handle* h, int last_n, const int32_t* used, const double* reference_P, int R,
                const int32_t* keep, const double* MAP_P, double credible_interval, double* votes,
                int32_t* assigned_ref, double* MAP_cosine, double* lower_cosine, double* upper_cosine);
/* bnmf_assign over any kept range: used[n_samples] flags iterations end_iter - n_samples + 1 ... end_iter (NULL = all); the range
 * rule and BNMF_ESIZE as for bnmf_map_at.  bnmf_assign(h, n, ...) is bnmf_assign_at(h, iter, n, ...). */
int bnmf_assign_at(bnmf_handle* h, int end_iter, int n_samples, const int32_t* used, const double* reference_P, int R,
                   const int32_t* keep, const double* MAP_P, double credible_interval, double* votes,
                   int32_t* assigned_ref, double* MAP_cosine, double* lower_cosine, double* upper_cosine);

/* The label-switching trace (plot_label_switching, R/postprocessing_visualizations.R:598-669): for every recorded iteration iters[i]
 * (each in [max(1, iter - window + 1), iter], else BNMF_ESIZE), the diagonal of hungarian_assignment(P_t, reference_P,
 * return_mat = TRUE, keep_all_est = TRUE) (R/helpers.R:287-398) over ALL N factors, included or not: the reference column that
 * maximises the total cosine and that cosine (the bits bnmf_assign votes with).  With N > R the factors left without a partner get
 * -1 and cosine 0.0 (the reference's "None" padding).  included[i][n] = (A_t[n] != 0).  Row-major [n_iters][N] outputs. */
int bnmf_label_switching(bnmf_handle* h, const int32_t* iters, int n_iters, const double* reference_P, int R,
                         int32_t* assigned /* [n_iters][N], 0-based column or -1 */, double* cosine /* [n_iters][N] */,
                         int32_t* included /* [n_iters][N], may be NULL */);

/* WAIC of a recorded range, on the device: over the recorded samples flagged in used[] (oldest first; NULL = all; they
 * should share one rank, e.g. bnmf_map's used[]) every cell (k, g) of the data gets the log-likelihood l_s of each sample's fit
 * P_s diag(A_s) E_s (the Poisson cell term of the loglikelihood metric with the 1e-6 clip, or dnorm(m, c, sqrt(sigmasq_s[g]), log = TRUE)),
 * lppd_kg = log mean_s exp(l_s) and p_kg = var_s(l_s) (n - 1 form).  col [3][G]: the sums over k of lppd, p and mean_s(l_s) per column;
 * cell [2][K*G] (column-major): lppd_kg, p_kg; either may be NULL.  info: the totals (elpd_waic = lppd - p_waic, waic = -2 elpd_waic,
 * mean_loglik = the mean over the used samples of the log-likelihood), se_elpd = sqrt(K G var_cells(lppd_kg - p_kg)), n_high_var = the
 * cells with p_kg > 0.4.  The sums are taken in a fixed order: the same call gives the same bits.  Read-only for the chain.
 * bnmf_waic_at: the n_samples iterations that end at end_iter; the range rule and BNMF_ESIZE as for bnmf_map_at;
 * bnmf_waic(h, n, ...) is bnmf_waic_at(h, iter, n, ...).  Refused before any device work: null info and a used[] value other than 0 / 1
 * (the index named) with BNMF_EINVAL, fewer than 2 used samples with BNMF_ESIZE, window = 0 or a poisoned handle with BNMF_ESTATE. */
typedef struct { int32_t n_used, n_high_var;
                 double lppd, p_waic, elpd_waic, waic /* -2 elpd_waic */, se_elpd, mean_loglik; } bnmf_waic_info;
int bnmf_waic(bnmf_handle*, int last_n, const int32_t* used /* [last_n], NULL = all */,
              double* col /* [3][G]: lppd, p_waic, mean_loglik per column; may be NULL */,
              double* cell /* [2][K*G] column-major: lppd_kg, p_kg; may be NULL */, bnmf_waic_info* info);
int bnmf_waic_at(bnmf_handle*, int end_iter, int n_samples, const int32_t* used, double* col, double* cell, bnmf_waic_info* info);

/* Mixing diagnostics of a recorded range, on the device: for every element of the renormalised P (K x N: P / colSums(P))
 * and E (N x G: E * colSums(P)), over the recorded samples flagged in used[] (oldest first; NULL = all), numbered s = 0 .. S-1.  A lag
 * counts used samples, not iterations: a used[] with gaps is treated as one contiguous series, as get_MAP_'s idx is.
 * P_out [BNMF_NMIX][K*N], E_out [BNMF_NMIX][N*G] (each row column-major as P and E; either may be NULL), the rows:
 *   0 mean   1 var (S - 1 form)   2 ess (Geyer's initial monotone sequence over the autocorrelations; tau floored at 1 / log10(S))
 *   3 mcse = sqrt(var / ess)   4 rhat (split R-hat: halves of S / 2 samples, an odd middle sample dropped)
 *   5 pairs (the Gammas summed; 0 for a series without variance)   6 exit (0: a Gamma was not positive; 1: the lags ran out)
 *   7 mean_a   8 var_a   9 mean_b   10 var_b (the halves' moments, from which a between-chain R-hat is combined on the host)
 * An element whose series is constant (every sample equal to the first: a fixed_P column, an MH element that never moved), has no
 * variance or holds a NaN gets ess = mcse = rhat = NaN, pairs = exit = 0 (its mean and var are still the formulas': rounding noise).  info: a sequential scan, element index ascending, P then E, over the elements of the factors with keep[n] != 0
 * (NULL = all): the counts, and the smallest ess / largest rhat of each side with the element index (column-major position in P / E;
 * the first index wins a tie, NaN entries are skipped, -1 and NaN if there is none).  The sums are taken in a fixed order: the same
 * call gives the same bits.  Read-only for the chain.
 * bnmf_mixing_at: the n_samples iterations that end at end_iter; the range rule and BNMF_ESIZE as for bnmf_map_at;
 * bnmf_mixing(h, n, ...) is bnmf_mixing_at(h, iter, n, ...).  Refused before any device work: null info and a used[] / keep[] value other
 * than 0 / 1 (the index named) with BNMF_EINVAL; fewer than 4 used samples (each half needs a variance) and more than
 * BNMF_MIXING_MAX_SAMPLES (one element's series must fit the 160 KB of LDS; never truncated) with BNMF_ESIZE; window = 0 or a poisoned
 * handle with BNMF_ESTATE. */
#define BNMF_NMIX 11
#define BNMF_MIXING_MAX_SAMPLES 13653     /* 160 KB / (8 B of the series + 4 B of the slot list) per sample */
#define BNMF_MIXING_LOW_ESS 100.0         /* n_low_ess counts ess < this; n_high_rhat counts rhat > the next: the published conventions */
#define BNMF_MIXING_HIGH_RHAT 1.01        /* (Vehtari, Gelman, Simpson, Carpenter, Buerkner 2021) */
typedef struct { int32_t n_used, n_half;
                 int64_t n_const, n_ran_out /* exit == 1 */, n_low_ess, n_high_rhat;
                 int64_t min_ess_P_at, min_ess_E_at, max_rhat_P_at, max_rhat_E_at;
                 double min_ess_P, min_ess_E, max_rhat_P, max_rhat_E; } bnmf_mixing_info;
int bnmf_mixing(bnmf_handle*, int last_n, const int32_t* used /* [last_n], NULL = all */, const int32_t* keep /* [N], NULL = all */,
                double* P_out /* [BNMF_NMIX][K*N], may be NULL */, double* E_out /* [BNMF_NMIX][N*G], may be NULL */, bnmf_mixing_info* info);
int bnmf_mixing_at(bnmf_handle*, int end_iter, int n_samples, const int32_t* used, const int32_t* keep, double* P_out, double* E_out,
                   bnmf_mixing_info* info);

/* Posterior predictive checks of a recorded range, on the device: for every recorded sample flagged in used[] (oldest first;
 * NULL = all) a replicate y_s of the data is drawn from the sample's own fit c_s = P_s diag(A_s) E_s — Poisson(max(c_s, 1e-6)) by the
 * stream spec's rpois, or c_s + sqrt(sigmasq_s[g]) * a standard normal — on the stream (BNMF_V_YREP, element k + K g, the sample's
 * iteration) under the handle's key: the replicate of a cell and iteration is the same whichever range, used[] or call asks for it, and
 * the chain's own streams are not consumed.  Two discrepancies, each evaluated on the data and on the replicate against the same fit:
 *   Poisson  T1 = sum_k (sqrt(x) - sqrt(lambda))^2 (Freeman-Tukey)   T2 = the number of cells with x == 0
 *   Normal   T1 = sum_k z^2, z = (x - c_s) / sd                       T2 = max_k |z|
 * col [BNMF_PPC_NCOL][G]: per column the mean over the used samples of T on the data, of T on the replicate, and p = #(T_rep >= T_obs) / S,
 *   T1 in rows 0-2, T2 in rows 3-5 (a p near 0: the data of that column fit better than the model's own replicates do, near 1 the reverse;
 *   for T1 a column the model reconstructs badly has p near 0).
 * cell [4][K*G] (column-major): the mean and variance (S - 1 form) of the replicates, p_less = #(y < m) / S, p_equal = #(y == m) / S; the
 *   mid-PIT of a cell is p_less + 0.5 p_equal.
 * series [4][S]: the whole-matrix T1_obs, T1_rep, T2_obs, T2_rep of every used sample (sums over the columns; the maximum for the Normal T2).
 * info: p_T1 / p_T2 = the fraction of used samples whose whole-matrix T_rep >= T_obs, the means of the four series, n_tail_cells = the
 *   cells whose mid-PIT lies outside [0.025, 0.975].  col, cell and series may each be NULL.  Every sum is taken in a fixed order: the same
 *   call gives the same bits.  Read-only for the chain.
 * bnmf_ppc_at: the n_samples iterations that end at end_iter; the range rule and BNMF_ESIZE as for bnmf_map_at;
 * bnmf_ppc(h, n, ...) is bnmf_ppc_at(h, iter, n, ...).  Refused before any device work: null info and a used[] value other than 0 / 1
 * (the index named) with BNMF_EINVAL, fewer than 2 used samples with BNMF_ESIZE, window = 0 or a poisoned handle with BNMF_ESTATE. */
#define BNMF_PPC_NCOL 6   /* per T: mean T_obs, mean T_rep, p = #(T_rep >= T_obs)/S; T1 rows 0-2, T2 rows 3-5 */
typedef struct { int32_t n_used; int64_t n_tail_cells;   /* mid-PIT outside [0.025, 0.975] */
                 double p_T1, p_T2, mean_T1_obs, mean_T1_rep, mean_T2_obs, mean_T2_rep; } bnmf_ppc_info;
int bnmf_ppc(bnmf_handle*, int last_n, const int32_t* used, double* col /* [6][G] */, double* cell /* [4][K*G]: mean, var, p_less, p_equal */,
             double* series /* [4][S]: whole-matrix T1_obs, T1_rep, T2_obs, T2_rep per used sample */, bnmf_ppc_info* info);
int bnmf_ppc_at(bnmf_handle*, int end_iter, int n_samples, const int32_t* used, double* col, double* cell, double* series, bnmf_ppc_info* info);

/* Signature attribution of a recorded range, on the device: for every recorded sample flagged in used[] (oldest first;
 * NULL = all) the share of factor n in cell (k, g) is r_n = f_n / sum_n' f_n', f_n = P_s[k,n] A_s[n] E_s[n,g] (0 where the fit of the
 * cell is 0), and the mutations of the cell attributed to it x_n = m_kg r_n, the mean of the allocation Z given the sample (Normal
 * likelihood: x_n = f_n, the component of the fit; real-valued data are not allocated).  a_s[n,g] = sum_k x_n is the load of signature n
 * in tumour g under sample s.
 * load [BNMF_ATTR_NLOAD][N*G], each row laid out as E (n + N g): over the used samples the mean and the variance (S - 1 form) of a_s, the
 *   mean of a_s[n,g] / sum_n' a_s[n',g], and #(a_s >= min_load) / S: the probability that the signature is present in the tumour.
 * prob [K*N*G], laid out as Z (k + K (n + N g)): the mean over the used samples of r_n, the probability that a mutation of type k in
 *   tumour g came from signature n.
 * series [S][N] row-major: the cohort's load of every signature per used sample (a_s summed over the tumours).
 * info: total = the mean over the samples of the whole cohort's load (Poisson: close to the sum of the data), n_present = the (n, g)
 *   whose probability of presence is >= 0.5.  load, prob and series may each be NULL.  Factor n is taken to be the same signature in
 *   every sample, as bnmf_map takes it when it averages P and E element-wise.  Every sum is taken in a fixed order: the same call
 *   gives the same bits.  Read-only for the chain.
 * bnmf_attribution_at: the n_samples iterations that end at end_iter; the range rule and BNMF_ESIZE as for bnmf_map_at;
 * bnmf_attribution(h, n, ...) is bnmf_attribution_at(h, iter, n, ...).  Refused before any device work: null info, a used[] value other
 * than 0 / 1 (the index named) and a min_load that is NaN, infinite or negative with BNMF_EINVAL, fewer than 2 used samples with
 * BNMF_ESIZE, window = 0 or a poisoned handle with BNMF_ESTATE. */
#define BNMF_ATTR_NLOAD 4   /* load rows: mean, variance, mean share, probability of presence */
typedef struct { int32_t n_used, _pad; int64_t n_present; double min_load, total; } bnmf_attr_info;
int bnmf_attribution(bnmf_handle*, int last_n, const int32_t* used, double min_load,
                     double* load   /* [BNMF_ATTR_NLOAD][N*G], each row laid out as E (n + N g); may be NULL */,
                     double* prob   /* [K*N*G], laid out as Z (k + K (n + N g)); may be NULL */,
                     double* series /* [S][N] row-major; may be NULL */, bnmf_attr_info* info);
int bnmf_attribution_at(bnmf_handle*, int end_iter, int n_samples, const int32_t* used, double min_load,
                        double* load, double* prob, double* series, bnmf_attr_info* info);

/* Exposures of new tumours under the recorded signatures, on the device: X (K x J, column-major; counts or any
 * non-negative real values) is a second set of tumours — a validation cohort, one patient, a bootstrap of the data.  For every recorded
 * sample flagged in used[] (oldest first; NULL = all) every column of X is refitted to the sample's renormalised signatures
 * x[k,n] = P_s[k,n] / colSums(P_s)[n] by n_steps steps of the KL multiplicative update (EM), started from equal exposures that sum to the
 * column's total; a factor with A_s[n] == 0 or an all-zero column takes no part and has exposure +0.0.  No random number is drawn.
 * load [BNMF_PROJ_NLOAD][N*J], each row laid out as E (n + N j): over the used samples the mean and the variance (S - 1 form) of the
 *   exposure e_s[n,j], the mean of e_s[n,j] / sum_n' e_s[n',j], and #(e_s >= min_load) / S: bnmf_attribution's four rows.
 * fit [BNMF_PROJ_NFIT][J]: per new tumour the mean over the used samples of the cosine between the column and its fit x e (NaN where a
 *   sample's cosine is: an all-zero column, or a sample without factors), the mean of sum_k |X - x e| / sum_k X, and the largest over
 *   the samples of max_n |e_n(last step) - e_n(the step before)| / sum_k X: how far from converged n_steps left the refit.
 * series [S][N] row-major: the exposures summed over the new tumours, per used sample.
 * exposures [S][N*J]: every used sample's exposures, each laid out as E (caller-sized; they leave the device in batches).
 * info: total and n_present as bnmf_attribution's; max_rel_change the largest entry of fit row 2; min_cosine the smallest entry of fit
 *   row 0 that is not NaN and min_cosine_at its j (the first wins a tie; NaN and -1 if there is none).
 * load, fit, series and exposures may each be NULL.  Only + * /, sqrt and comparisons in a fixed order: the same call gives the same
 * bits, whatever the batches and wherever a tumour stands in X.  Read-only for the chain; none of its streams is consumed.
 * bnmf_project_at: the n_samples iterations that end at end_iter; the range rule and BNMF_ESIZE as for bnmf_map_at;
 * bnmf_project(h, n, ...) is bnmf_project_at(h, iter, n, ...).  Refused before any device work: null info or X, a used[] value other than
 * 0 / 1 (the index named), J < 1, n_steps outside 1..100000, a min_load that is NaN, infinite or negative, a cell of X that is NaN,
 * infinite or negative (the first bad cell [k, j] named) with BNMF_EINVAL; the Normal likelihood with BNMF_EMODEL (its refit is a
 * different algorithm); fewer than 2 used samples or N > BNMF_PROJ_MAX_N with BNMF_ESIZE; window = 0 or a poisoned handle with
 * BNMF_ESTATE. */
#define BNMF_PROJ_NLOAD 4      /* load rows: mean, variance (S - 1 form), mean share, probability of presence: bnmf_attribution's */
#define BNMF_PROJ_NFIT  3      /* fit rows per new tumour: mean cosine, mean relative L1 error, largest last-step change */
#define BNMF_PROJ_MAX_N 128
typedef struct { int32_t n_used, n_steps; int64_t n_present; double min_load, total, max_rel_change, min_cosine;
                 int64_t min_cosine_at /* j; -1 if none */; } bnmf_project_info;
int bnmf_project(bnmf_handle*, int last_n, const int32_t* used, const double* X /* K x J column-major */, int J, int n_steps,
                 double min_load, double* load /* [4][N*J], rows laid out as E: n + N j */, double* fit /* [3][J] */,
                 double* series /* [S][N] */, double* exposures /* [S][N*J], each sample laid out as E */, bnmf_project_info* info);
int bnmf_project_at(bnmf_handle*, int end_iter, int n_samples, const int32_t* used, const double* X, int J, int n_steps,
                    double min_load, double* load, double* fit, double* series, double* exposures, bnmf_project_info* info);

/* Decomposition of the recorded signatures into a reference catalogue, on the device: is factor n a mixture of known
 * signatures?  reference_P (K x R, column-major; finite, not negative, no all-zero column) is normalised to unit column sums on the host.
 * For every recorded sample flagged in used[] (oldest first; NULL = all) and every factor n with keep[n] != 0 (NULL = all), A_s[n] != 0 and
 * a positive column sum, the renormalised column y = P_s[, n] / colSums(P_s)[n] is refitted to the catalogue by n_steps steps of the KL
 * multiplicative update (EM) from equal weights; then every reference whose weight is below min_share of the column's total is dropped
 * for good (the largest stays if none reaches it) and n_steps more steps refit the rest.  min_share == 0 skips the pruning and the second
 * stage.  A factor that takes no part in a sample has every weight +0.0 there, a NaN cosine and nactive 0; its column is never read.  No
 * random number is drawn.
 * weight [BNMF_DEC_NW][R*N], each row laid out r + R n: over the used samples the mean and the variance (S - 1 form) of the weight
 *   w_s[r,n], the mean of w_s[r,n] / sum_r' w_s[r',n], and #(w_s >= min_share) / S: the probability that reference r is part of factor n.
 * fit [BNMF_DEC_NFIT][N]: per factor the mean over the used samples of the cosine between y and its fit z w (NaN where a sample's is:
 *   a sample in which the factor takes no part), the mean of sum_k |y - z w| / sum_k y, and the largest over the samples of
 *   max_r |w_r(last step) - w_r(the step before)| / sum_k y: how far from converged n_steps left the refit.
 * nactive [S][N] row-major: the references left after the pruning, per used sample and factor.
 * included [N]: the used samples in which the factor took part.  A sample that excludes a factor enters its means with +0.0: flag in
 *   used[] the samples of one rank pattern (bnmf_map's used[]), as for bnmf_waic.
 * weights [S][R*N]: every used sample's weights, each laid out r + R n (caller-sized; they leave the device in batches).
 * info: n_present the (r, n) whose probability is >= 0.5; max_rel_change the largest entry of fit row 2; min_cosine the smallest entry of
 *   fit row 0 that is not NaN and min_cosine_at its n (the first wins a tie; NaN and -1 if there is none).
 * weight, fit, nactive, included and weights may each be NULL.  Only + * /, sqrt and comparisons in a fixed order: the same call gives the
 * same bits, whatever the batches.  Any likelihood: only P and A are read.  Read-only for the chain; none of its streams is consumed.
 * bnmf_decompose_at: the n_samples iterations that end at end_iter; the range rule and BNMF_ESIZE as for bnmf_map_at;
 * bnmf_decompose(h, n, ...) is bnmf_decompose_at(h, iter, n, ...).  Refused before any device work: null info or reference_P, a used[] or
 * keep[] value other than 0 / 1 (the index named), R outside 1..BNMF_DEC_MAX_R, n_steps outside 1..100000, a min_share that is NaN,
 * infinite, negative or >= 1, a cell of reference_P that is NaN, infinite or negative (the first bad cell [k, r] named), an all-zero column
 * of it (the column named) with BNMF_EINVAL; fewer than 2 used samples with BNMF_ESIZE; window = 0, a poisoned handle or nothing recorded
 * with BNMF_ESTATE. */
#define BNMF_DEC_NW 4        /* weight rows: mean, variance (S - 1), mean share, P(w >= min_share) */
#define BNMF_DEC_NFIT 3      /* per factor: mean cosine, mean relative L1, largest last-step change */
#define BNMF_DEC_MAX_R 128
typedef struct { int32_t n_used, n_steps, R, _pad; int64_t n_present /* (r, n) with P >= 0.5 */;
                 double min_share, max_rel_change, min_cosine; int64_t min_cosine_at /* n; -1 if none */; } bnmf_decompose_info;
int bnmf_decompose(bnmf_handle*, int last_n, const int32_t* used, const double* reference_P /* K x R column-major */, int R, const int32_t* keep,
                   int n_steps, double min_share,
                   double* weight   /* [4][R*N], each row r + R n; may be NULL */,
                   double* fit      /* [3][N]; may be NULL */,
                   int32_t* nactive /* [S][N] row-major; may be NULL */,
                   int32_t* included/* [N]; may be NULL */,
                   double* weights  /* [S][R*N], every sample's weights, r + R n; may be NULL; leaves the device in batches */,
                   bnmf_decompose_info* info);
int bnmf_decompose_at(bnmf_handle*, int end_iter, int n_samples, const int32_t* used, const double* reference_P, int R, const int32_t* keep,
                      int n_steps, double min_share, double* weight, double* fit, int32_t* nactive, int32_t* included, double* weights,
                      bnmf_decompose_info* info);

/* Group contrasts of exposures over a recorded range, on the device: does the activity of a signature differ between groups
 * of tumours?  groups [G] labels every tumour 0 .. C-1 (C = 1 + the largest label, every label in between with a member) or -1 = left
 * out.  For every recorded sample flagged in used[] (oldest first; NULL = all), s = 0 .. S-1, with cs_s = colSums(P_s):
 *   x_s[n,g] = A_s[n] != 0 ? E_s[n,g] cs_s[n] : +0.0, bnmf_map's renormalised exposure: the mutations of tumour g expected from signature n;
 *   t = sum_n x_s[n,g];  the share r = x / t (0 where t is not positive);  the presence flag b = (x >= min_load).
 *   Per group c of m_c tumours and factor n: v0 = the mean load (the group mean of x), v1 = the mean share (of r), v2 = the prevalence
 *   #(b) / m_c, each sum in the canonical W = 64 order of bnmf_mixing over the members in ascending tumour order.
 * The S values of v_q[n,c] are draws from the posterior of that group statistic; the difference of two groups then has a posterior too.
 * group [BNMF_CON_NSTAT][BNMF_CON_NGROW][N*C], each row laid out n + N c: per statistic q over the used samples the mean, the variance
 *   (S - 1 form) and the type-7 quantiles at (1 -+ credible_interval) / 2 of v_q[n,c].
 * pair [BNMF_CON_NSTAT][BNMF_CON_NPROW][N*NP], each row n + N p: NP = C (C - 1) / 2 pairs (a, b), a < b, numbered with a ascending, then b
 *   ascending; the same four rows of d_s = v_q[n,a] - v_q[n,b], then p_greater = #(d_s > 0) / S and p_less = #(d_s < 0) / S.  With C = 1
 *   there is no pair and pair is not written.
 * series [BNMF_CON_NSTAT][S][N*C]: v_q per used sample, each laid out n + N c.   sizes [C]: m_c.
 * info: n_credible[q] = the (n, p) whose interval excludes 0 (lower > 0 or upper < 0); n_left_out = the tumours labelled -1.
 * credible_interval <= 0 means no interval: the rows lower / upper are NaN and n_credible is 0.  group, pair, series and sizes may each be
 * NULL.  Factor n is taken to be the same signature in every sample, as bnmf_map takes it.  Only + - * /, comparisons and integer counts
 * in a fixed order: the same call gives the same bits; renumbering the groups permutes the outputs.  Any likelihood and prior: only P (its
 * column sums), E and A are read.  Read-only for the chain; none of its streams is consumed and no random number is drawn.
 * bnmf_contrast_at: the n_samples iterations that end at end_iter; the range rule and BNMF_ESIZE as for bnmf_waic_at;
 * bnmf_contrast(h, n, ...) is bnmf_contrast_at(h, iter, n, ...).  Refused before any device work: null info or groups, a used[] value other
 * than 0 / 1 (the index named), a label below -1 or >= BNMF_CON_MAX_GROUPS (the tumour named), a group 0 .. C-1 without a member (the group
 * named), no tumour in any group, a min_load that is NaN, infinite or negative, a credible_interval that is NaN or >= 1 with BNMF_EINVAL;
 * fewer than 2 used samples with BNMF_ESIZE; window = 0, a poisoned handle or nothing recorded with BNMF_ESTATE. */
#define BNMF_CON_MAX_GROUPS 64
#define BNMF_CON_NSTAT 3    /* 0 load, 1 share, 2 prevalence */
#define BNMF_CON_NGROW 4    /* group rows: mean, variance (S - 1 form), lower, upper */
#define BNMF_CON_NPROW 6    /* pair rows: mean, variance, lower, upper, p_greater, p_less */
typedef struct { int32_t n_used, n_groups, n_pairs, n_left_out; int64_t n_credible[BNMF_CON_NSTAT];
                 double min_load, credible_interval; } bnmf_contrast_info;
int bnmf_contrast(bnmf_handle*, int last_n, const int32_t* used, const int32_t* groups /* [G]: 0..C-1, -1 = left out */,
                  double min_load, double credible_interval,
                  double* group  /* [3][4][N*C], each row laid out n + N c; may be NULL */,
                  double* pair   /* [3][6][N*NP], each row n + N p; may be NULL */,
                  double* series /* [3][S][N*C]; may be NULL */,
                  int32_t* sizes /* [C]; may be NULL */, bnmf_contrast_info* info);
int bnmf_contrast_at(bnmf_handle*, int end_iter, int n_samples, const int32_t* used, const int32_t* groups, double min_load,
                     double credible_interval, double* group, double* pair, double* series, int32_t* sizes, bnmf_contrast_info* info);

/* Regression of exposures on tumour covariates over a recorded range, on the device: does the activity of a signature follow
 * age, dose or purity, and is a group difference still there once other covariates are in the model?  design [G x Q] column-major, one row
 * per tumour, Q in 1 .. BNMF_REG_MAX_Q; it is taken as given: the caller supplies the column of ones.  include [G] holds 0 / 1 (NULL = all):
 * the m included tumours g_0 < g_1 < ...; the design cells of the others are not read.  For every recorded sample flagged in used[] (oldest
 * first; NULL = all), s = 0 .. S-1, with x_s[n,g], t and u = t > 0 ? 1 / t : 0.0 as for bnmf_contrast, the three responses are
 *   y0 = x the load,   y1 = x u the share,   y2 = sqrt(x) the variance-stabilised load,
 * and per (s, response q, factor n) the call solves the least-squares problem min_beta sum_i (y_i - sum_j design[g_i,j] beta_j)^2 by the
 * normal equations: canonB is the blocked canonical sum over the included tumours in ascending order (blocks of BNMF_REG_BLOCK members, a
 * block the canonical W = 64 sum of bnmf_mixing, the blocks added in order from +0.0);  Gm[j][k] = canonB(design[g_i,j] design[g_i,k]) and its
 * Cholesky factor L (on the host, once per call);  w_j = canonB(y_i design[g_i,j]),  sy = canonB(y_i);  L z = w,  L' beta = z;  yhat_i = sum_j
 * design[g_i,j] beta_j;  rss = canonB((y_i - yhat_i)^2),  tss = canonB((y_i - sy / m)^2),  r2 = tss > 0 ? 1 - rss / tss : NaN,  sigma2 = rss / (m - Q).
 * A factor the sample excludes has y = +0.0: beta = 0, r2 = NaN.  sqrt of a negative load (real-valued data) is NaN by IEEE and stays one.
 * The S values of beta_j are draws from the posterior of the cohort's own least-squares coefficient, the finite-population quantity, as
 * bnmf_contrast's group means are: the sampling error of the tumours as a sample of a population is NOT added.
 * coef [BNMF_REG_NSTAT][BNMF_REG_NCROW][N*Q], each row laid out n + N j: over the used samples the mean, the variance (S - 1 form), the type-7
 *   quantiles at (1 -+ credible_interval) / 2 of beta_j, p_greater = #(beta_j > 0) / S and p_less = #(beta_j < 0) / S.
 * fit [BNMF_REG_NSTAT][BNMF_REG_NFIT][N]: the mean and the two quantiles of r2 over the samples whose r2 is not NaN, their number (NaN, NaN,
 *   NaN, 0 without one), and the mean of sigma2 over all used samples.
 * coef_series [BNMF_REG_NSTAT][S][N*Q]: beta per used sample, each n + N j.   r2_series [BNMF_REG_NSTAT][S][N].
 * info: n_credible[q][j] = the factors whose interval for column j excludes 0 (lower > 0 or upper < 0), per column so that the intercept
 *   does not drown the covariates;  min_pivot_ratio = min_j d_j / Gm[j][j] over the Cholesky pivots d_j and min_pivot_at its j: how close to
 *   collinear the design is (1 for orthogonal columns, towards 0 for a nearly dependent one);  n_blocks = ceil(m / BNMF_REG_BLOCK).
 * credible_interval <= 0 means no interval: lower / upper are NaN and n_credible is 0.  coef, fit, coef_series and r2_series may each be
 * NULL.  Only + - * /, sqrt, comparisons and integer counts in a fixed order: the bits depend on the recorded samples, used, design,
 * include and credible_interval alone; scaling a design column by a power of two divides its beta by it exactly; leaving tumours out
 * through include gives the bits of a chain and design without them.  Read-only for the chain; no random number is drawn.
 * bnmf_regress_at: the n_samples iterations that end at end_iter; the range rule and BNMF_ESIZE as for bnmf_waic_at;
 * bnmf_regress(h, n, ...) is bnmf_regress_at(h, iter, n, ...).  Refused before any device work: null info or design, a used[] or include[]
 * value other than 0 / 1 (the index named), Q outside 1 .. BNMF_REG_MAX_Q, a NaN or infinite design cell of an included tumour (the cell
 * named), a credible_interval that is NaN or >= 1 with BNMF_EINVAL; fewer than 2 used samples or m <= Q with BNMF_ESIZE; a design not of
 * full column rank (a pivot d_j that is not > 0 or not finite; the column named, no threshold) with BNMF_EINVAL; window = 0, a poisoned
 * handle or nothing recorded with BNMF_ESTATE. */
#define BNMF_REG_MAX_Q 16
#define BNMF_REG_BLOCK 1024
#define BNMF_REG_NSTAT 3   /* 0 load, 1 share, 2 sqrt(load) */
#define BNMF_REG_NCROW 6   /* coef rows: mean, variance (S - 1), lower, upper, p_greater, p_less */
#define BNMF_REG_NFIT  5   /* fit rows per factor: mean r2, lower r2, upper r2, samples with an r2, mean sigma2 */
typedef struct { int32_t n_used, Q, n_included, n_left_out, n_blocks, min_pivot_at;
                 int64_t n_credible[BNMF_REG_NSTAT][BNMF_REG_MAX_Q];
                 double credible_interval, min_pivot_ratio; } bnmf_regress_info;
int bnmf_regress(bnmf_handle*, int last_n, const int32_t* used, const double* design /* G x Q column-major */, int Q,
                 const int32_t* include /* [G] 0 / 1, NULL = all */, double credible_interval,
                 double* coef        /* [3][6][N*Q], each row n + N j; may be NULL */,
                 double* fit         /* [3][5][N]; may be NULL */,
                 double* coef_series /* [3][S][N*Q]; may be NULL */,
                 double* r2_series   /* [3][S][N]; may be NULL */, bnmf_regress_info* info);
int bnmf_regress_at(bnmf_handle*, int end_iter, int n_samples, const int32_t* used, const double* design, int Q, const int32_t* include,
                    double credible_interval, double* coef, double* fit, double* coef_series, double* r2_series, bnmf_regress_info* info);

/* Co-activity of signatures over a recorded range, on the device: do two signatures act in the same tumours or exclude each
 * other, and is a signature split into two factors (a high cosine of two columns of P whose exposures are negatively correlated)?  include
 * [G] holds 0 / 1 (NULL = all): the m included tumours g_0 < g_1 < ..., the member list of bnmf_regress.  NP = N (N - 1) / 2 pairs (a, b),
 * a < b, numbered with a ascending, then b ascending (bnmf_contrast's numbering of its pairs of groups).  For every recorded sample flagged
 * in used[] (oldest first; NULL = all), s = 0 .. S-1, with x_s[n,g] as for bnmf_contrast and canonB the blocked canonical sum of
 * bnmf_regress over the members, four statistics per pair:
 *   v0 Pearson:   mu_n = canonB(x[n,g_i]) / m;  d_n,i = x[n,g_i] - mu_n;  S_ab = canonB(d_a,i d_b,i);
 *                 v0 = S_aa S_bb > 0 ? S_ab / sqrt(S_aa S_bb) : NaN.
 *   v1 Spearman:  c_n,i = 2 #(x_j < x_i) + #(x_j == x_i) - m  (twice the midrank less m + 1; values compared as doubles, -0.0 == +0.0);
 *                 T_ab = sum_i c_a,i c_b,i in int64;  v1 = T_aa > 0 && T_bb > 0 ? (double)T_ab / sqrt((double)T_aa (double)T_bb) : NaN;
 *                 a factor with a load that is not finite among its included tumours has v1 = NaN in that sample.
 *   v2 co-presence: with b_n,i = (x[n,g_i] >= min_load) and the 2 x 2 counts n11, n10, n01, n00 the phi coefficient
 *                 ((double)n11 n00 - (double)n10 n01) / sqrt(((double)n1. n0.) ((double)n.1 n.0)), NaN when a margin is 0.
 *   v3 cosine:    of the raw columns P_s[, a] and P_s[, b]: dot, nn_a, nn_b summed over k ascending from +0.0, dot / sqrt(nn_a nn_b); NaN
 *                 when A_s excludes a or b.
 * pair [BNMF_COA_NSTAT][BNMF_COA_NPROW][NP]: per statistic and pair over the S' samples whose value is not NaN the mean, the variance
 *   (S' - 1 form, NaN with S' < 2), the type-7 quantiles at (1 -+ credible_interval) / 2, p_greater = #(v > 0) / S', p_less = #(v < 0) / S'
 *   and n_valid = S'; with S' = 0 the first six rows are NaN.   series [BNMF_COA_NSTAT][S][NP]: every v, NaN included.
 * info: n_credible[q] (q < 3) = the pairs whose interval excludes 0 (lower > 0 or upper < 0; unadjusted for the number of pairs);
 *   max_cosine and max_cosine_at = the largest mean cosine and its pair (the first wins a tie; NaN and -1 without one);
 *   n_blocks = ceil(m / BNMF_REG_BLOCK).
 * credible_interval <= 0 means no interval: lower / upper are NaN and n_credible is 0.  pair and series may each be NULL.  Only + - * /,
 * sqrt, comparisons and whole numbers in a fixed order: the bits depend on the recorded samples, used, include, min_load and
 * credible_interval alone.  Works for every likelihood and prior; read-only for the chain; no random number is drawn.
 * bnmf_coactivity_at: the n_samples iterations that end at end_iter; the range rule and BNMF_ESIZE as for bnmf_waic_at;
 * bnmf_coactivity(h, n, ...) is bnmf_coactivity_at(h, iter, n, ...).  Refused before any device work: null info, a used[] or include[]
 * value other than 0 / 1 (the index named), a min_load that is NaN, infinite or negative, a credible_interval that is NaN or >= 1 with
 * BNMF_EINVAL; N < 2, fewer than 2 used samples, m < 3 or m > BNMF_COA_MAX_M (4 m^3 stays inside int64) with BNMF_ESIZE; window = 0, a
 * poisoned handle or nothing recorded with BNMF_ESTATE. */
#define BNMF_COA_NSTAT 4         /* 0 pearson, 1 spearman, 2 co-presence (phi), 3 cosine of the columns of P */
#define BNMF_COA_NPROW 7         /* pair rows: mean, variance, lower, upper, p_greater, p_less, n_valid */
#define BNMF_COA_MAX_M 1000000
typedef struct { int32_t n_used, n_included, n_left_out, n_pairs, n_blocks, _pad;
                 int64_t n_credible[3];      /* q0..q2: pairs whose interval excludes 0 (unadjusted) */
                 int64_t max_cosine_at;      /* pair with the largest mean cosine; first wins a tie; -1 if none */
                 double max_cosine, min_load, credible_interval; } bnmf_coactivity_info;
int bnmf_coactivity(bnmf_handle*, int last_n, const int32_t* used, const int32_t* include /* [G] 0 / 1, NULL = all */,
                    double min_load, double credible_interval,
                    double* pair   /* [BNMF_COA_NSTAT][BNMF_COA_NPROW][NP]; may be NULL */,
                    double* series /* [BNMF_COA_NSTAT][S][NP]; may be NULL */, bnmf_coactivity_info* info);
int bnmf_coactivity_at(bnmf_handle*, int end_iter, int n_samples, const int32_t* used, const int32_t* include, double min_load,
                       double credible_interval, double* pair, double* series, bnmf_coactivity_info* info);

/* Silhouette stability of the recorded signatures, on the device: are the N signatures well-separated, reproducible objects,
 * or do two factors keep sharing one signature, or does a signature dissolve between samples?  The points are the columns of P of every
 * recorded sample flagged in used[] (oldest first; NULL = all), s = 0 .. S-1: ring point (s, n) has index s N + n and the label
 * labels[row of s][n] (labels NULL: n), and extra column x (other chains, a catalogue) has index S N + x and the label extra_label[x].
 * labels has one row per sample of the whole range, so with gaps in used[] it is not bnmf_relabel's perm (one row per used sample): a
 * caller scatters those rows.  A ring point is a member when its label is not -1, A_s[n] != 0 and nn = sum_k P_s[k,n]^2 (k ascending from
 * +0.0) is finite and > 0; any other ring position is left out (n_left_out).  An extra column is always a member.  The member list of
 * cluster j: its ring members by ascending index, then its extras by ascending x; m_j its length.
 *   dot(i, i') = sum_k p_i[k] p_i'[k], k ascending from +0.0, multiply and add rounded separately;
 *   d(i, i') = 1 - dot / sqrt(nn_i nn_i')  (bitwise symmetric);
 *   D[i][j] = canonB over the member list of j of d(i, i'), the self term entered as +0.0  (canonB: bnmf_regress's blocked canonical sum).
 * Per member i of cluster c:  a = m_c >= 2 ? D[i][c] / (m_c - 1) : +0.0;  b = the smallest D[i][j] / m_j over j != c with m_j >= 1 (j
 * ascending, the first wins a tie), nearest = that j;  the silhouette is +0.0 when m_c < 2, NaN when no other cluster has a member (b NaN,
 * nearest -1), else with mx = max(a, b): mx > 0 ? (b - a) / mx : +0.0.
 * point [BNMF_STAB_NPOINT][S N + X]: silhouette, a, b, nearest; a left-out position has NaN, NaN, NaN, -1.
 * factor [BNMF_STAB_NFROW][N]: m_j; the canonical W = 64 sum of the members' silhouettes in list order / m_j (the stability; NaN if any is
 *   NaN or m_j = 0); the smallest silhouette (NaN likewise); the same mean of a and of b; #(silhouette < 0) / m_j.
 * between [N][N]: the canonical W = 64 sum over the members i of cluster a (list order) of D[i][b] / m_b, divided by m_a; on the diagonal
 *   the mean of a_i (factor row 3); NaN where a or b is empty.
 * medoid [K*N], medoid_at [N]: per cluster the member with the smallest D[i][j] (list order, the first wins a tie), its column divided by
 *   its sum over k ascending: the consensus signature; NaN and -1 for an empty cluster.
 * info: n_points = the members, n_clusters = #(m_j >= 1), n_negative = #(silhouette < 0), mean_silhouette = the canonical W = 64 sum of all
 *   members' silhouettes in index order / n_points, min_stability and min_stability_at = the smallest non-NaN factor row 1 and its label
 *   (the first wins a tie; NaN and -1 without one).
 * Only + - * /, sqrt, comparisons and whole numbers in a fixed order: the bits depend on the recorded samples, used, labels and the extras
 * alone; renumbering the labels permutes the outputs.  Works for every likelihood and prior (only P and A are read); read-only for the
 * chain; no random number is drawn.  bnmf_stability_at: the n_samples iterations that end at end_iter; the range rule and BNMF_ESIZE as
 * for bnmf_waic_at; bnmf_stability(h, n, ...) is bnmf_stability_at(h, iter, n, ...).  Refused before any device work: null info, a used[]
 * value other than 0 / 1 (the index named), a label outside -1 .. N-1 (sample and factor named), X < 0, X > 0 with a null extra_P or
 * extra_label, an extra label outside 0 .. N-1, an extra cell that is not finite (named) or an extra column that is all zero (named) with
 * BNMF_EINVAL; N < 2 or fewer than 2 used samples with BNMF_ESIZE; window = 0, a poisoned handle or nothing recorded with BNMF_ESTATE.
 * Refused after the pass that takes the norms of the ring points, which decides the members: fewer than 2 members in all or more than
 * BNMF_STAB_MAX_POINTS with BNMF_ESIZE. */
#define BNMF_STAB_NPOINT 4       /* point rows: silhouette, a (own cluster), b (nearest other), nearest (label as a double, -1: none) */
#define BNMF_STAB_NFROW  6       /* factor rows: members, mean silhouette (the stability), min silhouette, mean a, mean b, share with silhouette < 0 */
#define BNMF_STAB_MAX_POINTS 65536
typedef struct { int32_t n_used, n_points, n_extra, n_left_out, n_clusters, min_stability_at /* label; -1 if none */;
                 int64_t n_negative; double mean_silhouette, min_stability; } bnmf_stability_info;
int bnmf_stability(bnmf_handle*, int last_n, const int32_t* used,
                   const int32_t* labels   /* [n_samples][N] row-major over the whole range, rows of unused samples not read: the cluster of factor n of that sample, -1 = left out; NULL: n */,
                   const double* extra_P   /* K x X column-major: further columns (other chains, a catalogue); may be NULL with X = 0 */,
                   const int32_t* extra_label /* [X], 0 .. N-1 */, int X,
                   double* point   /* [BNMF_STAB_NPOINT][S*N + X]; may be NULL */,
                   double* factor  /* [BNMF_STAB_NFROW][N]; may be NULL */,
                   double* between /* [N][N] row-major; may be NULL */,
                   double* medoid  /* [K*N] column-major; may be NULL */,
                   int64_t* medoid_at /* [N] point index, -1: empty cluster; may be NULL */,
                   bnmf_stability_info* info);
int bnmf_stability_at(bnmf_handle*, int end_iter, int n_samples, const int32_t* used, const int32_t* labels, const double* extra_P,
                      const int32_t* extra_label, int X, double* point, double* factor, double* between, double* medoid, int64_t* medoid_at,
                      bnmf_stability_info* info);

/* Reconstruction quality per tumour over recorded samples, on the device: how well is each tumour of the cohort the chain
 * was run on reconstructed, and which signatures does it need?  Over the recorded samples flagged in used[] (oldest first; NULL = all),
 * s = 1 .. S, per tumour g and mutation type k, with m the data cell as a double (for a Normal handle the fp64 data of bnmf_create_f64,
 * negative cells included):
 *   f_n       = (P_s[k,n] * A_s[n]) * E_s[n,g]                    bnmf_attribution's expression, the same bits
 *   pre_0     = +0.0;  pre_{n+1} = pre_n + f_n                    n ascending
 *   suf_{N-1} = +0.0;  suf_{n-1} = suf_n + f_n                    n descending
 *   c    = pre_N                                                  the fit of the cell: bnmf_waic's c_s, the same bits
 *   c_-n = pre_n + suf_n                                          the fit without factor n: no subtraction, never negative
 *   d    = m - c
 * Per (s, g), each sum over k ascending from +0.0 (bnmf_project's order for its fit rows):
 *   dot = sum m c   cc = sum c c   l1 = sum |d|   sse = sum d d   dot_-n = sum m c_-n   cc_-n = sum c_-n c_-n
 * Per g, once, in the same order:   mm = sum m m   t = sum |m|
 *   cosv(dot, cc) = mm > 0 ? (cc > 0 ? dot / sqrt(mm * cc) : +0.0) : NaN     an empty fit explains nothing; an all-zero tumour is undefined
 *   cos    = cosv(dot, cc);   rel_l1 = t > 0 ? l1 / t : 0.0;   rmse = sqrt(sse / (double)K)
 *   cos_-n = A_s[n] != 0 ? cosv(dot_-n, cc_-n) : cos              an excluded factor is selected, not recomputed:
 *   drop_n = A_s[n] != 0 ? cos - cos_-n        : +0.0             its drop is exactly +0.0
 * The remaining exposures are NOT refitted after the removal.  The cosine does not depend on the scale of the fit, so no rescaling is
 * needed, but a refit could recover part of the loss: drop_n is an upper bound of what removing signature n costs the tumour.
 * (bnmf_prune below removes with a refit after every removal.)
 * Over s ascending every running mean and variance is bnmf_attribution's Welford (d = a - mu; mu = mu + d * (1 / s); M2 = M2 + d * (a - mu)),
 * the rest are plain counts:
 * tumour [BNMF_REC_NTUM][G]: 0 the mean of cos, 1 its variance M2 / (S - 1), 2 the smallest cos over the samples (from +inf, v < d ? v : d),
 *   3 the mean rel_l1, 4 the mean rmse, 5 #(cos >= min_cosine) / S; a tumour with mm == 0 has NaN in rows 0, 1, 2 and 5.
 * drop [BNMF_REC_NDROP][N*G], each row laid out n + N g: 0 the mean of drop_n, 1 its variance, 2 the mean of cos_-n, 3 #(drop_n >=
 *   min_drop) / S, the probability that the tumour needs the signature; all rows NaN where mm == 0.
 * series [S]: per used sample the mean cos over the defined tumours (mm > 0): the sum over g in the canonical W = 1024 order of
 *   bnmf_attribution's series, an undefined tumour entered as +0.0, divided by the number of defined tumours; NaN if there is none.
 * signature [BNMF_REC_NSIG][N]: 0 the number of tumours with drop row 3 >= 0.5, 1 the mean of drop row 0 (the canonical W = 64 sum over
 *   the defined tumours ascending, divided by their number; NaN without one), 2 the largest drop row 0 over the defined tumours (NaN
 *   without one).
 * info: n_used = S; n_undefined = the all-zero tumours; n_poor = the defined tumours whose mean cosine is < min_cosine; n_needed = the
 *   (n, g) with drop row 3 >= 0.5; min_cosine and min_drop as given; worst_cosine and worst_at = the smallest tumour row 0 and its g
 *   (the first wins a tie; NaN and -1 if no tumour is defined).
 * Only + - * /, sqrt, |.|, comparisons and whole numbers, no contraction, every sum in the order above: the bits depend on the samples,
 * used[], the data and the two thresholds only, not on the batch size, the tiling or the form of the kernel.  Reads only the P, E and A
 * rings and the data; works for every likelihood and prior; draws no random number, consumes none of the chain's streams and is
 * read-only for the chain.  bnmf_reconstruction_at: the n_samples iterations that end at end_iter; the range rule, used[] and BNMF_ESIZE
 * as for bnmf_attribution_at; bnmf_reconstruction(h, n, ...) is bnmf_reconstruction_at(h, iter, n, ...).  Refused before any device work:
 * a null info, a used[] value other than 0 / 1 (the index named), a min_cosine or min_drop that is NaN or infinite with BNMF_EINVAL; fewer
 * than 2 used samples with BNMF_ESIZE; window = 0, a poisoned handle or nothing recorded with BNMF_ESTATE. */
#define BNMF_REC_NTUM  6         /* tumour rows: mean cos, its variance, smallest cos, mean rel_l1, mean rmse, share of samples with cos >= min_cosine */
#define BNMF_REC_NDROP 4         /* drop rows: mean drop, its variance, mean leave-one-out cosine, share of samples with drop >= min_drop */
#define BNMF_REC_NSIG  3         /* signature rows: tumours that need it, mean of the mean drop, largest mean drop */
typedef struct { int32_t n_used, n_undefined; int64_t n_poor, n_needed, worst_at /* g; -1 if none */; double min_cosine, min_drop, worst_cosine; }
    bnmf_reconstruction_info;
int bnmf_reconstruction(bnmf_handle*, int last_n, const int32_t* used, double min_cosine, double min_drop,
                        double* tumour    /* [BNMF_REC_NTUM][G]; may be NULL */,
                        double* drop      /* [BNMF_REC_NDROP][N*G], each row laid out as E; may be NULL */,
                        double* series    /* [S]; may be NULL */,
                        double* signature /* [BNMF_REC_NSIG][N]; may be NULL */,
                        bnmf_reconstruction_info* info);
int bnmf_reconstruction_at(bnmf_handle*, int end_iter, int n_samples, const int32_t* used, double min_cosine, double min_drop, double* tumour,
                           double* drop, double* series, double* signature, bnmf_reconstruction_info* info);

/* Similarity of tumours over recorded samples, on the device: which tumours have the exposure profile of this one, does the
 * cohort fall into subtypes, which tumours resemble nobody?  The cosine of two tumours' exposure vectors is a sum over the factors, so it
 * is immune to label switching: no bnmf_relabel is needed first.  The members are the m included tumours g_0 < g_1 < ... (include[g] != 0;
 * NULL = all: bnmf_regress's member list); the samples are the recorded samples flagged in used[] (oldest first; NULL = all), s = 1 .. S.
 * Per sample, with cs_s[n] bnmf_map's column sum of P_s:
 *   x_s[n,g]   = A_s[n] != 0 ? E_s[n,g] * cs_s[n] : +0.0           bnmf_contrast's renormalised exposure, the same bits
 *   nn_s[g]    = sum_n x_s[n,g] * x_s[n,g]                          n ascending from +0.0; multiply and add rounded separately
 *   dot_s(g,h) = sum_n x_s[n,g] * x_s[n,h]                          the same order
 *   c_s(g,h)   = nn_s[g] * nn_s[h] == 0 ? +0.0 : dot_s(g,h) / sqrt(nn_s[g] * nn_s[h])
 * A tumour without any exposure in a sample resembles nothing (+0.0, which is also what a product that underflows to 0 gives); nn is a
 * sum of squares, so the product is > 0, 0 or NaN, and a NaN or an infinity takes the division and propagates by IEEE.  c_s is bitwise
 * symmetric in (g, h).  Per pair g != h of members, over s ascending, bnmf_attribution's Welford (d = c - mu; mu = mu + d * (1 / s);
 * M2 = M2 + d * (c - mu)) and a count:   mean = mu,   variance = M2 / (S - 1),   p_similar = #(c_s >= min_cosine) / S.
 * neighbour_at [G][top_k] (row-major) and neighbour [BNMF_SIM_NNROW][G][top_k]: for member g the top_k other members with the largest
 *   mean, the mean descending and the lower tumour first among equal means; a NaN mean is never listed.  Rows: 0 mean, 1 variance,
 *   2 p_similar.  Unfilled places (fewer than top_k candidates) and every place of a left-out tumour hold -1 / NaN.
 * dense [BNMF_SIM_NDROW][Q][G]: rows 0 mean, 1 variance, 2 p_similar of query[q] against every tumour g; NaN where g is left out or
 *   g == query[q].  query = all tumours of a small cohort gives the whole matrix.  A tumour may be named more than once.
 * tumour [BNMF_SIM_NTUM][G]: 0 the typicality: the mean over the other members of the mean cosine, the sum taken as bnmf_regress's
 *   blocked canonical sum (blocks of BNMF_REG_BLOCK members in member order, each the canonical W = 64 sum, the blocks added ascending
 *   from +0.0) with the self term entered as +0.0, divided by m - 1; 1 the mean cosine of the first neighbour (the largest mean to
 *   another member under the order above; NaN if every mean is NaN); 2 the degree: the other members with p_similar >= 0.5.  NaN for
 *   a left-out tumour.
 * info: n_used = S, n_included = m, n_left_out = G - m, top_k, n_query = Q, n_pairs = m (m - 1) / 2, min_cosine as given; and from the
 *   pass over all pairs: n_similar_pairs = the unordered pairs with p_similar >= 0.5, n_isolated = the members of degree 0,
 *   mean_similarity = the canonical W = 64 sum of tumour row 0 over the members ascending, divided by m; least_typical and
 *   least_typical_at = the smallest non-NaN tumour row 0 and its g (the first wins; NaN and -1 without one).
 * With top_k == 0, tumour == NULL and Q > 0 only the Q rows of dense are computed and the pass over all pairs does not run: then
 * n_similar_pairs = n_isolated = -1, mean_similarity = least_typical = NaN and least_typical_at = -1.  In every other case the pass
 * runs, whichever outputs are NULL.  Each of the four arrays may be NULL.
 * Only + - * /, sqrt, comparisons and whole numbers, no contraction, every sum in the order above: the bits depend on the samples,
 * used[], include[], query[], top_k and min_cosine only, not on the tiling, the band of rows that passes through the scratch or the form
 * of the kernel.  A pair's values involve its two tumours only and every sum over tumours runs over the member list, so leaving tumours
 * out through include[] gives the bits of a cohort without them.  Reads only the P, E and A rings; works for every likelihood and
 * prior; draws no random number, consumes none of the chain's streams and is read-only for the chain.  bnmf_similarity_at: the
 * n_samples iterations that end at end_iter; the range rule, used[] and BNMF_ESIZE as for bnmf_attribution_at; bnmf_similarity(h, n, ...)
 * is bnmf_similarity_at(h, iter, n, ...).  Refused before any device work: a null info, a used[] or include[] value other than 0 / 1
 * (the index named), Q < 0, Q > 0 with a null query, a query[q] outside 0 .. G-1 or left out (q named), top_k outside
 * 0 .. BNMF_SIM_MAX_K, a min_cosine that is NaN or infinite with BNMF_EINVAL; fewer than 2 used samples or m < 2 with BNMF_ESIZE;
 * window = 0, a poisoned handle or nothing recorded with BNMF_ESTATE. */
#define BNMF_SIM_NNROW 3         /* neighbour rows: mean, variance, p_similar */
#define BNMF_SIM_NDROW 3         /* dense rows: mean, variance, p_similar */
#define BNMF_SIM_NTUM  3         /* tumour rows: typicality, mean cosine of the first neighbour, degree */
#define BNMF_SIM_MAX_K 32        /* the largest top_k */
typedef struct { int32_t n_used, n_included, n_left_out, top_k, n_query, _pad; int64_t n_pairs, n_similar_pairs, n_isolated,
                 least_typical_at /* g; -1 if none */; double mean_similarity, least_typical, min_cosine; } bnmf_similarity_info;
int bnmf_similarity(bnmf_handle*, int last_n, const int32_t* used,
                    const int32_t* include /* [G] 0 / 1, NULL = all */,
                    const int32_t* query /* [Q] tumours, may be NULL with Q = 0 */, int Q,
                    int top_k, double min_cosine,
                    int32_t* neighbour_at /* [G][top_k] row-major; may be NULL */,
                    double*  neighbour    /* [BNMF_SIM_NNROW][G][top_k]; may be NULL */,
                    double*  dense        /* [BNMF_SIM_NDROW][Q][G]; may be NULL */,
                    double*  tumour       /* [BNMF_SIM_NTUM][G]; may be NULL */,
                    bnmf_similarity_info* info);
int bnmf_similarity_at(bnmf_handle*, int end_iter, int n_samples, const int32_t* used, const int32_t* include, const int32_t* query, int Q,
                       int top_k, double min_cosine, int32_t* neighbour_at, double* neighbour, double* dense, double* tumour,
                       bnmf_similarity_info* info);

/* Subtypes of tumours over recorded samples, on the device: does the cohort fall into subtypes, and how certain is the
 * grouping?  Every recorded sample flagged in used[] (oldest first; NULL = all) is clustered by the same Lloyd iteration (k-means) from
 * the same start centres0, so subtype c means the same thing in every sample; the statistics over the samples say how often a tumour
 * carries which label.  The members are the m included tumours g_0 < g_1 < ... (include[g] != 0; NULL = all), position i = 0 .. m-1.
 * Per used sample s, with cs_s[n] bnmf_map's column sum of P_s:
 *   x[n,g] = A_s[n] != 0 ? E_s[n,g] * cs_s[n] : +0.0              bnmf_contrast's renormalised exposure, the same bits
 *   t      = sum_n x[n,g]                                           n ascending from +0.0
 *   g is unassigned in s unless t > 0 && t < inf: its label is -1, it enters every sum below as +0.0 and enters no count
 *   u = 1 / t;  r[n] = x[n,g] * u                                   the share profile
 *   q[perm[s][n]] = r[n]                                            the aligned profile; perm NULL: q = r
 * perm [last_n][N] (row-major, a row per sample of the whole range, read for the used ones) is bnmf_relabel's: a row of -1 throughout
 * leaves the sample out whole (unmatched, as bnmf_stability leaves it out); every other row must be a permutation of 0 .. N-1.  The
 * matched samples are S' of the S used ones.
 * Lloyd steps from mu = centres0 (N x C column-major, mu[j,c] at j + N c):
 *   assign  d(g,c) = sum_j (q[j] - mu[j,c]) * (q[j] - mu[j,c])    j ascending from +0.0; subtract, multiply, add rounded separately
 *           label = 0, dmin = d(g,0); for c = 1 .. C-1 in order: d(g,c) replaces them only if d(g,c) < dmin.  The lowest c wins a tie,
 *           a NaN never replaces anything (a NaN d(g,0) stays: label 0, dmin NaN)
 *   update  n_c = #(label == c);  where n_c > 0:  mu[j,c] = canonB_i(label_i == c ? q_i[j] : +0.0) / n_c;  n_c == 0 keeps the centre.
 *           canonB is bnmf_regress's blocked canonical sum over the positions i of the member list: blocks of BNMF_REG_BLOCK positions,
 *           each the canonical W = 64 sum (accumulator l adds positions l, l + 64, ... of the block ascending from +0.0, then the
 *           halving tree), the block sums added ascending from +0.0
 *   stop    after the first step that changes no label (step 1 is compared with all -1), or after n_steps.  steps_s = the steps run.
 * The sample's labels are the last assignment's, its centres and n_c the update after it, inertia_s = canonB_i(dmin_i) of that assignment
 * (an unassigned tumour +0.0).
 * Over the matched samples, with count_c[g] = #(label_s[g] == c) and a_g = the samples in which g is assigned:
 * membership [C][G]: count_c[g] / a_g; NaN where a_g == 0 or g is left out.
 * label [G]: the c of the largest count, the lowest c among equals; -1 where a_g == 0 or g is left out.
 * tumour [BNMF_SUB_NTUM][G]: 0 certainty = membership[label[g]][g]; 1 a_g / S'; 2 the runner-up: the largest membership of a c other
 *   than label[g].  Rows 0 and 2 are NaN where a_g == 0; all rows NaN for a left-out tumour.
 * centre [BNMF_SUB_NCROW][N*C] and size [BNMF_SUB_NCROW][C]: over the S' samples of every centre coordinate (j + N c) and of every n_c the
 *   rows 0 mean (the canonical W = 64 sum / S'), 1 variance (the canonical sum of (v - mean)^2 / (S' - 1)), 2 and 3 the type-7 quantiles
 *   at (1 - 0.95) / 2 and (1 + 0.95) / 2, as bnmf_contrast forms them.  The credible interval is fixed at 0.95.
 * together [Q][G]: the consensus row of query[q]: #(label_s[query[q]] == label_s[g] >= 0) / #(both assigned in s); NaN where that is 0,
 *   where g is left out or g == query[q].  All tumours of a small cohort as queries give the consensus matrix.
 * labels [S][G] (a row per USED sample): the sample's labels; -2 for a left-out tumour, -1 for an unassigned one, -2 throughout for an
 *   unmatched sample.
 * series [BNMF_SUB_NSER][S]: 0 inertia_s, 1 steps_s, 2 the assigned tumours of s; NaN for an unmatched sample.
 * info: n_used = S, n_matched = S', n_unmatched, n_included = m, n_left_out = G - m, C, n_steps, n_query = Q, min_certainty as given;
 *   n_not_converged = the samples that ran n_steps steps and changed a label in the last; n_certain = the members with certainty >=
 *   min_certainty; n_never_assigned = the members with a_g == 0; mean_certainty = the canonical W = 64 sum of the certainties of the
 *   members that have one, in member order, divided by their number (NaN without one); least_certain and least_certain_at = the smallest
 *   certainty and its g (the first wins; NaN and -1 without one); smallest_subtype and smallest_subtype_at = the smallest size row 0 and
 *   its c (the first wins).
 * Only + - * /, comparisons and whole numbers, no contraction, no square root, every sum in the order above: the bits depend on the
 * samples, used[], include[], perm, centres0, n_steps and query[] only, not on the form of the kernel, its tiles or the batch of samples
 * that passes through the scratch.  Every sum over tumours runs over the member list and a tumour's own values involve no other tumour,
 * so include[] gives the bits of a cohort without the tumours left out.  Reads only the P, E and A rings; works for every likelihood
 * and prior; draws no random number, consumes none of the chain's streams and is read-only for the chain.  bnmf_subtypes_at: the
 * n_samples iterations that end at end_iter; the range rule, used[], BNMF_ESIZE and BNMF_ESTATE as for bnmf_similarity_at;
 * bnmf_subtypes(h, n, ...) is bnmf_subtypes_at(h, iter, n, ...).  Every output array may be NULL.  Refused before any device work, with
 * BNMF_EINVAL: a null info or centres0; a used[] or include[] value other than 0 / 1 (the index named); C outside 2 .. BNMF_SUB_MAX_C;
 * n_steps outside 1 .. BNMF_SUB_MAX_STEPS; Q < 0 or Q > 0 with a null query; a query[q] outside 0 .. G-1 or left out (q named); a cell
 * of centres0 that is NaN, infinite or negative (the first one named); a min_certainty that is NaN or outside [0, 1]; a perm row of a
 * used sample that is neither a permutation nor -1 throughout (the sample named).  With BNMF_ESIZE: fewer than 2 used samples, fewer
 * than 2 matched samples, m < C, N > BNMF_SUB_MAX_N.  With BNMF_ESTATE: window = 0, a poisoned handle or nothing recorded. */
#define BNMF_SUB_NTUM  3         /* tumour rows: certainty, share of samples assigned, runner-up membership */
#define BNMF_SUB_NCROW 4         /* centre and size rows: mean, variance, lower, upper (0.95) */
#define BNMF_SUB_NSER  3         /* series rows: inertia, steps, assigned tumours */
#define BNMF_SUB_MAX_C 32        /* the most subtypes */
#define BNMF_SUB_MAX_N 128       /* the most factors */
#define BNMF_SUB_MAX_STEPS 1000  /* the most Lloyd steps */
typedef struct { int32_t n_used, n_matched, n_unmatched, n_included, n_left_out, C, n_steps, n_query, n_not_converged, n_certain,
                 n_never_assigned, smallest_subtype_at /* c */; int64_t least_certain_at /* g; -1 if none */;
                 double mean_certainty, least_certain, smallest_subtype, min_certainty; } bnmf_subtypes_info;
int bnmf_subtypes(bnmf_handle*, int last_n, const int32_t* used,
                  const int32_t* include  /* [G] 0 / 1, NULL = all */,
                  const int32_t* perm     /* [last_n][N] row-major: bnmf_relabel's perm over the whole range; NULL = identity */,
                  const double*  centres0 /* N x C column-major */, int C, int n_steps,
                  const int32_t* query    /* [Q] tumours, may be NULL with Q = 0 */, int Q, double min_certainty,
                  double*  membership /* [C][G]; may be NULL */,
                  int32_t* label      /* [G]; may be NULL */,
                  double*  tumour     /* [BNMF_SUB_NTUM][G]; may be NULL */,
                  double*  centre     /* [BNMF_SUB_NCROW][N*C]; may be NULL */,
                  double*  size       /* [BNMF_SUB_NCROW][C]; may be NULL */,
                  double*  together   /* [Q][G]; may be NULL */,
                  int32_t* labels     /* [S][G]; may be NULL */,
                  double*  series     /* [BNMF_SUB_NSER][S]; may be NULL */,
                  bnmf_subtypes_info* info);
int bnmf_subtypes_at(bnmf_handle*, int end_iter, int n_samples, const int32_t* used, const int32_t* include, const int32_t* perm,
                     const double* centres0, int C, int n_steps, const int32_t* query, int Q, double min_certainty, double* membership,
                     int32_t* label, double* tumour, double* centre, double* size, double* together, int32_t* labels, double* series,
                     bnmf_subtypes_info* info);

/* Residual structure of recorded samples, on the device: what does the model leave unexplained, and do the misfits of
 * different tumours point in the same direction?  A shared direction is what a missing signature looks like: a rank that is too LOW.
 * The members are the m included tumours g_0 < g_1 < ... (include[g] != 0; NULL = all), position i = 0 .. m-1.  Per recorded sample s
 * flagged in used[] (oldest first; NULL = all), member i (tumour g) and mutation type k, M the data cell as a double:
 *   c = bnmf_reconstruction's pre_N (bnmf_waic's c_s), the same bits: from +0.0, n ascending, + (P_s[k,n] * A_s[n]) * E_s[n,g]
 *   Poisson: lam = c < 1e-6 ? 1e-6 : c;  z = (M - lam) / sqrt(lam).     Normal: z = (M - c) / sqrt(sigmasq_s[g]), real-valued data included
 *   C_s[k,k'] = canonB_i(z[k,i] * z[k',i]) / m  for k' <= k, mirrored: bitwise symmetric.  The product is rounded before it is added; canonB is
 *     bnmf_regress's blocked canonical sum over the positions i of the member list (blocks of BNMF_REG_BLOCK, each the canonical W = 64 sum,
 *     the block sums added ascending from +0.0)
 *   b_s[k] = canonB_i(z[k,i]) / m;   q_s[k] = C_s[k,k];   tr_s = sum_k C_s[k,k], k ascending from +0.0;   chi_s[i] = (sum_k z z) / K, k ascending
 * The leading component of a symmetric K x K matrix C, one routine for every C_s (device) and for the mean matrix (host):
 *   1 k* = the largest diagonal element, the first wins;  y = C[:,k*]
 *   2 nn = sum_k y[k] y[k], k ascending from +0.0;  v = y / sqrt(nn)
 *   3 n_steps times: y[k] = sum_k' C[k,k'] v[k'], k' ascending from +0.0, multiply and add rounded separately; then 2
 *   4 one further product y = C v:  lambda = sum_k v[k] y[k];  nn = sum_k y[k] y[k];  move = max_k |y[k] / sqrt(nn) - v[k]| (how far one
 *     more step would go; the maximum from +0.0, k ascending)
 *   5 v is flipped so that its element of largest magnitude (the first wins) is positive;  share = lambda / trace
 *   The matrix is flat if its trace is not > 0 and finite or if any nn (that of 4 included) is not > 0 and finite.  A flat sample is left
 *   out of everything below, as an unmatched sample is in bnmf_subtypes; S' of the S used samples are not flat.
 *   t_s[i] = sum_k v_s[k] z[k,i], k ascending from +0.0: the tumour's score on the sample's component.
 * Over the S' samples, means and variances in bnmf_contrast's canonical W = 64 forms over s (mean = canon(x) / S', variance =
 * canon((x - mean)^2) / (S' - 1)):  gram [K*K] = the mean of C_s (row-major; symmetric), vbar, lambda, share, move its leading component;
 * a_s = sum_k v_s[k] vbar[k], k ascending;  sgn_s = a_s < 0 ? -1 : 1.
 * type [BNMF_RES_NTYPE][K]: 0 mean of b, 1 variance of b, 2 #(b > 0) / S', 3 mean of q (the Pearson dispersion of the type: 1 is what a
 *   correct Poisson model gives), 4 variance of q.
 * component [BNMF_RES_NCOMP][K]: 0 vbar, 1 mean of sgn_s v_s[k], 2 its variance, 3 #(sgn_s v_s[k] > 0) / S'.
 * tumour [BNMF_RES_NTUM][G]: 0 mean of sgn_s t_s[g], 1 its variance, 2 mean of chi; all rows NaN for a left-out tumour.
 * series [BNMF_RES_NSER][S]: tr_s, lambda_s, share_s, move_s, a_s; NaN in a flat sample's column.
 * info: n_used = S, n_flat = S - S', n_included = m, n_left_out = G - m, n_steps, max_dispersion as given; lambda, share, move of the mean
 *   matrix; mean_share = canon(share_s) / S'; min_agreement and min_agreement_at = the smallest |a_s| and its s among the used samples
 *   (the first wins); n_biased = the types whose type row 2 is <= 0.025 or >= 0.975; n_overdispersed = the types whose row 3 is >
 *   max_dispersion (a reporting convention like min_cosine = 0.9, not a test); worst_type and worst_type_at = the largest row 3 and its k
 *   (the first wins).
 * Only + - * /, sqrt, |.|, comparisons and whole numbers, no contraction, every sum in the order above: the bits depend on the samples,
 * used[], include[], the data and n_steps only, not on the form of the kernel, its tiles or the batch of samples that passes through the
 * scratch.  Every sum over tumours runs over the member list and a tumour's own values involve no other tumour, so include[] gives the bits
 * of a cohort without the tumours left out.  Reads the P, E, A (Normal: and sigmasq) rings and the data; draws no random number, consumes
 * none of the chain's streams and is read-only for the chain.  bnmf_residuals_at: the n_samples iterations that end at end_iter; the range
 * rule, used[], BNMF_ESIZE and BNMF_ESTATE as for bnmf_similarity_at; bnmf_residuals(h, n, ...) is bnmf_residuals_at(h, iter, n, ...).
 * Every output array may be NULL.  Refused before any device work, with BNMF_EINVAL: a null info; a used[] or include[] value other than
 * 0 / 1 (the index named); n_steps outside 1 .. BNMF_RES_MAX_STEPS; a max_dispersion that is NaN or negative.  With BNMF_ESIZE: fewer than 2
 * used samples, m < 2, K > BNMF_RES_MAX_K; and, known only after the device pass, S' < 2.  With BNMF_ESTATE: window = 0, a poisoned handle
 * or nothing recorded. */
#define BNMF_RES_NTYPE 5         /* type rows: mean b, variance of b, share of b > 0, mean q (dispersion), variance of q */
#define BNMF_RES_NCOMP 4         /* component rows: vbar, mean, variance and share > 0 of the aligned v_s */
#define BNMF_RES_NTUM  3         /* tumour rows: mean and variance of the aligned score, mean chi */
#define BNMF_RES_NSER  5         /* series rows: trace, lambda, share, move, agreement */
#define BNMF_RES_MAX_K 2048      /* the most mutation types */
#define BNMF_RES_MAX_STEPS 10000 /* the most power steps */
typedef struct { int32_t n_used, n_flat, n_included, n_left_out, n_steps, n_biased, n_overdispersed, worst_type_at /* k */,
                 min_agreement_at /* s; -1 if none */, _pad;
                 double lambda, share, move, mean_share, min_agreement, worst_type, max_dispersion; } bnmf_residuals_info;
int bnmf_residuals(bnmf_handle*, int last_n, const int32_t* used,
                   const int32_t* include   /* [G] 0 / 1, NULL = all */, int n_steps, double max_dispersion,
                   double* gram      /* [K*K]; may be NULL */,
                   double* type      /* [BNMF_RES_NTYPE][K]; may be NULL */,
                   double* component /* [BNMF_RES_NCOMP][K]; may be NULL */,
                   double* tumour    /* [BNMF_RES_NTUM][G]; may be NULL */,
                   double* series    /* [BNMF_RES_NSER][S]; may be NULL */,
                   bnmf_residuals_info* info);
int bnmf_residuals_at(bnmf_handle*, int end_iter, int n_samples, const int32_t* used, const int32_t* include, int n_steps, double max_dispersion,
                      double* gram, double* type, double* component, double* tumour, double* series, bnmf_residuals_info* info);

/* Trade-offs between signatures within a tumour over recorded samples, on the device: which signatures exchange mutations
 * from sample to sample in one tumour, and how uncertain is a SUM of exposures?  Flat or similar signatures trade mutations: each marginal
 * interval is wide while their sum is sharply determined, which no per-signature output shows.  The members are the m included tumours
 * g_0 < g_1 < ... (include[g] != 0; NULL = all), position i = 0 .. m-1.  The samples are the recorded ones flagged in used[] (oldest
 * first; NULL = all).  perm [last_n][N] (row-major, a row per sample of the whole range, read for the used ones) is bnmf_relabel's, as
 * bnmf_subtypes takes it: NULL = identity; a row of -1 throughout leaves the sample out (unmatched); every other row of a used sample
 * must be a permutation of 0 .. N-1.  The S' matched samples of the S used ones are numbered t = 1 .. S' in order.
 * Per matched sample and member g, with cs_s[n] bnmf_map's column sum of P_s:
 *   x[n]            = A_s[n] != 0 ? E_s[n,g] * cs_s[n] : +0.0        bnmf_contrast's renormalised exposure, the same bits
 *   q_t[perm[s][n]] = x[n]                                            the aligned exposure
 * Two passes over the samples, per member:
 *   mu[j]    = (sum_t q_t[j], t ascending from +0.0) / S'
 *   d_t[j]   = q_t[j] - mu[j]
 *   cov[j,l] = (sum_t d_t[j] * d_t[l], t ascending from +0.0; the product rounded before it is added) / (S' - 1)    for l <= j, mirrored
 *   r[j,l]   = cov[j,j] * cov[l,l] > 0 and finite ? cov[j,l] / sqrt(cov[j,j] * cov[l,l]) : NaN   (j != l; "undefined": a factor never
 *              active in this tumour, e.g. excluded by A in every sample, has variance 0);   r[j,j] = NaN
 * The matrix is bitwise symmetric.
 * tumour [BNMF_TRD_NTUM][G]: 0 the smallest defined r[j,l] over j > l (j ascending, then l ascending, the first wins; NaN without one);
 *   1 the number of defined pairs j > l; 2 vt / sv, the variance of the tumour's total over the sum of the marginal variances:
 *   vt = sum_j (sum_l cov[j,l]), l ascending inside and j ascending outside, both from +0.0; sv = sum_j cov[j,j]; NaN unless sv > 0 and
 *   finite.  Below 1 the signatures trade mutations, 1 means they vary independently.  All rows NaN for a left-out tumour.
 * pair_at [G]: j * N + l of row 0's pair; -1 without one or for a left-out tumour.
 * pair [BNMF_TRD_NPAIR][N*N] (row-major j * N + l, symmetric, the diagonal NaN), over the members with a defined r[j,l], n_def of them:
 *   0 the mean r: canonB over the member positions of (defined ? r : +0.0), divided by n_def (NaN if n_def = 0); canonB is bnmf_regress's
 *   blocked canonical sum (blocks of BNMF_REG_BLOCK positions, each the canonical W = 64 sum, the block sums added ascending from +0.0);
 *   1 n_def; 2 #(r <= -min_corr) / n_def; 3 #(r >= min_corr) / n_def (both NaN if n_def = 0); 4 the mean covariance canonB(cov[j,l]) / m
 *   over all members.
 * dense [Q][2][N*N]: for query[q] the covariance matrix, then the correlation matrix (the diagonal NaN).  A tumour may be named more than
 *   once.
 * setstat [BNMF_TRD_NSET][C][G], with sets [N] (values 0 .. C-1, or -1 for a signature in no set; NULL with C = 0: no sets), per set c and
 *   member: 0 sum_{j in c} mu[j], j ascending from +0.0; 1 the variance of the set's summed exposure sum_{j in c} (sum_{l in c} cov[j,l]),
 *   nested and ordered as vt (the SD^2 to quote for "SBS2 + SBS13"; no marginal output gives it); 2 sum_{j in c} cov[j,j]; 3 row 1 / row 2,
 *   NaN unless row 2 > 0 and finite.  NaN for a left-out tumour.
 * info (sizeof = 64): n_used = S, n_matched = S', n_unmatched, n_included = m, n_left_out = G - m, n_sets = C, n_query = Q, min_corr as
 *   given; n_traded = the members whose tumour row 0 is <= -min_corr; strongest_pair and strongest_pair_at = the smallest pair row 0 over
 *   j > l and its j * N + l (the first wins; NaN and -1 without one); mean_ratio = the canonical W = 64 sum of tumour row 2 over the
 *   members that have one, in member order, divided by their number (NaN without one).  min_corr is a reporting convention like
 *   min_cosine = 0.9, not a test.
 * Only + - * /, sqrt, comparisons and whole numbers, no contraction, every sum in the order above: the bits depend on the samples, used[],
 * include[], perm, sets, query and min_corr only, not on the form of the kernel, its tiles or the band of members whose covariances pass
 * through the scratch.  A tumour's own values involve no other tumour and every sum over tumours runs over the member list, so include[]
 * gives the bits of a cohort without the tumours left out.  Reads only the P, E and A rings; works for every likelihood and prior; draws
 * no random number, consumes none of the chain's streams and is read-only for the chain.  bnmf_tradeoff_at: the n_samples iterations that
 * end at end_iter; the range rule, used[], BNMF_ESIZE and BNMF_ESTATE as for bnmf_subtypes_at; bnmf_tradeoff(h, n, ...) is
 * bnmf_tradeoff_at(h, iter, n, ...).  Every output array may be NULL.  Refused before any device work, with BNMF_EINVAL: a null info; a
 * used[] or include[] value other than 0 / 1 (the index named); a perm row of a used sample that is neither a permutation nor -1
 * throughout (the sample named); C outside 0 .. BNMF_TRD_MAX_C, C > 0 with a null sets, a sets value outside -1 .. C-1 (the factor
 * named), an empty set (named); Q < 0 or Q > 0 with a null query; a query[q] outside 0 .. G-1 or left out (q named); a min_corr that is
 * NaN or outside [0, 1].  With BNMF_ESIZE: fewer than 2 used samples, fewer than 2 matched samples, m < 1, N > BNMF_TRD_MAX_N.  With
 * BNMF_ESTATE: window = 0, a poisoned handle or nothing recorded. */
#define BNMF_TRD_NTUM  3         /* tumour rows: smallest correlation, defined pairs, variance of the total / sum of the variances */
#define BNMF_TRD_NPAIR 5         /* pair rows: mean r, n_def, share r <= -min_corr, share r >= min_corr, mean covariance */
#define BNMF_TRD_NSET  4         /* setstat rows: mean, variance of the sum, sum of the variances, their ratio */
#define BNMF_TRD_MAX_C 32        /* the most sets */
#define BNMF_TRD_MAX_N 128       /* the most factors */
typedef struct { int32_t n_used, n_matched, n_unmatched, n_included, n_left_out, n_sets, n_query, n_traded, strongest_pair_at /* j * N + l; -1 if none */,
                 _pad; double strongest_pair, mean_ratio, min_corr; } bnmf_tradeoff_info;
int bnmf_tradeoff(bnmf_handle*, int last_n, const int32_t* used,
                  const int32_t* include /* [G] 0 / 1, NULL = all */,
                  const int32_t* perm    /* [last_n][N] row-major: bnmf_relabel's perm over the whole range; NULL = identity */,
                  const int32_t* sets    /* [N] 0 .. C-1 or -1; NULL with C = 0 */, int C,
                  const int32_t* query   /* [Q] tumours, may be NULL with Q = 0 */, int Q, double min_corr,
                  double*  tumour  /* [BNMF_TRD_NTUM][G]; may be NULL */,
                  int32_t* pair_at /* [G]; may be NULL */,
                  double*  pair    /* [BNMF_TRD_NPAIR][N*N]; may be NULL */,
                  double*  dense   /* [Q][2][N*N]; may be NULL */,
                  double*  setstat /* [BNMF_TRD_NSET][C][G]; may be NULL */,
                  bnmf_tradeoff_info* info);
int bnmf_tradeoff_at(bnmf_handle*, int end_iter, int n_samples, const int32_t* used, const int32_t* include, const int32_t* perm, const int32_t* sets, int C,
                     const int32_t* query, int Q, double min_corr, double* tumour, int32_t* pair_at, double* pair, double* dense, double* setstat,
                     bnmf_tradeoff_info* info);

/* Sparse per-tumour assignment with refit over recorded samples, on the device: which signatures does a tumour keep, and how
 * large are they once the others are gone?  Backward elimination with a KL refit of the remaining exposures after every removal, until the
 * fit's cosine would fall by more than max_loss: the refit that bnmf_reconstruction's drop_n leaves out, and the table signature-assignment
 * tools report.  Done for every recorded sample it also gives the probability that a tumour keeps a signature.  The members are the m
 * included tumours g_0 < g_1 < ... (include[g] != 0; NULL = all).  The samples are the recorded ones flagged in used[] (oldest first;
 * NULL = all), numbered s = 1 .. S.
 * Only + - * /, sqrt, |.|, comparisons and whole numbers, no contraction, every sum in the order given here.  Per used sample s and member
 * g, with m_k the data cell as a double:
 *   set-up    cs[n] = bnmf_map's column sum of P_s[, n].  Factor n takes part iff A_s[n] != 0 and cs[n] > 0.  The places i = 0 .. N_in-1
 *             are the factors that take part, ascending (bnmf_project's idx), and x[k,i] = P_s[k,idx[i]] / cs[idx[i]].
 *             t = sum_k m_k, mm = sum_k m_k m_k, k ascending from +0.0.
 *             Warm start: e_i = E_s[idx[i], g] * cs[idx[i]], the sample's own renormalised exposure (bnmf_contrast's x, the same bits).
 *   step      with an active flag per place (a place that is not active holds e_i = +0.0):  every g_i = +0.0;  for k ascending:
 *             c = sum_i x[k,i] * e_i (i ascending over all places from +0.0; an inactive place adds +0.0), q = c > 0 ? m_k / c : 0.0,
 *             g_i = g_i + x[k,i] * q;  then e_i = active_i ? e_i * g_i : +0.0 and d = max_i |e_i(new) - e_i(old)| (from +0.0,
 *             v > d ? v : d).  This is bnmf_project's step with the flags.
 *   cosine    of a state: c_k as above, dot = sum_k m_k c_k, cc = sum_k c_k c_k (k ascending from +0.0);
 *             cos = mm > 0 ? (cc > 0 ? dot / sqrt(mm * cc) : +0.0) : NaN   (bnmf_reconstruction's cosv)
 *   round 0   every place active; n_steps steps from the warm start give the state and cos_0.
 *   rounds    while more than one place is active: order the active places by (e_i ascending, i ascending).  For each candidate i in that
 *             order: copy the state, set e_i = +0.0, clear its flag, run n_steps steps, cos_t = the cosine; every trial is counted.  The
 *             first candidate with cos_t >= cos_0 - max_loss (the difference formed once; a comparison with NaN is false) becomes the
 *             state and the next round starts.  If no candidate of a round passes, the elimination stops.
 *   A tumour with mm == 0 is undefined: no trials, NaN outputs, counted in info.
 *   Per (s, g): e_sparse[n] by factor number, exactly +0.0 for a removed or non-participating factor; cos_0; cos_f, the cosine of the last
 *   accepted state; n_kept, the places still active; trials; change = t > 0 ? d / t : 0.0 with d of the last step of the last accepted
 *   state (how a user judges n_steps).
 * Over s ascending, bnmf_attribution's Welford (d = a - mu; mu = mu + d * (1 / s); M2 = M2 + d * (a - mu)) and plain counts:
 * load [BNMF_PRN_NLOAD][N*G] (n + N g): 0 the mean of e_sparse; 1 its variance M2 / (S - 1) (NaN by IEEE for S = 1); 2 the mean share
 *   (sum_s e_n * u) / S with u = 1 / sum_n e_n (n ascending from +0.0; 0.0 where the sum is not positive), bnmf_attribution's share rule;
 *   3 p_kept = #(e_n > 0) / S.  NaN for an undefined or left-out tumour.
 * tumour [BNMF_PRN_NTUM][G]: 0 the mean cos_0 and 1 the mean cos_f (Welford's mu); 2 the mean n_kept (the whole-number sum / S); 3 the
 *   smallest and 4 the largest n_kept; 5 the largest change; 6 the mean trials (sum / S).  NaN for an undefined or left-out tumour.
 * series [BNMF_PRN_NSER][S]: per used sample 0 the mean n_kept and 1 the mean cos_f over the defined members: the canonical W = 1024 sum
 *   over the member positions (an undefined member entered as +0.0; bnmf_reconstruction's series order), divided by the number of defined
 *   members (NaN without one).
 * signature [BNMF_PRN_NSIG][N], over the defined members ascending: 0 the number with p_kept >= 0.5; 1 the mean p_kept and 2 the sum of
 *   the mean loads (row 0 of load), both the canonical W = 64 sum, row 1 divided by their number (NaN without one).
 * exposures [S][N*G]: every used sample's e_sparse, laid out as E (n + N g), as bnmf_project's exposures; NaN for an undefined or
 *   left-out tumour.
 * info (sizeof = 48): n_used = S, n_included = m, n_undefined, n_single = the defined members whose largest n_kept is 1, n_steps and
 *   max_loss as given, trials = all trials of the call, max_change = the largest change of any defined member (from +0.0).
 * n_steps = 20 and max_loss = 0.01 are the defaults of the Python and R layers: reporting conventions like min_cosine = 0.9, not tests.
 * The bits depend on the samples, used[], include[], the data, n_steps and max_loss only: not on a tumour's place, the batch of samples
 * that passes through the scratch (at most 256 MB; BNMF_PRN_BATCH overrides the batch for tests), the tiling or the form of the kernel
 * (BNMF_PRN_FORM = 1 asks for the form with the lane's vectors in the LDS at any N).  A tumour's own values involve no other tumour and
 * every sum over tumours runs over the member list, so include[] gives the bits of a cohort without the tumours left out.  Reads only the
 * P, E and A rings and the data; draws no random number, consumes none of the chain's streams and is read-only for the chain.
 * bnmf_prune_at: the n_samples iterations that end at end_iter; the range rule, used[], BNMF_ESIZE and BNMF_ESTATE as for bnmf_project_at;
 * bnmf_prune(h, n, ...) is bnmf_prune_at(h, iter, n, ...).  Every output array may be NULL.  Refused before any device work: a null info
 * (BNMF_EINVAL); the Normal likelihood (BNMF_EMODEL: the KL update needs counts); a used[] or include[] value other than 0 / 1 (the index
 * named), n_steps outside 1 .. 100000, a max_loss that is not finite (BNMF_EINVAL); no used sample, no included tumour,
 * N > BNMF_PRN_MAX_N (BNMF_ESIZE); window = 0, a poisoned handle or nothing recorded (BNMF_ESTATE). */
#define BNMF_PRN_NLOAD 4         /* load rows: mean sparse exposure, its variance, mean share, p_kept */
#define BNMF_PRN_NTUM  7         /* tumour rows: mean cos_0, mean cos_f, mean / smallest / largest n_kept, largest change, mean trials */
#define BNMF_PRN_NSER  2         /* series rows: mean n_kept, mean cos_f */
#define BNMF_PRN_NSIG  3         /* signature rows: tumours with p_kept >= 0.5, mean p_kept, sum of the mean loads */
#define BNMF_PRN_MAX_N 128       /* the most factors */
typedef struct { int32_t n_used, n_included, n_undefined, n_single, n_steps, _pad; int64_t trials; double max_change, max_loss; } bnmf_prune_info;
int bnmf_prune(bnmf_handle*, int last_n, const int32_t* used,
               const int32_t* include /* [G] 0 / 1, NULL = all */, int n_steps, double max_loss,
               double* load      /* [BNMF_PRN_NLOAD][N*G]; may be NULL */,
               double* tumour    /* [BNMF_PRN_NTUM][G]; may be NULL */,
               double* series    /* [BNMF_PRN_NSER][S]; may be NULL */,
               double* signature /* [BNMF_PRN_NSIG][N]; may be NULL */,
               double* exposures /* [S][N*G]; may be NULL */,
               bnmf_prune_info* info);
int bnmf_prune_at(bnmf_handle*, int end_iter, int n_samples, const int32_t* used, const int32_t* include, int n_steps, double max_loss, double* load,
                  double* tumour, double* series, double* signature, double* exposures, bnmf_prune_info* info);

/* Cohort summary of signatures over recorded samples, on the device: how is a signature's load distributed across the
 * cohort?  Per recorded sample the median and the other quantiles of its load among all tumours and among its carriers, its prevalence, its
 * total and its part of the cohort's mutations: one draw each from the posterior of that statistic.  (The reference package's summary()
 * reports the carriers' median and the prevalence of the MAP point estimate alone.)  The members are the m included tumours g_0 < g_1 <
 * ... (include[g] != 0; NULL = all), position i = 0 .. m-1.  The samples are the recorded ones flagged in used[] (oldest first; NULL =
 * all), S of them.  perm [last_n][N] (row-major, a row per sample of the whole range, read for the used ones) is bnmf_relabel's: a row of -1
 * throughout leaves the sample out (every value of its series row is NaN); every other row must be a permutation of 0 .. N-1; NULL is the
 * identity.  The aligned samples are S_a of the S used ones.  Per aligned sample s and factor n, with cs_s[n] bnmf_map's column sum of P_s:
 *   x_i = (A_s[n] != 0 ? E_s[n,g_i] * cs_s[n] : +0.0) + 0.0     bnmf_contrast's renormalised load; + 0.0 maps -0.0 to +0.0, so ties carry
 *                                                               one bit pattern
 *   t_i = sum_n x_s[n,g_i]                                      n ascending from +0.0
 *   u_i = t_i > 0 ? 1 / t_i : 0.0;   r_i = x_i * u_i + 0.0      bnmf_contrast's share
 *   b_i = (x_i >= min_load);   c = #b
 * Every value goes to the place of its label perm[s][n].  With canonB bnmf_regress's blocked canonical sum over the members:
 *   prevalence   = c / m
 *   total        = canonB_i(x_i)
 *   fraction     = total_n / sum_n' total_n' (n' ascending from +0.0); NaN unless the denominator is > 0
 *   mean_present = canonB_i(b_i ? x_i : +0.0) / c; NaN for c = 0
 * and per level p = probs[l], l = 0 .. L-1 (1 <= L <= BNMF_SUM_MAX_Q, every level in [0, 1], strictly ascending) the type-7 order
 * statistic of a set sorted ascending y[0 .. k):  h = (double)(k - 1) * p, j = floor(h), g = h - j, a = y[j], b = y[min(j + 1, k - 1)],
 * the value a == b ? a : (1.0 - g) * a + g * b (bnmf_map's map_interp):
 *   load_all[l]      of the m loads x_i
 *   load_present[l]  of the c loads with b_i (the suffix [m - c, m) of the sorted loads); NaN for c = 0
 *   share_all[l]     of the m shares r_i
 * If a load or a share of the factor among the members is not finite in a sample, its 3 L order statistics of that sample are NaN and
 * the (sample, factor) is counted in info.n_nonfinite.  Where the sample excludes the factor every x is +0.0 and the formulas apply as
 * they stand.  The NSTAT = 4 + 3 L statistics are numbered prevalence, total, fraction, mean_present, load_all[0 .. L), load_present[0 ..
 * L), share_all[0 .. L).
 * stat [NSTAT][BNMF_SUM_NROW][N]: per statistic and label over the S' samples whose value is not NaN rows 0 the mean (the canonical W = 64
 *   sum / S'), 1 the variance in its S' - 1 form (NaN for S' < 2), 2 and 3 the type-7 quantiles at (1 -+ credible_interval) / 2 (NaN for
 *   credible_interval <= 0), 4 n_valid = S'; rows 0 - 3 NaN for S' = 0.
 * series [NSTAT][S][N]: every used sample's values.
 * info (sizeof = 48): n_used = S, n_aligned = S_a, n_included = m, n_left_out = G - m, n_levels = L, n_blocks = the blocks of canonB,
 *   n_nonfinite, min_load and credible_interval as given.
 * Only + - * /, comparisons and counts in a fixed order; an order statistic is exact and does not depend on any order of evaluation.  The
 * bits depend on the samples, used[], include[], perm, min_load, probs and credible_interval only: not on the form of the kernel (a cohort
 * of more than 16,384 members is sorted in chunks and every order statistic selected across them; BNMF_SUM_CHUNK asks for smaller chunks)
 * or the batch of samples that passes through the scratch (at most 256 MB; BNMF_SUM_BATCH overrides the batch), both for tests.  Reads
 * only the P, E and A rings; works for every likelihood and prior, real-valued data with negative loads included; draws no random number,
 * consumes none of the chain's streams and is read-only for the chain.  bnmf_summary_at: the n_samples iterations that end at end_iter;
 * the range rule, used[], BNMF_ESIZE and BNMF_ESTATE as for bnmf_waic_at; bnmf_summary(h, n, ...) is bnmf_summary_at(h, iter, n, ...).
 * stat and series may each be NULL.  Refused before any device work, with BNMF_EINVAL: a null info or probs; a used[] or include[] value
 * other than 0 / 1 (the index named); a perm row that is neither a permutation nor -1 throughout (the sample named); a min_load that is
 * NaN, infinite or negative; L outside 1 .. BNMF_SUM_MAX_Q; a level that is NaN, outside [0, 1] or not above the level before it (the
 * index named); a credible_interval that is NaN or >= 1.  With BNMF_ESIZE: fewer than 2 used samples, fewer than 2 aligned samples, m < 1,
 * m > BNMF_COA_MAX_M.  With BNMF_ESTATE: window = 0, a poisoned handle or nothing recorded. */
#define BNMF_SUM_MAX_Q 8         /* the most levels */
#define BNMF_SUM_NROW  5         /* stat rows: mean, variance, lower, upper, n_valid */
#define BNMF_SUM_NSCAL 4         /* the statistics before the order statistics: prevalence, total, fraction, mean_present */
typedef struct { int32_t n_used, n_aligned, n_included, n_left_out, n_levels, n_blocks; int64_t n_nonfinite; double min_load, credible_interval; } bnmf_summary_info;
int bnmf_summary(bnmf_handle*, int last_n, const int32_t* used,
                 const int32_t* include /* [G] 0 / 1, NULL = all */,
                 const int32_t* perm /* [last_n][N] row-major (bnmf_relabel's), NULL = identity */,
                 double min_load, const double* probs /* [L] */, int L, double credible_interval,
                 double* stat   /* [4 + 3 L][BNMF_SUM_NROW][N]; may be NULL */,
                 double* series /* [4 + 3 L][S][N]; may be NULL */,
                 bnmf_summary_info* info);
int bnmf_summary_at(bnmf_handle*, int end_iter, int n_samples, const int32_t* used, const int32_t* include, const int32_t* perm, double min_load,
                    const double* probs, int L, double credible_interval, double* stat, double* series, bnmf_summary_info* info);

/* Label-switching correction of a recorded range, on the device.  The model is invariant under permutations of its factors,
 * so a chain may exchange two labels at any iteration; every element-wise summary (bnmf_map, bnmf_mixing, bnmf_attribution) then mixes
 * signatures.  This call aligns every recorded sample flagged in used[] (oldest first; NULL = all), numbered s = 0 .. S-1, to a pivot and
 * iterates the pivot to the aligned mean.  All N factors take part, included or not, as in bnmf_label_switching.  Round r = 1, 2, ...:
 *   pivot: K x N.  Round 1: pivot_P (column-major), or with NULL the newest used sample's P; later the aligned mean of the last round.
 *   C_s[n][j] = dot / sqrt(nn * refnorm2[j]), dot = sum_k P_s[k,n] pivot[k,j], nn = sum_k P_s[k,n]^2, refnorm2[j] = sum_k pivot[k,j]^2: the
 *     cosine of the raw P_s[, n] with pivot column j, the sums over k ascending from +0.0 (the operations bnmf_assign votes with).
 *   perm[s][.] = the assignment n -> j that maximises sum_n C_s[n][perm[s][n]] (shortest augmenting paths with potentials, rows in order,
 *     the lowest column among equal reduced costs): perm[s][n] is the label factor n of sample s receives; cosine[s][n] = C_s[n][perm[s][n]].
 *   A sample without an assignment (a cosine that is not finite: a zero column of P_s) is unmatched: perm[s][.] = -1, cosine[s][.] = NaN, it
 *     enters no sum and its aligned_* rows are NaN.  The others are the S' aligned samples, in order.  Fewer than 2 of them: BNMF_ESIZE.
 *   x_s[k,n] = P_s[k,n] / cs_s[n], e_s[n,g] = E_s[n,g] * cs_s[n], cs_s = colSums(P_s): bnmf_map's renormalisation.  With inv_s the inverse of
 *     perm[s][.], the aligned series of element (k, j) of P is x_s[k, inv_s(j)] and of element (j, g) of E e_s[inv_s(j), g], over the aligned
 *     samples;  mean = canon(series) / S',  var = canon((series - mean)^2) / (S' - 1),  canon the canonical W = 64 sum of bnmf_mixing.
 *   The next pivot is the aligned mean of P.  The rounds stop after the first in which no aligned sample's permutation differs from the round
 *   before (round 1: from the identity) — converged = 1 — or after max_rounds.
 * perm [S][N] and cosine [S][N] row-major, of the last round;  confusion [N][N] row-major: the aligned samples with perm[s][n] == j;
 * P_out [BNMF_NREL][K*N], E_out [BNMF_NREL][N*G]: mean and variance, each row column-major as P and E;  aligned_P [S][K*N], aligned_E [S][N*G]:
 * the aligned samples themselves (caller-sized: S times the matrix; they leave the device in batches of at most 256 MB).  Every output but
 * info may be NULL.  info: mean_cosine = canon over the S' N final cosines in (s, n) order / (S' N), min_cosine the smallest of them and
 * min_cosine_at = s * N + n its place (the first wins a tie).  Only + - * /, sqrt and comparisons in a fixed order: the same call gives
 * the same bits, whatever the batches.  Read-only for the chain.
 * bnmf_relabel_at: the n_samples iterations that end at end_iter; the range rule and BNMF_ESIZE as for bnmf_map_at;
 * bnmf_relabel(h, n, ...) is bnmf_relabel_at(h, iter, n, ...).  Refused before any device work: null info, a used[] value other than 0 / 1
 * (the index named), max_rounds < 1 and a pivot_P with a NaN, an infinite value or an all-zero column (the column named) with BNMF_EINVAL,
 * fewer than 2 used samples with BNMF_ESIZE, window = 0 or a poisoned handle with BNMF_ESTATE. */
#define BNMF_NREL 2   /* rows of P_out / E_out: mean, variance (S' - 1 form) */
typedef struct { int32_t n_used, n_aligned /* S' */, n_unmatched, rounds, converged /* the last round changed no permutation */,
                 n_switched /* aligned samples whose final permutation is not the identity */, n_changed_last, _pad;
                 double mean_cosine, min_cosine; int64_t min_cosine_at /* s * N + n */; } bnmf_relabel_info;
int bnmf_relabel(bnmf_handle*, int last_n, const int32_t* used /* [last_n], NULL = all */,
                 const double* pivot_P /* K x N column-major, NULL: the newest used sample's P */, int max_rounds,
                 int32_t* perm /* [S][N] */, double* cosine /* [S][N] */, int64_t* confusion /* [N][N] row-major */,
                 double* P_out /* [BNMF_NREL][K*N] */, double* E_out /* [BNMF_NREL][N*G] */,
                 double* aligned_P /* [S][K*N] */, double* aligned_E /* [S][N*G] */, bnmf_relabel_info* info);
int bnmf_relabel_at(bnmf_handle*, int end_iter, int n_samples, const int32_t* used, const double* pivot_P, int max_rounds,
                    int32_t* perm, double* cosine, int64_t* confusion, double* P_out, double* E_out,
                    double* aligned_P, double* aligned_E, bnmf_relabel_info* info);

int bnmf_get_iter(bnmf_handle* h, int* iter);

/* A chain's state in a file, and back (checkpoint / resume; the reference's save_object, saveRDS(self), R/bayesNMF_sampler.R:414-416).
 * The file is self-describing and deterministic: magic, a format version of its own, the bnmf_config without device,
 * a hash of the data as the handle holds it and of the temperature schedule, then records, each with since_iter, iter, typed sections
 * and a checksum.  A record holds what the chain's future and every kept read depend on: P, E, A, R, sigmasq, the current prior
 * parameters, the MH acceptance arrays, ZsumK / ZsumG (Poisson), Z and its records (save_Z), the record_sample rings of the kept
 * iterations [max(1, iter - window + 1), iter], the loglikelihood / logposterior / acceptance history of the MAP metrics; the base
 * record also the hyper-prior values.  What the next bnmf_run recomputes is not saved.
 * bnmf_save_state: since_iter = 0 writes a full record (the file is created or truncated); since_iter = S > 0 appends a delta — the
 *   file's last record must be this chain at iteration S — with the current state and the kept samples of iterations S+1 .. iter.
 *   Read-only for the chain: a chain that saves gives the same bits as one that does not.  bytes_written may be NULL.
 * bnmf_load_state: replays every record of `path` into a handle that bnmf_create / bnmf_create_f64 has just made with the same config
 *   and data, before bnmf_init (instead of it); the handle is then at the last record's iteration (*iter_out, may be NULL) and
 *   continues bit for bit as the saved chain would have.  Refused (BNMF_EINVAL / BNMF_ESTATE, the mismatch named) before any device
 *   write: another K / G / N, model, seed, chain_id, window or save_Z, other data, another schedule, bad magic or version, a truncated
 *   file or a bad checksum (the record named), a delta that does not follow its predecessor, a handle that has run.
 * bnmf_state_info: validates `path` (every checksum) and describes it without a handle and without a device. */
typedef struct {
  int32_t K, G, N, likelihood, prior, MH, learning_rank, rank_method, save_Z, window;
  uint64_t seed;
  uint32_t chain_id;
  int32_t format_version;
  int64_t n_temperature;
  uint64_t data_hash, temperature_hash;
  int32_t first_iter, last_iter, n_records, _pad;   /* first_iter: the full record's iteration; last_iter: where a load ends */
  int64_t bytes;
} bnmf_state_desc;
int bnmf_save_state(bnmf_handle* h, const char* path, int since_iter, size_t* bytes_written);
int bnmf_load_state(bnmf_handle* h, const char* path, int* iter_out);
int bnmf_state_info(const char* path, bnmf_state_desc* out);
/* sizes of the handle's per-iteration buffers (bench.py's byte counts): what = 0 bytes of item records written per iteration (save_Z on the
 * sorted schedule: samples$Z is kept as these records and expanded when read), 1 bytes of Mhat left for the per-column metric terms,
 * 2 whether samples$Z is a ring of records, 3 whether Z is expanded every iteration (BNMF_ZEAGER=1), 4 whether the MH sweep hosts what followed
 * its two kernels inside them (Poisson MH models at fixed rank; BNMF_MHPIPE=0: no), 5 the quads (4 counts) per item of the sorted schedule,
 * 6 the blocks (workgroups) of the static allocation schedule, 7 how many of them have no column of their own (sorted schedule),
 * 8 the number of columns of P held fixed (bnmf_set_fixed), 9 the form of the MH / Normal row sweep (1 Mhat in registers, 2 Mhat in memory; 0: no such
 * sweep), 10 the launches of the merged draw kernel so far, 11 whether the allocation kernel is k_zalloc_step.
 * BNMF_MHAT (bnmf_get_array; tests): the rows of Mhat as the last row sweep of the MH / Normal models left them, P_t diag(A) E_(t-1),
 * maintained factor by factor.  Readable where the sweep keeps them in memory (statistic 9 == 2: more than 5,120 columns, or a handle
 * created under BNMF_MHREG=0, which takes that form whatever G — the same bits, slower); else BNMF_EUNSET. */
int bnmf_get_stat(bnmf_handle* h, int what, double* out);

/* average device time (ms) of each kernel class over n_iter iterations, measured with HIP
 * events on the handle's own stream (advances the chain by n_iter iterations).
 * out_ms[BNMF_NKERNEL]; names from bnmf_kernel_name(). */
#define BNMF_NKERNEL 8
int bnmf_profile(bnmf_handle* h, int n_iter, int converged, double* out_ms);
const char* bnmf_kernel_name(int i);

/* measured ceilings of the device for bench.py's roofline: Philox4x32-7 words per second (the count-allocation generator) alone in a loop
 * (one word per allocated count: the floor of sample_Zkg, R/sample_params.R:253-265) and the device-to-device copy
 * bandwidth in GB/s (read + write), next to the nominal 8 TB/s */
int bnmf_ubench(int device, double* philox_words_per_s, double* copy_gbs);

/* device-side unit probes used by the parity tests (tests/test_gpu_*.py) */
int bnmf_test_math(int device, int fn, const double* in, double* out, size_t n);
/* which: 0 rgamma(a, b), 1 rtnorm0(a, b), 2 rnorm, 3 ralpha(a, b, c), 4 runif, 5 rexp(a), 6 ralpha_fast(a, b, c), 7 ralpha_fast_wave(a, b, c):
 * the wave-cooperative form of 6 (every lane of every wave calls it; the lanes past n take part without an element), 8 rpois(a): a whole
 * number in a double, 1e-6 <= a <= 2^24 (b and c are not read) */
int bnmf_test_sampler(int device, int which, uint64_t seed, uint32_t chain, uint32_t var,
                      uint32_t elem0, uint32_t iter, const double* a, const double* b,
                      const double* c, double* out, size_t n);
int bnmf_test_philox(int device, const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]);    /* Philox4x32-10 */
int bnmf_test_philox7(int device, const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]);   /* Philox4x32-7: the count-allocation words */

/* diagnostics of the builder's own tools and tests (tools/rankdbg.py, tools/zsprof.py, tools/zpprof.py, tests/test_gpu_parity.py):
 * phase time stamps of the rank sweep (BNMF_RANKDBG=1 at bnmf_create; returns the grid size), section ticks of the allocation
 * kernel (-DZSPROF / -DZPPROF builds only, else BNMF_ESTATE), and what a bounded in-kernel wait does when it gives up
 * (word 0: a draw kernel waiting for the hyper sweep, word 1: the rank sweep's exchange).  Not part of the drop-in boundary. */
/* host-only checks (no GPU) of what keeps the chains that share a device apart (api.hip DeviceGate, devlock_open; tests/test_abi_host.py):
 * the writer-preferring gate under overlapping sharers (how long the exclusive caller waited, sharers admitted while it did: 0), and the
 * opening of the device's two lock files under BNMF_LOCKDIR (or /tmp) with the lock order of bnmf_run.  Not part of the drop-in boundary. */
int bnmf_test_gate(int n_sharers, int calls_per_sharer, int hold_us, long* excl_wait_us, long* admitted_while_waiting);
int bnmf_test_devlock(const char* bus_tag, int* lock_ok, int* gate_ok);
/* host-only (no GPU): the static schedules of the allocation kernels as bnmf_create would plan them for this data on a device of n_cu
 * compute units, under the same environment switches (tests/test_schedule_host.py).  Every array may be NULL (size query: desc alone).
 * zsort: desc[14] = accepted, KP, GBc, blocks, waves, quads per item, 2-byte items, pk, large cells spread, blocks without an own column,
 *   ints of the column list as uploaded, items, words of Mblk, threshold blocks; blocks[4 per block] = item0, ntask, col0, ncols; items
 *   (4-byte form, always) and items16 (if 2-byte items are chosen: what is uploaded).
 * zstep: desc[11] = accepted, row chunks, workgroups, waves, GBP, 2-byte items, largest fragment index, batches, steps, columns, items;
 *   wgs[2 per workgroup] = batch0, nbatch; batches[2 per batch] = col0, ncols; steps[16 bytes per step] = int64 item0, int32 ntw, pad. */
int bnmf_test_zsort_plan(int K, int G, int N, int save_Z, int n_cu, const int32_t* M, long long* desc, int32_t* blocks, int32_t* cols,
                         uint32_t* items, uint16_t* items16, int32_t* Mblk);
int bnmf_test_zstep_plan(int K, int G, int N, int save_Z, int n_cu, const int32_t* M, long long* desc, int32_t* wgs, int32_t* batches,
                         void* steps, int32_t* cols, uint32_t* items, uint16_t* items16);
int bnmf_debug_rank(bnmf_handle* h, unsigned long long* out, size_t n);
int bnmf_debug_zsort(bnmf_handle* h, unsigned long long* out);
int bnmf_debug_set_timeout(bnmf_handle* h, int word);

/* Can two kernels on two streams of this device run at the same time?  Measured once per device and process by a two-stream
 * hand-off (kernel A spins, bounded, on a word kernel B sets).  bnmf_create uses it to choose between flag polling inside the
 * kernels (overlap) and stream waits on events ("serial-safe mode": counter collection, AMD_SERIALIZE_KERNEL, HIP_LAUNCH_BLOCKING
 * and any other tool that serialises dispatches).  *overlap = 1 / 0. */
int bnmf_probe_overlap(int device, int* overlap);

/* What destroyed handles leave cached on a device for the next handle — their record_sample rings (up to BNMF_RING_CACHE_GB, default 8)
 * and three HIP streams each — is released; bytes_released (may be NULL) = device memory given back. */
int bnmf_trim(int device, size_t* bytes_released);

int bnmf_device_info(int device, char* buf, size_t buflen);
int bnmf_device_count(void);
const char* bnmf_last_error(void);
int bnmf_version(void);

#ifdef __cplusplus
}
#endif
#endif
