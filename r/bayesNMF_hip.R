# r/bayesNMF_hip.R — reference-side binding: how bayesNMF_sampler is switched to the HIP engine.
#
# A subclass of the reference's R6 class that keeps every public field and method and replaces only the
# four private methods the loop body calls (R/bayesNMF_sampler.R:273-285: sample_prior_params,
# sample_params, record_sample, update_sample_metrics) by ONE `.Call` per block of iterations.
# Everything else (get_MAP, check_convergence, logging, save_object, summary/plot) is the reference's
# own code operating on fields that are refreshed from the device at block boundaries.
# EXPERIMENTAL: not runnable in this repository's container (no R).  The Python mirror bayesnmf_amd/sampler.py is
# the tested equivalent and performs the same C-ABI call sequence; keep this file logic-free.  The MAP checks use
# bnmf_map (get_MAP_ on the device: no window copy), the warm-up loop and the MH tail one call each (bnmf_run_until,
# bnmf_run_post_warmup) unless periodic_save asks for the block-by-block loop; the recorded samples are materialised
# into self$samples ONCE, at the end; assign_signatures_ensemble goes through bnmf_assign (bnmf_assign_at for a MAP of an earlier
# range, get_MAP(end_iter, n_samples) -> bnmf_map_at), label_switching_df through bnmf_label_switching.  See INTEGRATION.md.
# The handle is an external pointer: readRDS of a saved sampler gives a dead one.  With save_engine_state = TRUE every save_object()
# also writes the device state to engine_state.bin (a full record, then deltas: bnmf_save_state), and load_bayesNMF_hip(output_dir)
# (end of this file) reads sampler.rds back, recreates the handle with the stored spec and replays that file into it (bnmf_load_state).

.bnmf_ids <- c(P = 0L, E = 1L, A = 2L, R = 3L, Z = 4L, sigmasq = 7L,
               Alpha_p = 10L, Beta_p = 11L, Alpha_e = 12L, Beta_e = 13L, Mu_p = 14L, Sigmasq_p = 15L,
               Mu_e = 16L, Sigmasq_e = 17L, Lambda_p = 18L, Lambda_e = 19L,
               A_p = 30L, B_p = 31L, C_p = 32L, D_p = 33L, M_p = 34L, S_p = 35L,
               A_e = 40L, B_e = 41L, C_e = 42L, D_e = 43L, M_e = 44L, S_e = 45L,
               P_acceptance_rate = 50L, E_acceptance_rate = 51L)
.bnmf_metric_names <- c("iter", "RMSE", "KL", "loglikelihood", "logposterior", "n_params", "BIC", "rank", "temp",
                        "P_mean_acceptance_rate", "E_mean_acceptance_rate")

bayesNMF_sampler_hip <- R6::R6Class(
  "bayesNMF_sampler", inherit = bayesNMF::bayesNMF_sampler,
  public = list(
    handle = NULL,
    # fixed_P (K x F): known signatures held fixed as columns 1..F of P, never drawn (bnmf_set_fixed).  The rank, or the top of a rank
    # range, must be >= F; F == rank is a refit (only E is sampled).  Checked before the reference constructor runs.
    initialize = function(..., seed = 1, chain_id = 0L, device = 0L, save_Z = FALSE, save_engine_state = FALSE, fixed_P = NULL) {
      private$hip <- list(seed = seed, chain_id = chain_id, device = device, save_Z = save_Z, save_engine_state = save_engine_state,
                          state_iter = 0L, post_warmup_done = 0, fixed_P = private$check_fixed_P(fixed_P))
      super$initialize(...)     # runs the reference constructor; its prior draws are redirected below
    },
    # save_object (R/bayesNMF_sampler.R:414-416): sampler.rds, then (save_engine_state) the device state beside it — a full record at
    # the first save, a delta since the previous save afterwards
    save_object = function() {
      since <- private$hip$state_iter
      if (isTRUE(private$hip$save_engine_state)) private$hip$state_iter <- as.integer(self$state$iter)
      super$save_object()
      if (isTRUE(private$hip$save_engine_state)) {
        path <- file.path(self$specs$output_dir, "engine_state.bin")
        if (since == 0L || !file.exists(path)) .Call("C_bnmf_save_state", self$handle, path, 0L)
        else if (since < self$state$iter) .Call("C_bnmf_save_state", self$handle, path, as.integer(since))
      }
      invisible(self)
    },
    run_gibbs_sampler = function() {
      cc <- self$specs$convergence_control
      start_time <- Sys.time()
      if (!self$specs$periodic_save) {
        private$absorb(.Call("C_bnmf_run_until", self$handle, private$cc_int(), as.double(cc$tol), private$cc_state()), cc)
      }
      while (!self$state$converged & self$state$iter < cc$maxiters) {        # block-by-block (periodic_save)
        nxt <- (self$state$iter %/% cc$MAP_every + 1) * cc$MAP_every
        private$run_block(min(nxt, cc$maxiters) - self$state$iter, converged = FALSE)
        it <- self$state$iter
        if ((it %% cc$MAP_every == 0 & it >= max(cc$MAP_over, cc$MAP_every)) | it >= cc$maxiters) {
          self$get_MAP()
          msg <- private$check_convergence(); self$log(msg, verbosity = 1)
          if (self$specs$periodic_save) self$save_object()
        }
      }
      if (self$specs$MH) {
        if (!self$specs$periodic_save) {
          private$absorb(.Call("C_bnmf_run_post_warmup", self$handle, private$cc_int(), as.double(cc$tol), private$cc_state(),
                               as.integer(self$specs$post_warmup)), cc)
          self$get_MAP(final = TRUE)
        } else {
          done <- private$hip$post_warmup_done                 # (a sampler reopened by load_bayesNMF_hip continues its tail)
          while (done < self$specs$post_warmup) {
            nxt <- (self$state$iter %/% cc$MAP_every + 1) * cc$MAP_every
            n <- min(nxt - self$state$iter, self$specs$post_warmup - done)
            private$run_block(n, converged = TRUE); done <- done + n; private$hip$post_warmup_done <- done
            if (self$state$iter %% cc$MAP_every == 0 | done == self$specs$post_warmup) {
              self$get_MAP(final = done == self$specs$post_warmup)
              private$check_convergence(final = done == self$specs$post_warmup)
              self$save_object()
            }
          }
        }
      } else self$get_MAP(final = TRUE)
      private$pull_state(); private$pull_window()      # self$params / self$samples for summary(), plot(), saveRDS: once
      self$time$total <- difftime(Sys.time(), start_time, units = "mins")
      self$time$per_iter <- self$time$total / self$state$iter
      self$save_object()
    },
    # get_MAP_ (R/utils.R:194-288) on the device: mode of A, renormalised means, 95 % bounds at the final MAP.  end_iter = iter: the
    # window state$MAP_idx (n_samples is not used, as in the reference); another end_iter (save_all_samples only): iterations
    # end_iter - n_samples + 1 ... end_iter (bnmf_map_at)
    get_MAP = function(end_iter = self$state$iter, n_samples = self$specs$convergence_control$MAP_over, final = FALSE,
                       credible_interval = 0.95) {
      if (!self$specs$save_all_samples & end_iter != self$state$iter) {
        stop("end_iter cannot be provided unless self$specs$save_all_samples is TRUE")
      }
      if (end_iter == self$state$iter) {
        n <- min(self$specs$convergence_control$MAP_over, self$state$iter)
        r <- .Call("C_bnmf_map", self$handle, as.integer(n), as.double(if (final) credible_interval else 0),
                   c(self$dims$K, self$dims$G, self$dims$N))
      } else {
        n <- n_samples
        r <- .Call("C_bnmf_map_at", self$handle, as.integer(end_iter), as.integer(n), as.double(if (final) credible_interval else 0),
                   c(self$dims$K, self$dims$G, self$dims$N))
      }
      keep <- if (final) which(r$A[1, ] == 1) else seq_len(self$dims$N)
      first <- end_iter - n + 1
      pats <- apply(r$top_A[seq_len(min(5, r$n_patterns)), , drop = FALSE], 1, paste, collapse = "")
      self$MAP <- list(P = r$P[, keep, drop = FALSE], A = r$A[, keep, drop = FALSE], E = r$E[keep, , drop = FALSE],
                       idx = first + which(r$used) - 1, A_counts = stats::setNames(r$top_counts[seq_along(pats)], pats),
                       keep_sigs = keep, RMSE = r$rmse, KL = r$kl)
      if (final) self$credible_intervals <- list(P = list(lower = r$P_lower[, keep, drop = FALSE], upper = r$P_upper[, keep, drop = FALSE]),
                                                 E = list(lower = r$E_lower[keep, , drop = FALSE], upper = r$E_upper[keep, , drop = FALSE]))
      invisible(self$MAP)
    },
    # assign_signatures_ensemble_ (R/postprocessing.R:175-341) on the recorded samples MAP$idx: cosine matrices on the device
    assign_signatures_ensemble = function(reference_P, credible_interval = 0.95) {
      n <- min(self$specs$convergence_control$MAP_over, self$state$iter)
      keep <- rep(FALSE, self$dims$N); keep[self$MAP$keep_sigs] <- TRUE
      Pfull <- matrix(0, self$dims$K, self$dims$N); Pfull[, self$MAP$keep_sigs] <- self$MAP$P
      if (min(self$MAP$idx) > self$state$iter - n) {          # within the last window
        used <- rep(FALSE, n); used[self$MAP$idx - (self$state$iter - n)] <- TRUE
        r <- .Call("C_bnmf_assign", self$handle, as.integer(n), used, as.matrix(reference_P), keep, Pfull, as.double(credible_interval),
                   c(self$dims$K, self$dims$G, self$dims$N))
      } else {                                                # a MAP of get_MAP(end_iter, n_samples): min(idx) ... max(idx)
        first <- min(self$MAP$idx); last <- max(self$MAP$idx)
        used <- rep(FALSE, last - first + 1); used[self$MAP$idx - first + 1] <- TRUE
        r <- .Call("C_bnmf_assign_at", self$handle, as.integer(last), as.integer(last - first + 1), used, as.matrix(reference_P), keep, Pfull,
                   as.double(credible_interval), c(self$dims$K, self$dims$G, self$dims$N))
      }
      self$reference_comparison$reference_P <- reference_P
      self$reference_comparison$votes <- r$votes[self$MAP$keep_sigs, , drop = FALSE]
      self$reference_comparison$assignments <- data.frame(sig = self$MAP$keep_sigs, ref = colnames(reference_P)[r$assigned[self$MAP$keep_sigs]],
                                                          cos_sim = r$MAP_cosine[self$MAP$keep_sigs], lower = r$lower[self$MAP$keep_sigs],
                                                          upper = r$upper[self$MAP$keep_sigs])
      self$reference_comparison$idxs <- self$MAP$idx
      invisible(self$reference_comparison)
    },
    # The Watanabe-Akaike criterion over recorded samples, on the device (bnmf_waic_at; not in the reference): iterations
    # end_iter - n_samples + 1 ... end_iter (defaults as get_MAP: the last MAP_over samples), restricted to idx — "MAP_idx": MAP$idx,
    # the samples whose A is the mode, all of one rank; NULL: every sample of the range; else a vector of recorded iterations.
    # list(n_used, n_high_var, lppd, p_waic, elpd_waic, waic, se_elpd, mean_loglik), with pointwise also col (G x 3: lppd, p_waic,
    # mean_loglik per column), lppd_cell and p_waic_cell (K x G)
    get_WAIC = function(end_iter = self$state$iter, n_samples = min(self$specs$convergence_control$MAP_over, self$state$iter),
                        idx = "MAP_idx", pointwise = FALSE) {
      first <- end_iter - n_samples + 1
      if (is.character(idx)) {
        if (idx != "MAP_idx") stop("Parameter `idx` must be 'MAP_idx', NULL or a vector of recorded iterations")
        idx <- self$MAP$idx
      }
      used <- NULL
      if (!is.null(idx)) {
        idx <- idx[idx >= first & idx <= end_iter]
        used <- rep(FALSE, n_samples); used[idx - first + 1] <- TRUE
      }
      .Call("C_bnmf_waic", self$handle, as.integer(end_iter), as.integer(n_samples), used, as.logical(pointwise), as.logical(pointwise),
            c(self$dims$K, self$dims$G, self$dims$N))
    },
    # Mixing diagnostics of the recorded samples, on the device (bnmf_mixing_at; not in the reference): for every element of the
    # renormalised P and E over iterations end_iter - n_samples + 1 ... end_iter (defaults as get_WAIC), restricted to idx, the mean,
    # variance, Geyer's effective sample size, Monte-Carlo standard error, split R-hat and the halves' moments: P (K N x 11) and
    # E (N G x 11), columns mean, var, ess, mcse, rhat, pairs, exit, mean_a, var_a, mean_b, var_b; and the summary over the factors of
    # MAP$keep_sigs (counts, smallest ESS and largest R-hat of each side with their 1-based positions, 0 = none).  A lag counts USED samples:
    # where idx leaves gaps in the range the remaining samples are treated as one contiguous series, as get_MAP's idx is.
    get_mixing = function(end_iter = self$state$iter, n_samples = min(self$specs$convergence_control$MAP_over, self$state$iter),
                          idx = "MAP_idx", arrays = TRUE) {
      first <- end_iter - n_samples + 1
      if (is.character(idx)) {
        if (idx != "MAP_idx") stop("Parameter `idx` must be 'MAP_idx', NULL or a vector of recorded iterations")
        idx <- self$MAP$idx
      }
      used <- NULL
      if (!is.null(idx)) {
        idx <- idx[idx >= first & idx <= end_iter]
        used <- rep(FALSE, n_samples); used[idx - first + 1] <- TRUE
      }
      keep <- NULL
      if (!is.null(self$MAP$keep_sigs)) { keep <- rep(FALSE, self$dims$N); keep[self$MAP$keep_sigs] <- TRUE }
      r <- .Call("C_bnmf_mixing", self$handle, as.integer(end_iter), as.integer(n_samples), used, keep, as.logical(arrays),
                 c(self$dims$K, self$dims$G, self$dims$N))
      cols <- c("mean", "var", "ess", "mcse", "rhat", "pairs", "exit", "mean_a", "var_a", "mean_b", "var_b")
      if (!is.null(r$P)) { colnames(r$P) <- cols; colnames(r$E) <- cols }
      r
    },
    # Posterior predictive checks of the recorded samples, on the device (bnmf_ppc_at; not in the reference): over iterations
    # end_iter - n_samples + 1 ... end_iter (defaults as get_WAIC), restricted to idx, a replicate of the data is drawn from every
    # sample's own fit and compared with the data through two discrepancies (Poisson: Freeman-Tukey and the number of zero cells;
    # Normal: the sum of squared standardised residuals and the largest one).  list(n_used, n_tail_cells, p_T1, p_T2, mean_T1_obs,
    # mean_T1_rep, mean_T2_obs, mean_T2_rep, col (G x 6: T1_obs, T1_rep, p_T1, T2_obs, T2_rep, p_T2 per column of the data; a p_T1 near 0
    # marks a column the model reconstructs worse than its own replicates), series (S x 4 per used sample, over the whole matrix)), with
    # pointwise also mean_cell, var_cell, p_less_cell, p_equal_cell and pit = p_less_cell + 0.5 p_equal_cell (K x G)
    get_PPC = function(end_iter = self$state$iter, n_samples = min(self$specs$convergence_control$MAP_over, self$state$iter),
                       idx = "MAP_idx", pointwise = FALSE) {
      first <- end_iter - n_samples + 1
      if (is.character(idx)) {
        if (idx != "MAP_idx") stop("Parameter `idx` must be 'MAP_idx', NULL or a vector of recorded iterations")
        idx <- self$MAP$idx
      }
      used <- NULL
      if (!is.null(idx)) {
        idx <- idx[idx >= first & idx <= end_iter]
        used <- rep(FALSE, n_samples); used[idx - first + 1] <- TRUE
      }
      r <- .Call("C_bnmf_ppc", self$handle, as.integer(end_iter), as.integer(n_samples), used, as.logical(pointwise),
                 c(self$dims$K, self$dims$G, self$dims$N))
      colnames(r$col) <- c("T1_obs", "T1_rep", "p_T1", "T2_obs", "T2_rep", "p_T2")
      colnames(r$series) <- c("T1_obs", "T1_rep", "T2_obs", "T2_rep")
      if (pointwise) r$pit <- r$p_less_cell + 0.5 * r$p_equal_cell
      r
    },
    # Which signature produced the mutations of which tumour, on the device (bnmf_attribution_at; not in the reference): over iterations
    # end_iter - n_samples + 1 ... end_iter (defaults as get_WAIC), restricted to idx, every sample allocates the count of every cell to
    # the factors in proportion to their parts of the fit.  list(load_mean, load_sd, share, p_present (N x G: the mean and standard
    # deviation over the samples of the mutations of tumour g attributed to signature n, its mean share of the tumour, the fraction of
    # samples in which it carries at least min_load mutations), cohort (a data frame with one row per signature: the mean and the
    # credible_interval bounds, quantile type 7, of its load over the whole cohort), n_used, n_present (the (n, g) with p_present >= 0.5),
    # total), with prob also prob (K x N x G: the probability that a mutation of type k in tumour g came from signature n).  Factor n is
    # taken to be the same signature in every sample, as get_MAP takes it.
    get_attribution = function(end_iter = self$state$iter, n_samples = min(self$specs$convergence_control$MAP_over, self$state$iter),
                               idx = "MAP_idx", min_load = 1, credible_interval = 0.95, prob = FALSE) {
      first <- end_iter - n_samples + 1
      if (is.character(idx)) {
        if (idx != "MAP_idx") stop("Parameter `idx` must be 'MAP_idx', NULL or a vector of recorded iterations")
        idx <- self$MAP$idx
      }
      used <- NULL
      if (!is.null(idx)) {
        idx <- idx[idx >= first & idx <= end_iter]
        used <- rep(FALSE, n_samples); used[idx - first + 1] <- TRUE
      }
      K <- self$dims$K; G <- self$dims$G; N <- self$dims$N
      r <- .Call("C_bnmf_attribution", self$handle, as.integer(end_iter), as.integer(n_samples), used, as.double(min_load),
                 as.logical(prob), c(K, G, N))
      a <- (1 - credible_interval) / 2
      out <- list(load_mean = matrix(r$load[, 1], N, G), load_sd = sqrt(matrix(r$load[, 2], N, G)), share = matrix(r$load[, 3], N, G),
                  p_present = matrix(r$load[, 4], N, G),
                  cohort = data.frame(signature = seq_len(N), mean = rowMeans(r$series),
                                      lower = apply(r$series, 1, quantile, probs = a, type = 7, names = FALSE),
                                      upper = apply(r$series, 1, quantile, probs = 1 - a, type = 7, names = FALSE)),
                  n_used = r$n_used, n_present = r$n_present, total = r$total)
      if (prob) out$prob <- array(r$prob, c(K, N, G))
      out
    },
    # How well is every tumour of the cohort reconstructed, and which signatures does it need?  On the device
    # (bnmf_reconstruction_at; not in the reference): over iterations end_iter - n_samples + 1 ... end_iter (defaults as get_WAIC),
    # restricted to idx, every sample gives per tumour the cosine between its data and its fit, the relative L1 error and the RMSE, and
    # per signature the cosine of the fit without it.  The remaining exposures are not refitted after the removal, so the drop is an
    # upper bound of what removing the signature costs the tumour.  list(tumour (6 x G: mean, variance and smallest cosine over the
    # samples, mean relative L1 error, mean RMSE, share of samples with cosine >= min_cosine; NaN for an all-zero tumour) with its rows
    # as cosine, cosine_var, min_cosine_sample, rel_l1, rmse, p_good; drop (4 x N x G: mean and variance of the drop, mean
    # leave-one-out cosine, share of samples with drop >= min_drop) with its rows as drop_mean, drop_var, loo_cosine, p_needed (N x G);
    # series (S), signature (3 x N: tumours that need it, mean and largest mean drop), n_used, n_undefined, n_poor, n_needed,
    # min_cosine, min_drop, worst_cosine, worst_at (1-based tumour; NA if none)).
    get_reconstruction = function(end_iter = self$state$iter, n_samples = min(self$specs$convergence_control$MAP_over, self$state$iter),
                                  idx = "MAP_idx", min_cosine = 0.9, min_drop = 0.01) {
      first <- end_iter - n_samples + 1
      if (is.character(idx)) {
        if (idx != "MAP_idx") stop("Parameter `idx` must be 'MAP_idx', NULL or a vector of recorded iterations")
        idx <- self$MAP$idx
      }
      used <- NULL
      if (!is.null(idx)) {
        idx <- idx[idx >= first & idx <= end_iter]
        used <- rep(FALSE, n_samples); used[idx - first + 1] <- TRUE
      }
      K <- self$dims$K; G <- self$dims$G; N <- self$dims$N
      r <- .Call("C_bnmf_reconstruction", self$handle, as.integer(end_iter), as.integer(n_samples), used, as.double(min_cosine),
                 as.double(min_drop), c(K, G, N))
      drop <- aperm(array(r$drop, c(N, G, 4)), c(3, 1, 2))
      out <- list(tumour = t(r$tumour), drop = drop, series = r$series, signature = t(r$signature),
                  cosine = r$tumour[, 1], cosine_var = r$tumour[, 2], min_cosine_sample = r$tumour[, 3], rel_l1 = r$tumour[, 4],
                  rmse = r$tumour[, 5], p_good = r$tumour[, 6], drop_mean = matrix(r$drop[, 1], N, G), drop_var = matrix(r$drop[, 2], N, G),
                  loo_cosine = matrix(r$drop[, 3], N, G), p_needed = matrix(r$drop[, 4], N, G), n_used = r$n_used,
                  n_undefined = r$n_undefined, n_poor = r$n_poor, n_needed = r$n_needed, min_cosine = r$min_cosine, min_drop = r$min_drop,
                  worst_cosine = r$worst_cosine, worst_at = if (r$worst_at < 0) NA_integer_ else as.integer(r$worst_at) + 1L)
      message(sprintf("Reconstruction: %d of %d tumours below cosine %g, worst %.3g; %d (signature, tumour) pairs with a drop >= %g",
                      as.integer(r$n_poor), G - r$n_undefined, r$min_cosine, r$worst_cosine, as.integer(r$n_needed), r$min_drop))
      out
    },
    # Does the activity of a signature differ between groups of tumours?  On the device (bnmf_contrast_at; not in the reference): groups
    # is a vector of G labels, one per tumour (NA: the tumour is left out), numbered in order of first appearance.  Over iterations
    # end_iter - n_samples + 1 ... end_iter (defaults as get_WAIC), restricted to idx, every sample gives one draw of each group's mean
    # load of every signature (the renormalised exposure of get_MAP), mean share of the tumour's total and prevalence (the fraction of
    # the group's tumours in which the signature carries at least min_load mutations), so the difference of two groups has a posterior.
    # list(names, pair_names (NP x 2: a before b), load, share, prevalence (each a list: mean, var, lower, upper (N x C, quantile type 7
    # at credible_interval) and diff_mean, diff_var, diff_lower, diff_upper, p_greater, p_less (N x NP) of the difference a - b), sizes,
    # n_used, n_groups, n_pairs, n_left_out, n_credible (per statistic the (signature, pair) whose interval excludes 0), min_load,
    # credible_interval), with series also series (N x C x S x 3).  No multiple-testing adjustment is made.
    get_contrast = function(groups, end_iter = self$state$iter, n_samples = min(self$specs$convergence_control$MAP_over, self$state$iter),
                            idx = "MAP_idx", min_load = 1, credible_interval = 0.95, series = FALSE) {
      first <- end_iter - n_samples + 1
      if (is.character(idx)) {
        if (idx != "MAP_idx") stop("Parameter `idx` must be 'MAP_idx', NULL or a vector of recorded iterations")
        idx <- self$MAP$idx
      }
      used <- NULL
      if (!is.null(idx)) {
        idx <- idx[idx >= first & idx <= end_iter]
        used <- rep(FALSE, n_samples); used[idx - first + 1] <- TRUE
      }
      K <- self$dims$K; G <- self$dims$G; N <- self$dims$N
      if (length(groups) != G) stop("groups must have one label per tumour (G = ", G, ")")
      names <- unique(groups[!is.na(groups)])
      labels <- match(groups, names) - 1L
      r <- .Call("C_bnmf_contrast", self$handle, as.integer(end_iter), as.integer(n_samples), used, as.integer(labels), as.double(min_load),
                 as.double(credible_interval), as.logical(series), c(K, G, N))
      C <- r$n_groups; NP <- r$n_pairs
      pairs <- if (NP > 0) t(utils::combn(C, 2)) else matrix(integer(0), 0, 2)
      pair_names <- matrix(as.character(names)[pairs], NP, 2)
      stat <- function(q) {
        o <- list(mean = matrix(r$group[, 4 * q + 1], N, C), var = matrix(r$group[, 4 * q + 2], N, C),
                  lower = matrix(r$group[, 4 * q + 3], N, C), upper = matrix(r$group[, 4 * q + 4], N, C))
        if (NP > 0) {
          rows <- c("diff_mean", "diff_var", "diff_lower", "diff_upper", "p_greater", "p_less")
          for (i in seq_along(rows)) o[[rows[i]]] <- matrix(r$pair[, 6 * q + i], N, NP)
        }
        o
      }
      out <- list(names = names, pair_names = pair_names, load = stat(0), share = stat(1), prevalence = stat(2), sizes = r$sizes,
                  n_used = r$n_used, n_groups = C, n_pairs = NP, n_left_out = r$n_left_out, n_credible = r$n_credible, min_load = r$min_load,
                  credible_interval = r$credible_interval)
      if (series) out$series <- array(r$series, c(N, C, r$n_used, 3))
      message(sprintf("Contrast: groups %s; %d pair(s) %s; n_credible load %g, share %g, prevalence %g",
                      paste(sprintf("%s (%d)", names, r$sizes), collapse = ", "), NP, paste(pair_names[, 1], pair_names[, 2], sep = " - ", collapse = ", "),
                      r$n_credible[1], r$n_credible[2], r$n_credible[3]))
      out
    },
    # Does the activity of a signature follow a covariate of the tumours (age, dose, purity), and is a group difference still there once
    # other covariates are in the model?  On the device (bnmf_regress_at; not in the reference): covariates is a G x Q0 numeric matrix or
    # a data frame of numeric columns, one row per tumour (a row with an NA is left out); intercept prepends the column of ones;
    # standardize centres and scales the other columns by the included rows' mean and sd.  Over iterations end_iter - n_samples + 1 ...
    # end_iter (defaults as get_WAIC), restricted to idx, every sample gives one least-squares fit per signature of its load (the
    # renormalised exposure of get_MAP), of its share of the tumour's total and of the square root of its load: the coefficients over the
    # samples are draws from the posterior of the cohort's own coefficient (the tumours' sampling error is not added).
    # list(names, load, share, sqrt_load (each a list: mean, var, lower, upper, p_greater, p_less (N x Q, quantile type 7 at
    # credible_interval) and r2_mean, r2_lower, r2_upper, r2_samples, sigma2_mean (N)), include, n_used, Q, n_included, n_left_out, n_blocks,
    # min_pivot_ratio, min_pivot_at (the column closest to a combination of those before it), n_credible (Q x 3: the signatures whose
    # interval for a column excludes 0), credible_interval), with series also coef_series (N x Q x S x 3) and r2_series (N x S x 3).
    get_regression = function(covariates, end_iter = self$state$iter, n_samples = min(self$specs$convergence_control$MAP_over, self$state$iter),
                              idx = "MAP_idx", intercept = TRUE, standardize = FALSE, credible_interval = 0.95, series = FALSE) {
      first <- end_iter - n_samples + 1
      if (is.character(idx)) {
        if (idx != "MAP_idx") stop("Parameter `idx` must be 'MAP_idx', NULL or a vector of recorded iterations")
        idx <- self$MAP$idx
      }
      used <- NULL
      if (!is.null(idx)) {
        idx <- idx[idx >= first & idx <= end_iter]
        used <- rep(FALSE, n_samples); used[idx - first + 1] <- TRUE
      }
      K <- self$dims$K; G <- self$dims$G; N <- self$dims$N
      X <- as.matrix(covariates)
      if (!is.numeric(X) || nrow(X) != G) stop("covariates must be numeric with one row per tumour (G = ", G, ")")
      names <- if (is.null(colnames(X))) paste0("x", seq_len(ncol(X))) else colnames(X)
      include <- stats::complete.cases(X)
      if (standardize) for (j in seq_len(ncol(X))) {
        v <- X[include, j]
        if (!(stats::sd(v) > 0)) stop("covariate ", names[j], " is constant over the included tumours: it cannot be standardized")
        X[, j] <- (X[, j] - mean(v)) / stats::sd(v)
      }
      if (intercept) { X <- cbind(1, X); names <- c("(Intercept)", names) }
      storage.mode(X) <- "double"
      r <- .Call("C_bnmf_regress", self$handle, as.integer(end_iter), as.integer(n_samples), used, X, if (all(include)) NULL else include,
                 as.double(credible_interval), as.logical(series), c(K, G, N))
      Q <- r$Q
      stat <- function(q) {
        rows <- c("mean", "var", "lower", "upper", "p_greater", "p_less")
        o <- list()
        for (i in seq_along(rows)) o[[rows[i]]] <- matrix(r$coef[, 6 * q + i], N, Q, dimnames = list(NULL, names))
        frows <- c("r2_mean", "r2_lower", "r2_upper", "r2_samples", "sigma2_mean")
        for (i in seq_along(frows)) o[[frows[i]]] <- r$fit[, 5 * q + i]
        o
      }
      out <- list(names = names, load = stat(0), share = stat(1), sqrt_load = stat(2), include = include, n_used = r$n_used, Q = Q,
                  n_included = r$n_included, n_left_out = r$n_left_out, n_blocks = r$n_blocks, min_pivot_ratio = r$min_pivot_ratio,
                  min_pivot_at = r$min_pivot_at + 1L, n_credible = r$n_credible, credible_interval = r$credible_interval)
      if (series) { out$coef_series <- array(r$coef_series, c(N, Q, r$n_used, 3)); out$r2_series <- array(r$r2_series, c(N, r$n_used, 3)) }
      message(sprintf("Regression: %d tumours included, %d left out; Q = %d, min_pivot_ratio %.3g (column %s); n_credible for the load %s",
                      r$n_included, r$n_left_out, Q, r$min_pivot_ratio, names[r$min_pivot_at + 1L],
                      paste(sprintf("%s %g", names, r$n_credible[, 1]), collapse = ", ")))
      out
    },
    # Similarity of the tumours, on the device (bnmf_similarity_at; not in the reference): which tumours have the exposure profile of
    # this one, does the cohort fall into subtypes, which tumours resemble nobody?  Over iterations end_iter - n_samples + 1 ... end_iter
    # (defaults as get_WAIC), restricted to idx, every sample gives for every pair of included tumours the cosine of their renormalised
    # exposure vectors; it is a sum over the factors, so label switching does not touch it.  include: a logical of G flags (NULL = all);
    # a tumour with FALSE or NA is left out.  query: tumours (1-based indices, or column names of the data) whose similarity to every
    # tumour is returned in full.  list(neighbours (a data frame: tumour, rank, neighbour, mean, sd, p_similar: per included tumour the
    # top_k others with the largest mean cosine; p_similar is the share of samples with cosine >= min_cosine), dense (3 x Q x G: mean,
    # variance, p_similar; NA on the query itself and on left-out tumours) with query, tumours (a data frame: tumour, typicality,
    # nearest_mean, degree, included), neighbour_at (G x top_k, 1-based, NA = none), neighbour (3 x G x top_k), n_used, n_included,
    # n_left_out, top_k, n_query, n_pairs, n_similar_pairs, n_isolated, mean_similarity, least_typical, least_typical_at (1-based; NA if
    # none), min_cosine).
    get_similarity = function(include = NULL, query = NULL, top_k = 10, min_cosine = 0.9, end_iter = self$state$iter,
                              n_samples = min(self$specs$convergence_control$MAP_over, self$state$iter), idx = "MAP_idx") {
      first <- end_iter - n_samples + 1
      if (is.character(idx)) {
        if (idx != "MAP_idx") stop("Parameter `idx` must be 'MAP_idx', NULL or a vector of recorded iterations")
        idx <- self$MAP$idx
      }
      used <- NULL
      if (!is.null(idx)) {
        idx <- idx[idx >= first & idx <= end_iter]
        used <- rep(FALSE, n_samples); used[idx - first + 1] <- TRUE
      }
      K <- self$dims$K; G <- self$dims$G; N <- self$dims$N
      if (!is.null(include)) {
        if (length(include) != G) stop("include must have one flag per tumour (G = ", G, ")")
        include <- as.logical(include); include[is.na(include)] <- FALSE
      }
      names <- colnames(self$data)
      label <- function(g) if (is.null(names)) g else names[g]
      q <- NULL
      if (!is.null(query)) {
        if (is.character(query)) {
          q <- match(query, names)
          if (anyNA(q)) stop("query names no tumour of the data: ", paste(utils::head(query[is.na(q)], 5), collapse = ", "))
        } else q <- as.integer(query)
      }
      r <- .Call("C_bnmf_similarity", self$handle, as.integer(end_iter), as.integer(n_samples), used, include,
                 if (is.null(q)) NULL else as.integer(q - 1L), c(as.integer(top_k), 1L), as.double(min_cosine), c(K, G, N))
      k <- r$top_k
      at <- if (k > 0) t(r$neighbour_at) else matrix(integer(0), G, 0)            # G x k, 0-based, -1 = none
      nb <- if (k > 0) aperm(array(r$neighbour, c(k, G, 3)), c(3, 2, 1)) else array(numeric(0), c(3, G, 0))
      rows <- which(t(at) >= 0, arr.ind = TRUE)                                   # (rank, tumour), the ranks of a tumour together
      neighbours <- data.frame(tumour = label(rows[, 2]), rank = rows[, 1], neighbour = label(at[rows[, 2:1, drop = FALSE]] + 1L),
                               mean = matrix(nb[1, , ], G, k)[rows[, 2:1, drop = FALSE]], sd = sqrt(matrix(nb[2, , ], G, k)[rows[, 2:1, drop = FALSE]]),
                               p_similar = matrix(nb[3, , ], G, k)[rows[, 2:1, drop = FALSE]])
      out <- list(neighbours = neighbours, neighbour_at = ifelse(at < 0, NA_integer_, at + 1L), neighbour = nb, tumour = t(r$tumour),
                  tumours = data.frame(tumour = label(seq_len(G)), typicality = r$tumour[, 1], nearest_mean = r$tumour[, 2], degree = r$tumour[, 3],
                                       included = if (is.null(include)) rep(TRUE, G) else include),
                  n_used = r$n_used, n_included = r$n_included, n_left_out = r$n_left_out, top_k = k, n_query = r$n_query, n_pairs = r$n_pairs,
                  n_similar_pairs = r$n_similar_pairs, n_isolated = r$n_isolated, mean_similarity = r$mean_similarity,
                  least_typical = r$least_typical, least_typical_at = if (r$least_typical_at < 0) NA_integer_ else as.integer(r$least_typical_at) + 1L,
                  min_cosine = r$min_cosine)
      if (!is.null(q)) {
        out$dense <- aperm(array(r$dense, c(G, length(q), 3)), c(3, 2, 1))
        out$query <- label(q)
      }
      message(sprintf("Similarity: %d tumours included, %d left out; %g of %g pairs similar (cosine >= %g in at least half of the samples), %g tumours resemble nobody; mean similarity %.3g",
                      r$n_included, r$n_left_out, r$n_similar_pairs, r$n_pairs, r$min_cosine, r$n_isolated, r$mean_similarity))
      out
    },
    # Subtypes of the tumours, on the device (bnmf_subtypes_at; not in the reference): does the cohort fall into subtypes, and how certain
    # is the grouping?  Over iterations end_iter - n_samples + 1 ... end_iter (defaults as get_WAIC), restricted to idx, every sample's
    # share profiles are clustered by at most n_steps Lloyd steps from one common start, so subtype c means the same in every sample; a
    # tumour's membership of c is the share of samples in which it carries label c.  With relabel the range is first aligned by
    # get_relabelling() and its perm is handed on; an unmatched sample is left out.  The start: centres (N x C share profiles), or seeds
    # (C tumours, 1-based indices or column names: their share profiles in the MAP exposures), or n_subtypes alone: seeds chosen by a
    # deterministic farthest-first walk over those profiles (the first is nearest the mean profile, each next is farthest from its
    # nearest chosen seed, the lower tumour wins a tie).  include and query as in get_similarity.  list(tumours (a data frame: tumour,
    # label (1-based, NA = none), certainty, runner_up, assigned, included), membership (C x G), subtypes (a data frame: subtype, size,
    # size_sd, size_lower, size_upper), centre (4 x N x C: mean, variance, lower, upper at 0.95), consensus (Q x G, with query), series
    # (3 x S: inertia, steps, assigned tumours), labels (S x G, 1-based, 0 = unassigned, NA = left out or unmatched; with labels = TRUE),
    # centres0, seeds and the info fields).
    get_subtypes = function(n_subtypes = NULL, centres = NULL, seeds = NULL, include = NULL, query = NULL, relabel = TRUE, n_steps = 50,
                            min_certainty = 0.9, end_iter = self$state$iter,
                            n_samples = min(self$specs$convergence_control$MAP_over, self$state$iter), idx = "MAP_idx", labels = FALSE) {
      first <- end_iter - n_samples + 1
      idx0 <- idx
      if (is.character(idx)) {
        if (idx != "MAP_idx") stop("Parameter `idx` must be 'MAP_idx', NULL or a vector of recorded iterations")
        idx <- self$MAP$idx
      }
      used <- NULL
      if (!is.null(idx)) {
        idx <- idx[idx >= first & idx <= end_iter]
        used <- rep(FALSE, n_samples); used[idx - first + 1] <- TRUE
      }
      K <- self$dims$K; G <- self$dims$G; N <- self$dims$N
      if (!is.null(include)) {
        if (length(include) != G) stop("include must have one flag per tumour (G = ", G, ")")
        include <- as.logical(include); include[is.na(include)] <- FALSE
      }
      member <- if (is.null(include)) rep(TRUE, G) else include
      names <- colnames(self$data)
      label <- function(g) if (is.null(names)) g else names[g]
      tumours <- function(v, what) {
        if (is.character(v)) {
          at <- match(v, names)
          if (anyNA(at)) stop(what, " names no tumour of the data: ", paste(utils::head(v[is.na(at)], 5), collapse = ", "))
          at
        } else as.integer(v)
      }
      q <- if (is.null(query)) NULL else tumours(query, "query")
      perm <- NULL
      if (relabel) {
        pm <- self$get_relabelling(end_iter = end_iter, n_samples = n_samples, idx = if (is.null(idx0)) NULL else idx0)$perm
        pm <- t(matrix(as.integer(pm), nrow = N))                       # get_relabelling's is N x S: here S x N, 1-based labels, NA = unmatched
        perm <- matrix(-1L, n_samples, N)
        perm[if (is.null(used)) seq_len(n_samples) else which(used), ] <- ifelse(is.na(pm), -1L, pm - 1L)
      }
      seed_at <- NULL
      if (!is.null(centres)) {
        c0 <- as.matrix(centres)
        if (nrow(c0) != N) stop("centres must have N = ", N, " rows")
      } else {
        if (is.null(seeds) && is.null(n_subtypes)) stop("get_subtypes needs one of n_subtypes, centres and seeds")
        E <- matrix(0, N, G); E[self$MAP$keep_sigs, ] <- self$MAP$E
        prof <- sweep(E, 2, pmax(colSums(E), .Machine$double.xmin), "/")
        if (!is.null(seeds)) seed_at <- tumours(seeds, "seeds") else {
          d <- colSums((prof - rowMeans(prof[, member, drop = FALSE]))^2); d[!member] <- Inf
          seed_at <- which.min(d)                                       # (which.min and which.max return the first of equals)
          near <- colSums((prof - prof[, seed_at])^2)
          while (length(seed_at) < n_subtypes) {
            g <- which.max(ifelse(member, near, -Inf)); seed_at <- c(seed_at, g)
            near <- pmin(near, colSums((prof - prof[, g])^2))
          }
        }
        if (any(!member[seed_at])) stop("a seed is a tumour that include leaves out")
        c0 <- prof[, seed_at, drop = FALSE]
      }
      C <- ncol(c0)
      r <- .Call("C_bnmf_subtypes", self$handle, as.integer(end_iter), as.integer(n_samples), used, include, perm, matrix(as.double(c0), N, C),
                 if (is.null(q)) NULL else as.integer(q - 1L), as.double(c(n_steps, min_certainty, if (labels) 1 else 0, K, G, N)))
      lab <- ifelse(r$label < 0, NA_integer_, r$label + 1L)
      out <- r[c("n_used", "n_matched", "n_unmatched", "n_included", "n_left_out", "C", "n_steps", "n_query", "n_not_converged", "n_certain",
                 "n_never_assigned", "mean_certainty", "least_certain", "smallest_subtype", "min_certainty")]
      out$least_certain_at <- if (r$least_certain_at < 0) NA_integer_ else as.integer(r$least_certain_at) + 1L
      out$smallest_subtype_at <- r$smallest_subtype_at + 1L
      out$tumours <- data.frame(tumour = label(seq_len(G)), label = lab, certainty = r$tumour[, 1], runner_up = r$tumour[, 3], assigned = r$tumour[, 2],
                                included = member)
      out$membership <- t(r$membership)
      out$subtypes <- data.frame(subtype = seq_len(C), size = r$size[, 1], size_sd = sqrt(r$size[, 2]), size_lower = r$size[, 3], size_upper = r$size[, 4])
      out$centre <- aperm(array(r$centre, c(N, C, 4)), c(3, 1, 2))
      out$series <- t(r$series)
      out$centres0 <- c0
      out$seeds <- if (is.null(seed_at)) NULL else label(seed_at)
      if (!is.null(q)) { out$consensus <- t(r$together); out$query <- label(q) }
      if (labels) out$labels <- t(ifelse(r$labels == -2L, NA_integer_, r$labels + 1L))
      message(sprintf("Subtypes: %d subtypes of %d tumours over %d samples (%d unmatched, %d not converged in %d steps); %d tumours with certainty >= %g, mean certainty %.3g",
                      C, r$n_included, r$n_matched, r$n_unmatched, r$n_not_converged, r$n_steps, r$n_certain, r$min_certainty, r$mean_certainty))
      out
    },
    # Residual structure, on the device (bnmf_residuals_at; not in the reference): what does the model leave unexplained, and is there a
    # process in the leftovers?  Over iterations end_iter - n_samples + 1 ... end_iter (defaults as get_WAIC), restricted to idx, every
    # sample gives the standardised residuals of every cell, their second-moment matrix over the included tumours along the mutation
    # types, its leading component (n_steps power steps) and every tumour's score on it.  A direction that the misfits of many tumours
    # share is what a missing signature looks like: a rank that is too low.  include as in get_similarity.  max_dispersion = 2.0 is a
    # reporting convention like min_cosine = 0.9 (it only sets the count n_overdispersed), not a test.  list(types (a data frame: type,
    # bias, bias_sd, p_positive, dispersion, dispersion_sd, component, component_mean, component_sd), tumours (a data frame: tumour, score,
    # score_sd, chi, included), candidate (K: the positive part of the mean matrix's component, or of its negative where that part has
    # the larger sum of squares, normalised to sum 1), candidate_cosine (with the columns of the MAP signatures), with reference_P (K x R)
    # reference_cosine, best_reference and best_reference_cosine, gram (K x K), series (5 x S: trace, lambda, share, move, agreement) and
    # the info fields).
    get_residuals = function(include = NULL, n_steps = 100, max_dispersion = 2.0, reference_P = NULL, end_iter = self$state$iter,
                             n_samples = min(self$specs$convergence_control$MAP_over, self$state$iter), idx = "MAP_idx") {
      first <- end_iter - n_samples + 1
      if (is.character(idx)) {
        if (idx != "MAP_idx") stop("Parameter `idx` must be 'MAP_idx', NULL or a vector of recorded iterations")
        idx <- self$MAP$idx
      }
      used <- NULL
      if (!is.null(idx)) {
        idx <- idx[idx >= first & idx <= end_iter]
        used <- rep(FALSE, n_samples); used[idx - first + 1] <- TRUE
      }
      K <- self$dims$K; G <- self$dims$G
      if (!is.null(include)) {
        if (length(include) != G) stop("include must have one flag per tumour (G = ", G, ")")
        include <- as.logical(include); include[is.na(include)] <- FALSE
      }
      member <- if (is.null(include)) rep(TRUE, G) else include
      names <- colnames(self$data)
      r <- .Call("C_bnmf_residuals", self$handle, as.integer(end_iter), as.integer(n_samples), used, include, as.double(c(n_steps, max_dispersion, K, G)))
      out <- r[c("n_used", "n_flat", "n_included", "n_left_out", "n_steps", "n_biased", "n_overdispersed", "lambda", "share", "move", "mean_share",
                 "min_agreement", "worst_type", "max_dispersion")]
      out$worst_type_at <- r$worst_type_at + 1L
      out$min_agreement_at <- if (r$min_agreement_at < 0) NA_integer_ else r$min_agreement_at + 1L
      vbar <- r$component[, 1]
      pos <- pmax(vbar, 0); neg <- pmax(-vbar, 0)
      part <- if (isTRUE(sum(neg^2) > sum(pos^2))) neg else pos
      cand <- if (isTRUE(sum(part) > 0) && is.finite(sum(part))) part / sum(part) else rep(NA_real_, K)
      cosines <- function(cols) as.numeric(crossprod(cols, cand)) / sqrt(colSums(cols^2) * sum(cand^2))
      out$candidate <- cand
      out$candidate_cosine <- cosines(as.matrix(self$MAP$P))
      if (!is.null(reference_P)) {
        ref <- as.matrix(reference_P)
        if (nrow(ref) != K) stop("reference_P must have K = ", K, " rows")
        rc <- cosines(ref)
        out$reference_cosine <- rc
        best <- if (all(is.na(rc))) NA_integer_ else which.max(rc)
        out$best_reference <- if (is.na(best)) NA else if (is.null(colnames(ref))) best else colnames(ref)[best]
        out$best_reference_cosine <- if (is.na(best)) NA_real_ else rc[best]
      }
      out$types <- data.frame(type = seq_len(K), bias = r$type[, 1], bias_sd = sqrt(r$type[, 2]), p_positive = r$type[, 3], dispersion = r$type[, 4],
                              dispersion_sd = sqrt(r$type[, 5]), component = vbar, component_mean = r$component[, 2], component_sd = sqrt(r$component[, 3]))
      out$tumours <- data.frame(tumour = if (is.null(names)) seq_len(G) else names, score = r$tumour[, 1], score_sd = sqrt(r$tumour[, 2]), chi = r$tumour[, 3],
                                included = member)
      out$gram <- r$gram
      out$series <- t(r$series)
      message(sprintf("Residuals: %d tumours over %d samples (%d flat); the leading component carries %.3g of the mean matrix's trace; %d types with dispersion > %g, %d biased",
                      r$n_included, r$n_used - r$n_flat, r$n_flat, r$share, r$n_overdispersed, r$max_dispersion, r$n_biased))
      out
    },
    # Trade-offs between signatures within a tumour, on the device (bnmf_tradeoff_at; not in the reference): which signatures exchange
    # mutations from sample to sample in one tumour, and how uncertain is a SUM of exposures?  Over iterations end_iter - n_samples + 1
    # ... end_iter (defaults as get_WAIC), restricted to idx, per tumour the N x N covariance of its renormalised exposures over the
    # samples and the correlations.  With relabel the range is first aligned by get_relabelling() and its perm is handed on; an unmatched
    # sample is left out.  sets: an integer label per signature (1-based, NA = in no set) or a named list of 1-based signature indices;
    # query: tumours (1-based indices or column names) whose whole matrices are wanted; include as in get_similarity.  min_corr = 0.5 is a
    # reporting convention like min_cosine = 0.9, not a test.  list(tumours (a data frame: tumour, min_corr, pair_j, pair_l (1-based, NA =
    # none), n_defined, total_ratio, included), pair (a list of N x N symmetric matrices with an NA diagonal: mean_corr, n_defined,
    # p_negative, p_positive, mean_cov), sets (a data frame: set, tumour, mean, sd_sum, sd_if_independent, ratio; with sets), dense (N x N
    # x 2 x Q: covariance, correlation; with query) and the info fields).
    get_tradeoff = function(sets = NULL, query = NULL, include = NULL, relabel = TRUE, min_corr = 0.5, end_iter = self$state$iter,
                            n_samples = min(self$specs$convergence_control$MAP_over, self$state$iter), idx = "MAP_idx") {
      first <- end_iter - n_samples + 1
      idx0 <- idx
      if (is.character(idx)) {
        if (idx != "MAP_idx") stop("Parameter `idx` must be 'MAP_idx', NULL or a vector of recorded iterations")
        idx <- self$MAP$idx
      }
      used <- NULL
      if (!is.null(idx)) {
        idx <- idx[idx >= first & idx <= end_iter]
        used <- rep(FALSE, n_samples); used[idx - first + 1] <- TRUE
      }
      G <- self$dims$G; N <- self$dims$N
      if (!is.null(include)) {
        if (length(include) != G) stop("include must have one flag per tumour (G = ", G, ")")
        include <- as.logical(include); include[is.na(include)] <- FALSE
      }
      member <- if (is.null(include)) rep(TRUE, G) else include
      names <- colnames(self$data)
      label <- function(g) if (is.null(names)) g else names[g]
      set_names <- NULL; st <- NULL
      if (is.list(sets)) {
        set_names <- if (is.null(names(sets))) seq_along(sets) else names(sets)
        st <- rep(-1L, N)
        for (c in seq_along(sets)) {
          at <- as.integer(sets[[c]])
          if (length(at) == 0 || any(at < 1 | at > N)) stop("set ", set_names[c], " is empty or names a signature outside 1 .. ", N)
          if (any(st[at] >= 0)) stop("set ", set_names[c], " holds a signature that another set holds")
          st[at] <- c - 1L
        }
      } else if (!is.null(sets)) {
        if (length(sets) != N) stop("sets must have one label per signature (N = ", N, ")")
        st <- ifelse(is.na(sets), -1L, as.integer(sets) - 1L)
        set_names <- seq_len(max(st) + 1L)
      }
      C <- if (is.null(st)) 0L else max(st) + 1L
      q <- NULL
      if (!is.null(query)) {
        q <- if (is.character(query)) match(query, names) else as.integer(query)
        if (anyNA(q)) stop("query names no tumour of the data: ", paste(utils::head(query[is.na(q)], 5), collapse = ", "))
      }
      perm <- NULL
      if (relabel) {
        pm <- self$get_relabelling(end_iter = end_iter, n_samples = n_samples, idx = if (is.null(idx0)) NULL else idx0)$perm
        pm <- t(matrix(as.integer(pm), nrow = N))                       # get_relabelling's is N x S: here S x N, 1-based labels, NA = unmatched
        perm <- matrix(-1L, n_samples, N)
        perm[if (is.null(used)) seq_len(n_samples) else which(used), ] <- ifelse(is.na(pm), -1L, pm - 1L)
      }
      r <- .Call("C_bnmf_tradeoff", self$handle, as.integer(end_iter), as.integer(n_samples), used, include, perm, st,
                 if (is.null(q)) NULL else as.integer(q - 1L), as.double(c(min_corr, C, G, N)))
      out <- r[c("n_used", "n_matched", "n_unmatched", "n_included", "n_left_out", "n_sets", "n_query", "n_traded", "strongest_pair", "mean_ratio", "min_corr")]
      out$strongest_pair_at <- if (r$strongest_pair_at < 0) NA_integer_ else c(r$strongest_pair_at %/% N, r$strongest_pair_at %% N) + 1L
      at <- r$pair_at
      out$tumours <- data.frame(tumour = label(seq_len(G)), min_corr = r$tumour[, 1], pair_j = ifelse(at < 0, NA_integer_, at %/% N + 1L),
                                pair_l = ifelse(at < 0, NA_integer_, at %% N + 1L), n_defined = r$tumour[, 2], total_ratio = r$tumour[, 3], included = member)
      rows <- c("mean_corr", "n_defined", "p_negative", "p_positive", "mean_cov")
      out$pair <- setNames(lapply(seq_along(rows), function(k) matrix(r$pair[, k], N, N)), rows)
      if (C > 0) {
        sst <- array(r$setstat, c(G, C, 4))
        out$sets <- do.call(rbind, lapply(seq_len(C), function(c) data.frame(set = set_names[c], tumour = label(seq_len(G)), mean = sst[, c, 1],
                                                                             sd_sum = sqrt(sst[, c, 2]), sd_if_independent = sqrt(sst[, c, 3]), ratio = sst[, c, 4])))
      }
      if (!is.null(q)) { out$dense <- array(r$dense, c(N, N, 2, length(q))); out$query <- label(q) }
      message(sprintf("Trade-offs: %d tumours over %d samples (%d unmatched); %d tumours with a correlation <= -%g; mean variance ratio of the total %.3g",
                      r$n_included, r$n_matched, r$n_unmatched, r$n_traded, r$min_corr, r$mean_ratio))
      out
    },
    # Cohort summary of the signatures, on the device (bnmf_summary_at; the reference's summary() reports the carriers' median and the
    # prevalence of the MAP point estimate alone): how is a signature's load distributed across the cohort?  Over iterations end_iter -
    # n_samples + 1 ... end_iter (defaults as get_WAIC), restricted to idx, per sample and signature the prevalence (tumours with a load
    # >= min_load), the total load, its fraction of the cohort's, the carriers' mean and at every level of probs the exact type-7 quantile
    # of all loads (load_all_<p>), of the carriers' loads (load_present_<p>) and of the shares (share_all_<p>).  With relabel the range is
    # first aligned by get_relabelling() and its perm is handed on; an unmatched sample is left out.  include: a logical of G flags (NULL =
    # all).  A list with, per statistic name, a data frame (signature, mean, var, lower, upper, n_valid), the info fields, names and
    # probs; with series also series (N x S x NSTAT).
    get_summary = function(probs = c(0.05, 0.25, 0.5, 0.75, 0.95), min_load = 1, include = NULL, relabel = TRUE, credible_interval = 0.95,
                           series = FALSE, end_iter = self$state$iter,
                           n_samples = min(self$specs$convergence_control$MAP_over, self$state$iter), idx = "MAP_idx") {
      first <- end_iter - n_samples + 1
      idx0 <- idx
      if (is.character(idx)) {
        if (idx != "MAP_idx") stop("Parameter `idx` must be 'MAP_idx', NULL or a vector of recorded iterations")
        idx <- self$MAP$idx
      }
      used <- NULL
      if (!is.null(idx)) {
        idx <- idx[idx >= first & idx <= end_iter]
        used <- rep(FALSE, n_samples); used[idx - first + 1] <- TRUE
      }
      G <- self$dims$G; N <- self$dims$N
      if (!is.null(include)) {
        if (length(include) != G) stop("include must have one flag per tumour (G = ", G, ")")
        include <- as.logical(include); include[is.na(include)] <- FALSE
      }
      perm <- NULL
      if (relabel) {
        pm <- self$get_relabelling(end_iter = end_iter, n_samples = n_samples, idx = if (is.null(idx0)) NULL else idx0)$perm
        pm <- t(matrix(as.integer(pm), nrow = N))                       # get_relabelling's is N x S: here S x N, 1-based labels, NA = unmatched
        perm <- matrix(-1L, n_samples, N)
        perm[if (is.null(used)) seq_len(n_samples) else which(used), ] <- ifelse(is.na(pm), -1L, pm - 1L)
      }
      ci <- if (is.null(credible_interval)) 0 else credible_interval
      r <- .Call("C_bnmf_summary", self$handle, as.integer(end_iter), as.integer(n_samples), used, include, perm, as.double(probs),
                 as.double(c(min_load, ci, if (series) 1 else 0, G, N)))
      L <- length(probs)
      nms <- c("prevalence", "total", "fraction", "mean_present",
               as.vector(sapply(c("load_all", "load_present", "share_all"), function(f) paste0(f, "_", format(probs, trim = TRUE)))))
      out <- r[c("n_used", "n_aligned", "n_included", "n_left_out", "n_levels", "n_blocks", "n_nonfinite", "min_load", "credible_interval")]
      out$names <- nms; out$probs <- probs
      for (q in seq_along(nms)) {
        at <- 5L * (q - 1L)
        out[[nms[q]]] <- data.frame(signature = seq_len(N), mean = r$stat[, at + 1L], var = r$stat[, at + 2L], lower = r$stat[, at + 3L],
                                    upper = r$stat[, at + 4L], n_valid = r$stat[, at + 5L])
      }
      if (series) out$series <- array(r$series, c(N, r$n_used, length(nms)))
      message(sprintf("Summary: %d tumours over %d of %d samples, %d levels, min_load %g", r$n_included, r$n_aligned, r$n_used, L, r$min_load))
      out
    },
    # Sparse per-tumour assignment with refit, on the device (bnmf_prune_at; not in the reference): which signatures does each tumour keep,
    # and how large are they once the others are gone?  Over iterations end_iter - n_samples + 1 ... end_iter (defaults as get_WAIC),
    # restricted to idx, per sample and tumour backward elimination of the sample's signatures with a refit of the remaining exposures
    # after every removal (n_steps KL steps), while the cosine of the fit stays within max_loss of the full refit's: the refit that
    # get_reconstruction's drop leaves out.  max_loss = 0.01 and n_steps = 20 are reporting conventions like min_cosine = 0.9, not tests;
    # rel_change tells whether n_steps sufficed.  include: a logical of G flags (NULL = all).  list(assignment (a data frame: tumour,
    # signature (1-based), load, p_kept for every pair with p_kept >= 0.5), tumours (a data frame), load (a list of N x G matrices:
    # load_mean, load_var, share, p_kept), series (S x 2), signature (N x 3), exposures (N x G x S, with exposures = TRUE) and the info
    # fields).  NA for an all-zero or left-out tumour.
    get_sparse_assignment = function(max_loss = 0.01, n_steps = 20L, include = NULL, end_iter = self$state$iter,
                                     n_samples = min(self$specs$convergence_control$MAP_over, self$state$iter), exposures = FALSE, idx = "MAP_idx") {
      first <- end_iter - n_samples + 1
      if (is.character(idx)) {
        if (idx != "MAP_idx") stop("Parameter `idx` must be 'MAP_idx', NULL or a vector of recorded iterations")
        idx <- self$MAP$idx
      }
      used <- NULL
      if (!is.null(idx)) {
        idx <- idx[idx >= first & idx <= end_iter]
        used <- rep(FALSE, n_samples); used[idx - first + 1] <- TRUE
      }
      G <- self$dims$G; N <- self$dims$N
      if (!is.finite(max_loss)) stop("max_loss must be a finite number")
      if (n_steps < 1 || n_steps != as.integer(n_steps)) stop("n_steps must be a whole number >= 1")
      if (!is.null(include)) {
        if (length(include) != G) stop("include must have one flag per tumour (G = ", G, ")")
        include <- as.logical(include); include[is.na(include)] <- FALSE
      }
      member <- if (is.null(include)) rep(TRUE, G) else include
      names <- colnames(self$data)
      label <- function(g) if (is.null(names)) g else names[g]
      r <- .Call("C_bnmf_prune", self$handle, as.integer(end_iter), as.integer(n_samples), used, include,
                 as.double(c(n_steps, max_loss, if (exposures) 1 else 0, G, N)))
      out <- r[c("n_used", "n_included", "n_undefined", "n_single", "n_steps", "trials", "max_change", "max_loss", "series", "signature")]
      rows <- c("load_mean", "load_var", "share", "p_kept")
      out$load <- setNames(lapply(seq_along(rows), function(k) matrix(r$load[, k], N, G)), rows)
      kept <- which(!is.na(out$load$p_kept) & out$load$p_kept >= 0.5, arr.ind = TRUE)
      kept <- kept[order(kept[, 2], kept[, 1]), , drop = FALSE]
      out$assignment <- data.frame(tumour = label(kept[, 2]), signature = kept[, 1], load = out$load$load_mean[kept], p_kept = out$load$p_kept[kept])
      out$tumours <- data.frame(tumour = label(seq_len(G)), cos_0 = r$tumour[, 1], cos_f = r$tumour[, 2], n_kept = r$tumour[, 3], n_kept_min = r$tumour[, 4],
                                n_kept_max = r$tumour[, 5], rel_change = r$tumour[, 6], mean_trials = r$tumour[, 7], included = member)
      if (exposures) out$exposures <- array(r$exposures, c(N, G, r$n_used))
      message(sprintf("Sparse assignment: %d tumours (%d all-zero) over %d samples, max_loss %g, %d steps; %d pairs kept with p >= 0.5; largest last-step change %.3g",
                      r$n_included, r$n_undefined, r$n_used, r$max_loss, r$n_steps, nrow(out$assignment), r$max_change))
      out
    },
    # Co-activity of the signatures, on the device (bnmf_coactivity_at; not in the reference): do two signatures act in the same tumours
    # or exclude each other, and is a signature split into two factors (a high cosine of two columns of P whose exposures are
    # negatively correlated)?  Over iterations end_iter - n_samples + 1 ... end_iter (defaults as get_WAIC), restricted to idx, every
    # sample gives per pair of signatures the Pearson and the Spearman (midrank) correlation of their loads across the included tumours,
    # the phi coefficient of their presence (load >= min_load) and the cosine of their two columns of P.  include: a logical of G flags
    # (NULL = all); a tumour with FALSE or NA is left out.  list(pearson, spearman, copresence, cosine (each a list of N x N symmetric
    # matrices with an NA diagonal: mean, lower, upper, p_greater, n_valid, over the samples whose value is not NaN; quantile type 7),
    # pairs (NP x 2, 1-based), pair (NP x 7 x 4: every row of the call), include, n_used, n_included, n_left_out, n_pairs, n_blocks,
    # n_credible (pearson, spearman, copresence: the pairs whose interval excludes 0), max_cosine, max_cosine_at (1-based; NA if none),
    # min_load, credible_interval), with series also series (NP x S x 4).  No multiple-testing adjustment.
    get_coactivity = function(include = NULL, min_load = 1, credible_interval = 0.95, series = FALSE, end_iter = self$state$iter,
                              n_samples = min(self$specs$convergence_control$MAP_over, self$state$iter), idx = "MAP_idx") {
      first <- end_iter - n_samples + 1
      if (is.character(idx)) {
        if (idx != "MAP_idx") stop("Parameter `idx` must be 'MAP_idx', NULL or a vector of recorded iterations")
        idx <- self$MAP$idx
      }
      used <- NULL
      if (!is.null(idx)) {
        idx <- idx[idx >= first & idx <= end_iter]
        used <- rep(FALSE, n_samples); used[idx - first + 1] <- TRUE
      }
      K <- self$dims$K; G <- self$dims$G; N <- self$dims$N
      if (!is.null(include)) {
        if (length(include) != G) stop("include must have one flag per tumour (G = ", G, ")")
        include <- as.logical(include); include[is.na(include)] <- FALSE
      }
      r <- .Call("C_bnmf_coactivity", self$handle, as.integer(end_iter), as.integer(n_samples), used, include, as.double(min_load),
                 as.double(credible_interval), as.logical(series), c(K, G, N))
      pairs <- t(utils::combn(N, 2))
      stat <- function(q) {
        rows <- c(mean = 1, lower = 3, upper = 4, p_greater = 5, n_valid = 7)
        o <- list()
        for (nm in names(rows)) {
          m <- matrix(NA_real_, N, N)
          m[pairs] <- r$pair[, 7 * q + rows[[nm]]]; m[pairs[, 2:1, drop = FALSE]] <- r$pair[, 7 * q + rows[[nm]]]
          o[[nm]] <- m
        }
        o
      }
      out <- list(pearson = stat(0), spearman = stat(1), copresence = stat(2), cosine = stat(3), pairs = pairs,
                  pair = array(r$pair, c(nrow(pairs), 7, 4)), include = include, n_used = r$n_used, n_included = r$n_included,
                  n_left_out = r$n_left_out, n_pairs = r$n_pairs, n_blocks = r$n_blocks,
                  n_credible = stats::setNames(r$n_credible, c("pearson", "spearman", "copresence")), max_cosine = r$max_cosine,
                  max_cosine_at = if (r$max_cosine_at < 0) NA_integer_ else r$max_cosine_at + 1L, min_load = r$min_load,
                  credible_interval = r$credible_interval)
      if (series) out$series <- array(r$series, c(nrow(pairs), r$n_used, 4))
      message(sprintf("Co-activity: %d tumours included, %d left out; %d pairs, n_credible pearson %g, spearman %g, copresence %g; largest mean cosine %.3g",
                      r$n_included, r$n_left_out, r$n_pairs, r$n_credible[1], r$n_credible[2], r$n_credible[3], r$max_cosine))
      out
    },
    # Silhouette stability of the recorded signatures, on the device (bnmf_stability_at; not in the reference): over iterations
    # end_iter - n_samples + 1 ... end_iter (defaults as get_WAIC), restricted to idx, every recorded column of P is a point, the
    # distance is the cosine distance and the cluster of a point is its factor - with relabel the label get_relabelling() gave it, an
    # unmatched sample being left out.  extra_P (K x X) with extra_label (1-based) adds further columns.  list(stability, min_silhouette,
    # members, mean_a, mean_b, share_negative (length N), silhouette, a, b, nearest (S x N; nearest 1-based, NA = none), between (N x
    # N), medoid (K x N consensus signatures), medoid_at (1-based points, NA = empty), n_used, n_points, n_extra, n_left_out,
    # n_clusters, n_negative, mean_silhouette, min_stability, min_stability_at (1-based; NA if none)).
    get_stability = function(end_iter = self$state$iter, n_samples = min(self$specs$convergence_control$MAP_over, self$state$iter),
                             relabel = TRUE, extra_P = NULL, extra_label = NULL, idx = "MAP_idx") {
      first <- end_iter - n_samples + 1
      if (is.character(idx)) {
        if (idx != "MAP_idx") stop("Parameter `idx` must be 'MAP_idx', NULL or a vector of recorded iterations")
        idx <- self$MAP$idx
      }
      used <- NULL
      if (!is.null(idx)) {
        idx <- idx[idx >= first & idx <= end_iter]
        used <- rep(FALSE, n_samples); used[idx - first + 1] <- TRUE
      }
      K <- self$dims$K; G <- self$dims$G; N <- self$dims$N
      labels <- NULL
      if (relabel) {
        perm <- self$get_relabelling(end_iter = end_iter, n_samples = n_samples, idx = if (is.null(idx)) NULL else idx)$perm
        perm <- t(matrix(as.integer(perm), nrow = N))                 # get_relabelling's is N x S: here S x N, 1-based labels, NA = unmatched
        labels <- matrix(-1L, n_samples, N)
        labels[if (is.null(used)) seq_len(n_samples) else which(used), ] <- ifelse(is.na(perm), -1L, perm - 1L)
      }
      if (!is.null(extra_P)) {
        extra_P <- matrix(as.double(extra_P), nrow = K)
        extra_label <- as.integer(extra_label) - 1L
      }
      r <- .Call("C_bnmf_stability", self$handle, as.integer(end_iter), as.integer(n_samples), used, labels, extra_P, extra_label, c(K, G, N))
      S <- r$n_used
      ring <- function(j) matrix(r$point[seq_len(S * N), j], S, N, byrow = TRUE)
      one <- function(v) ifelse(v < 0, NA_integer_, as.integer(v) + 1L)
      out <- list(members = r$factor[, 1], stability = r$factor[, 2], min_silhouette = r$factor[, 3], mean_a = r$factor[, 4], mean_b = r$factor[, 5],
                  share_negative = r$factor[, 6], silhouette = ring(1), a = ring(2), b = ring(3), nearest = matrix(one(ring(4)), S, N),
                  between = t(r$between), medoid = r$medoid, medoid_at = one(r$medoid_at), n_used = r$n_used, n_points = r$n_points,
                  n_extra = r$n_extra, n_left_out = r$n_left_out, n_clusters = r$n_clusters, n_negative = r$n_negative,
                  mean_silhouette = r$mean_silhouette, min_stability = r$min_stability, min_stability_at = one(r$min_stability_at))
      message(sprintf("Stability: %d points in %d clusters, %d left out; mean silhouette %.3g, least stable signature %s at %.3g", r$n_points,
                      r$n_clusters, r$n_left_out, r$mean_silhouette, format(out$min_stability_at), r$min_stability))
      out
    },
    # Exposures of new tumours under the recorded signatures, on the device (bnmf_project_at; not in the reference): new_data is a
    # K x J matrix of counts (or other non-negative values) of tumours the chain has not seen.  Over iterations end_iter - n_samples + 1
    # ... end_iter (defaults as get_WAIC), restricted to idx, every column is refitted to every sample's renormalised signatures by
    # n_steps steps of the KL multiplicative update, so the uncertainty of the signatures reaches the exposures.  list(exposure_mean,
    # exposure_sd, share, p_present, lower, upper (N x J: moments over the samples, the mean share of the tumour, the fraction of samples
    # with at least min_load mutations, the credible_interval bounds, quantile type 7, computed here from the per-sample exposures), fit
    # (a data frame with one row per new tumour: cosine, rel_l1, max_rel_change), n_used, n_steps, n_present, total, max_rel_change,
    # min_cosine, min_cosine_at (1-based; NA if none)).  n_steps = 200 is a convention: max_rel_change says how far the refit still moved.
    get_projection = function(new_data, end_iter = self$state$iter, n_samples = min(self$specs$convergence_control$MAP_over, self$state$iter),
                              idx = "MAP_idx", n_steps = 200, min_load = 1, credible_interval = 0.95) {
      first <- end_iter - n_samples + 1
      if (is.character(idx)) {
        if (idx != "MAP_idx") stop("Parameter `idx` must be 'MAP_idx', NULL or a vector of recorded iterations")
        idx <- self$MAP$idx
      }
      used <- NULL
      if (!is.null(idx)) {
        idx <- idx[idx >= first & idx <= end_iter]
        used <- rep(FALSE, n_samples); used[idx - first + 1] <- TRUE
      }
      K <- self$dims$K; G <- self$dims$G; N <- self$dims$N
      X <- as.matrix(new_data)
      if (nrow(X) != K) stop("new_data must have K = ", K, " rows")
      storage.mode(X) <- "double"
      J <- ncol(X)
      r <- .Call("C_bnmf_project", self$handle, as.integer(end_iter), as.integer(n_samples), used, X, as.integer(n_steps),
                 as.double(min_load), TRUE, c(K, G, N))
      a <- (1 - credible_interval) / 2
      q <- apply(r$exposures, 1, quantile, probs = c(a, 1 - a), type = 7, names = FALSE)
      fit <- data.frame(cosine = r$fit[, 1], rel_l1 = r$fit[, 2], max_rel_change = r$fit[, 3])
      message(sprintf("Projection: J = %d, %d steps, max_rel_change %.3g, min_cosine %.4f", J, r$n_steps, r$max_rel_change, r$min_cosine))
      list(exposure_mean = matrix(r$load[, 1], N, J), exposure_sd = sqrt(matrix(r$load[, 2], N, J)), share = matrix(r$load[, 3], N, J),
           p_present = matrix(r$load[, 4], N, J), lower = matrix(q[1, ], N, J), upper = matrix(q[2, ], N, J), fit = fit,
           n_used = r$n_used, n_steps = r$n_steps, n_present = r$n_present, total = r$total, max_rel_change = r$max_rel_change,
           min_cosine = r$min_cosine, min_cosine_at = if (r$min_cosine_at < 0) NA_integer_ else as.integer(r$min_cosine_at) + 1L)
    },
    # Is a discovered signature a mixture of known ones?  On the device (bnmf_decompose_at; not in the reference): reference_P is a K x R
    # catalogue (its column names name the references).  Over iterations end_iter - n_samples + 1 ... end_iter (defaults as get_WAIC),
    # restricted to idx (the default keeps the samples of one rank pattern: a sample that excludes a factor enters its means with 0), every
    # renormalised column of every sample's P is refitted to the normalised catalogue by n_steps steps of the KL multiplicative update,
    # the references below min_share of the column are dropped and n_steps more steps refit the rest, so the uncertainty of the
    # signatures reaches the mixture weights.  keep: the factors to decompose (logical length N, NULL = all).  list(weight_mean, weight_sd,
    # share, p_present, lower, upper (R x N: moments over the samples, the mean share of the signature, the fraction of samples with a
    # weight of at least min_share, the credible_interval bounds, quantile type 7, computed here from the per-sample weights), fit (a data
    # frame with one row per signature: cosine, rel_l1, max_rel_change), nactive (N x S), included (N), components (per signature a data
    # frame of the references with p_present >= 0.5, the largest mean weight first), n_used, n_steps, R, n_present, min_share,
    # max_rel_change, min_cosine, min_cosine_at (1-based; NA if none)).
    get_decomposition = function(reference_P, end_iter = self$state$iter,
                                 n_samples = min(self$specs$convergence_control$MAP_over, self$state$iter), idx = "MAP_idx", n_steps = 200,
                                 min_share = 0.05, keep = NULL, credible_interval = 0.95, reference_names = colnames(reference_P)) {
      first <- end_iter - n_samples + 1
      if (is.character(idx)) {
        if (idx != "MAP_idx") stop("Parameter `idx` must be 'MAP_idx', NULL or a vector of recorded iterations")
        idx <- self$MAP$idx
      }
      used <- NULL
      if (!is.null(idx)) {
        idx <- idx[idx >= first & idx <= end_iter]
        used <- rep(FALSE, n_samples); used[idx - first + 1] <- TRUE
      }
      K <- self$dims$K; G <- self$dims$G; N <- self$dims$N
      ref <- as.matrix(reference_P)
      if (nrow(ref) != K) stop("reference_P must have K = ", K, " rows")
      storage.mode(ref) <- "double"
      R <- ncol(ref)
      if (is.null(reference_names)) reference_names <- seq_len(R)
      if (length(reference_names) != R) stop("reference_names must have one entry per column of reference_P")
      if (!is.null(keep)) keep <- as.logical(keep)
      r <- .Call("C_bnmf_decompose", self$handle, as.integer(end_iter), as.integer(n_samples), used, ref, keep, as.double(min_share),
                 c(as.integer(n_steps), 1L), c(K, G, N))
      a <- (1 - credible_interval) / 2
      q <- apply(r$weights, 1, quantile, probs = c(a, 1 - a), type = 7, names = FALSE)
      fit <- data.frame(cosine = r$fit[, 1], rel_l1 = r$fit[, 2], max_rel_change = r$fit[, 3])
      wm <- matrix(r$weight[, 1], R, N); pp <- matrix(r$weight[, 4], R, N)
      components <- lapply(seq_len(N), function(n) {
        i <- order(-wm[, n]); i <- i[pp[i, n] >= 0.5]
        data.frame(reference = reference_names[i], p_present = pp[i, n], weight_mean = wm[i, n])
      })
      message(sprintf("Decomposition: R = %d, %d steps, min_share %g, min_cosine %.4f, max_rel_change %.3g", R, r$n_steps, r$min_share,
                      r$min_cosine, r$max_rel_change))
      list(weight_mean = wm, weight_sd = sqrt(matrix(r$weight[, 2], R, N)), share = matrix(r$weight[, 3], R, N), p_present = pp,
           lower = matrix(q[1, ], R, N), upper = matrix(q[2, ], R, N), fit = fit, nactive = r$nactive, included = r$included,
           components = components, n_used = r$n_used, n_steps = r$n_steps, R = r$R, n_present = r$n_present, min_share = r$min_share,
           max_rel_change = r$max_rel_change, min_cosine = r$min_cosine,
           min_cosine_at = if (r$min_cosine_at < 0) NA_integer_ else as.integer(r$min_cosine_at) + 1L)
    },
    # Label-switching correction of the recorded samples, on the device (bnmf_relabel_at; not in the reference): over iterations
    # end_iter - n_samples + 1 ... end_iter (defaults as get_WAIC), restricted to idx, every sample's factors are permuted to the labels
    # of a pivot so that the total cosine is largest, and the pivot is iterated to the aligned mean (at most max_rounds rounds).
    # pivot: "MAP" (the MAP's P, the factors it dropped put back from the last sample), "last" (the newest used sample's P) or a K x N
    # matrix.  list(perm (N x S: the label of every factor per used sample, NA = no assignment), cosine (N x S), confusion (N x N),
    # P_mean, P_var (K x N), E_mean, E_var (N x G) over all N factors, P and E: the aligned means of the MAP's kept factors, n_used,
    # n_aligned, n_unmatched, rounds, converged, n_switched, n_changed_last, mean_cosine, min_cosine, min_cosine_at), with aligned also
    # aligned_P (K x N x S) and aligned_E (N x G x S)
    get_relabelling = function(end_iter = self$state$iter, n_samples = min(self$specs$convergence_control$MAP_over, self$state$iter),
                               idx = "MAP_idx", pivot = "MAP", max_rounds = 10, aligned = FALSE) {
      first <- end_iter - n_samples + 1
      if (is.character(idx)) {
        if (idx != "MAP_idx") stop("Parameter `idx` must be 'MAP_idx', NULL or a vector of recorded iterations")
        idx <- self$MAP$idx
      }
      used <- NULL
      if (!is.null(idx)) {
        idx <- idx[idx >= first & idx <= end_iter]
        used <- rep(FALSE, n_samples); used[idx - first + 1] <- TRUE
      }
      K <- self$dims$K; G <- self$dims$G; N <- self$dims$N
      ks <- if (is.null(self$MAP$keep_sigs)) seq_len(N) else self$MAP$keep_sigs
      if (is.character(pivot)) {
        if (pivot == "last") piv <- NULL
        else if (pivot == "MAP") {
          piv <- self$params$P
          piv[, ks] <- self$MAP$P
        } else stop("Parameter `pivot` must be 'MAP', 'last' or a K x N matrix")
      } else {
        piv <- as.matrix(pivot)
        if (!all(dim(piv) == c(K, N))) stop("pivot must be a K x N matrix")
      }
      if (!is.null(piv)) storage.mode(piv) <- "double"
      r <- .Call("C_bnmf_relabel", self$handle, as.integer(end_iter), as.integer(n_samples), used, piv, as.integer(max_rounds),
                 as.logical(aligned), c(K, G, N))
      out <- r[c("n_used", "n_aligned", "n_unmatched", "rounds", "converged", "n_switched", "n_changed_last", "mean_cosine", "min_cosine",
                 "min_cosine_at", "perm", "cosine", "confusion")]
      out$P_mean <- matrix(r$P[, 1], K, N); out$P_var <- matrix(r$P[, 2], K, N)
      out$E_mean <- matrix(r$E[, 1], N, G); out$E_var <- matrix(r$E[, 2], N, G)
      out$P <- out$P_mean[, ks, drop = FALSE]; out$E <- out$E_mean[ks, , drop = FALSE]
      if (aligned) { out$aligned_P <- array(r$aligned_P, c(K, N, ncol(r$perm))); out$aligned_E <- array(r$aligned_E, c(N, G, ncol(r$perm))) }
      out
    },
    # the data frame plot_label_switching (R/postprocessing_visualizations.R:598-669) builds before combine_below, on the device
    # (bnmf_label_switching): per recorded iteration in idx ("all": every kept sample) and latent factor, the reference signature
    # hungarian_assignment(keep_all_est = TRUE) gives it ("None": no partner), that cosine, and whether A includes the factor
    label_switching_df = function(reference_P, idx = "all") {
      save_df <- FALSE
      if (is.character(idx)) {
        if (idx != "all") stop("Parameter `idx` must be a vector of indices or 'all'")
        save_df <- TRUE
        W <- if (self$specs$save_all_samples) length(self$temperature_schedule) else self$specs$convergence_control$MAP_over
        idx <- seq(max(1, self$state$iter - W + 1), self$state$iter)
      }
      idx <- sort(as.integer(idx))
      N <- self$dims$N
      r <- .Call("C_bnmf_label_switching", self$handle, idx, as.matrix(reference_P), c(self$dims$K, self$dims$G, self$dims$N))
      ref_names <- if (is.null(colnames(reference_P))) paste0("Ref", seq_len(ncol(reference_P))) else colnames(reference_P)
      df <- data.frame(iter = rep(idx, each = N), estimated = paste0("Est", rep(seq_len(N), length(idx))),
                       assigned = ifelse(is.na(as.vector(r$assigned)), "None", ref_names[as.vector(r$assigned)]),
                       cosine_sim = as.vector(r$cosine), k = as.numeric(rep(seq_len(N), length(idx))),
                       included = ifelse(as.vector(r$included), "Included", "Excluded"))
      if (save_df) self$reference_comparison$label_switching_df <- df
      df
    }
  ),
  private = list(
    hip = NULL,
    # fixed_P as a double matrix, or NULL; refusals in the reference's ERROR: convention (what needs the dims is checked in sample_params)
    check_fixed_P = function(fixed_P) {
      if (is.null(fixed_P)) return(NULL)
      fp <- as.matrix(fixed_P); storage.mode(fp) <- "double"
      if (ncol(fp) < 1) stop("ERROR: fixed_P has no columns")
      if (anyNA(fp)) stop("ERROR: fixed_P has NaN entries")
      if (any(fp < 0 | is.infinite(fp))) stop("ERROR: fixed_P must be finite and non-negative")
      if (any(colSums(fp) == 0)) stop(glue::glue("ERROR: fixed_P column {which(colSums(fp) == 0)[1]} sums to 0"))
      unname(fp)
    },
    # the constructor's sample_params(from_prior = TRUE) + record_sample + update_sample_metrics
    sample_params = function(skip = c(), from_prior = FALSE) {
      if (!from_prior) stop("per-iteration sampling goes through run_block()")
      private$create_handle()
      for (nm in names(self$hyperprior_params)) if (nm %in% names(.bnmf_ids) && is.matrix(self$hyperprior_params[[nm]]))
        .Call("C_bnmf_set_array", self$handle, .bnmf_ids[[nm]], as.double(self$hyperprior_params[[nm]]))
      # prior parameters of iteration 1: the reference's constructor has already filled self$prior_params (user-supplied
      # init_prior_params verbatim, the rest drawn from the hyper-priors in R, R/sample_priors.R:15-141).  All of them go
      # to the device, which keeps supplied arrays verbatim (bnmf_set_array before bnmf_init), so samples$<name>[[1]]
      # equals what the constructor produced (vignettes/advanced.qmd:181-185, :245-249, :315-319).
      for (nm in names(self$prior_params)) if (nm %in% names(.bnmf_ids) && is.matrix(self$prior_params[[nm]]))
        .Call("C_bnmf_set_array", self$handle, .bnmf_ids[[nm]], as.double(self$prior_params[[nm]]))
      for (nm in skip) if (nm %in% names(.bnmf_ids)) .Call("C_bnmf_set_array", self$handle, .bnmf_ids[[nm]], as.double(self$params[[nm]]))
      fp <- private$hip$fixed_P
      if (!is.null(fp)) {
        if (nrow(fp) != self$dims$K) stop(glue::glue("ERROR: fixed_P has {nrow(fp)} rows, but data has {self$dims$K} rows."))
        if (ncol(fp) > self$dims$N) stop(glue::glue("ERROR: fixed_P has {ncol(fp)} columns, but the rank (or the top of the rank range) is {self$dims$N}; it must be >= {ncol(fp)}"))
        if ("P" %in% skip) {
          if (!identical(unname(as.matrix(self$params$P)[, seq_len(ncol(fp)), drop = FALSE]), unname(fp)))
            stop(glue::glue("ERROR: init_params$P contradicts fixed_P: its columns 1..{ncol(fp)} must equal fixed_P"))
        } else {                                             # the other columns: no value (NA), drawn from the prior by bnmf_init
          P0 <- matrix(NA_real_, self$dims$K, self$dims$N); P0[, seq_len(ncol(fp))] <- fp
          .Call("C_bnmf_set_array", self$handle, .bnmf_ids[["P"]], as.double(P0))
        }
        .Call("C_bnmf_set_fixed", self$handle, .bnmf_ids[["P"]], as.integer(seq_len(self$dims$N) <= ncol(fp)))
      }
      row <- .Call("C_bnmf_init", self$handle)
      private$pull_state(); private$bind_metrics(matrix(row, ncol = 1))
    },
    # the handle for this sampler's spec and data (C_bnmf_create, or C_bnmf_create_f64 for likelihood = "normal")
    create_handle = function() {
      lk <- c(poisson = 0L, normal = 1L); pr <- c(truncnormal = 0L, exponential = 1L, gamma = 2L)
      spec <- c(lk[[self$specs$likelihood]], pr[[self$specs$prior]], as.integer(self$specs$MH),
                as.integer(self$specs$learning_rank),
                if (isTRUE(self$specs$rank_method == "BFI")) 1L else 0L, as.integer(private$hip$save_Z),
                as.integer(if (self$specs$save_all_samples) length(self$temperature_schedule)
                           else self$specs$convergence_control$MAP_over))
      if (self$specs$likelihood == "normal") {
        # real-valued data, as the reference's Normal sampler reads them (R/sample_Pn.R, R/sample_params.R, R/utils.R)
        storage.mode(self$data) <- "double"
        self$handle <- .Call("C_bnmf_create_f64", self$data, c(self$dims$K, self$dims$G, self$dims$N), spec,
                             as.double(self$temperature_schedule), as.double(private$hip$seed),
                             as.integer(private$hip$chain_id), as.integer(private$hip$device))
      } else {
        storage.mode(self$data) <- "integer"
        self$handle <- .Call("C_bnmf_create", self$data, c(self$dims$K, self$dims$G, self$dims$N), spec,
                             as.double(self$temperature_schedule), as.double(private$hip$seed),
                             as.integer(private$hip$chain_id), as.integer(private$hip$device))
      }
      invisible(self$handle)
    },
    # load_bayesNMF_hip: a new handle on `device` with the stored spec, the saved device state replayed into it (bnmf_load_state:
    # parameters, hyper-priors, the kept samples, the MAP metrics' history), the log reopened for append
    reopen = function(output_dir, device) {
      path <- file.path(output_dir, "engine_state.bin")
      if (!file.exists(path)) stop(glue::glue("{path} does not exist: was the sampler run with save_engine_state = TRUE?"))
      info <- .Call("C_bnmf_state_info", path)           # every checksum, before a device is touched
      if (info$last_iter != self$state$iter) stop(glue::glue("{path} ends at iteration {info$last_iter}, sampler.rds at iteration {self$state$iter}"))
      private$hip$device <- as.integer(device)
      private$create_handle()
      if (!is.null(private$hip$fixed_P))                     # (the file carries the mask too: bnmf_load_state checks that the two agree)
        .Call("C_bnmf_set_fixed", self$handle, .bnmf_ids[["P"]], as.integer(seq_len(self$dims$N) <= ncol(private$hip$fixed_P)))
      it <- .Call("C_bnmf_load_state", self$handle, path)
      private$hip$state_iter <- as.integer(it)
      self$specs$output_dir <- output_dir
      self$log_con <- file(file.path(output_dir, "log.txt"), open = "at")
      invisible(self)
    },
    cc_int = function() {
      cc <- self$specs$convergence_control
      as.integer(c(cc$MAP_over, cc$MAP_every, cc$Ninarow_nochange, cc$Ninarow_nobest, cc$miniters, cc$maxiters,
                   match(cc$metric, c("loglikelihood", "logposterior", "RMSE", "KL", "BIC")) - 1L))
    },
    cc_state = function() {
      st <- self$state; have <- !is.null(st$prev_MAP_metric)
      nz <- function(x) if (is.null(x)) 0 else x
      as.double(c(isTRUE(st$converged), match(nz(st$why), c("no change", "no best", "max iters"), nomatch = 0), nz(st$best_iter),
                  nz(st$inarow_na), nz(st$inarow_no_change), nz(st$inarow_no_best), have, 0,
                  if (have) st$prev_MAP_metric else 0, if (have) st$best_MAP_metric else 0, nz(st$prev_percent_change)))
    },
    # what an engine-side loop returns -> state$sample_metrics, state$MAP_metrics, the convergence counters
    absorb = function(res, cc) {
      if (ncol(res$metrics) > 0) { private$bind_metrics(res$metrics); self$state$iter <- res$metrics[1, ncol(res$metrics)] }
      mm_names <- c("iter", "RMSE", "KL", "loglikelihood", "logposterior", "n_params", "BIC", "rank", "MAP_A_counts", "mean_temp",
                    "P_mean_acceptance_rate", "E_mean_acceptance_rate")
      for (j in seq_len(ncol(res$map_rows))) {
        row <- as.data.frame(t(res$map_rows[1:12, j])); names(row) <- mm_names
        self$state$MAP_metrics <- rbind(self$state$MAP_metrics, row[, names(self$state$MAP_metrics)])
      }
      st <- res$state
      if (st[7] == 1) {
        self$state$prev_MAP_metric <- st[9]; self$state$best_MAP_metric <- st[10]; self$state$prev_percent_change <- st[11]
        self$state$inarow_na <- st[4]; self$state$inarow_no_change <- st[5]; self$state$inarow_no_best <- st[6]
        if (st[3] > 0) self$state$best_iter <- st[3]
      }
      if (st[1] == 1 && !isTRUE(self$state$converged)) {
        self$state$converged <- TRUE; self$state$why <- c("no change", "no best", "max iters")[st[2]]
        self$state$converged_iter <- self$state$iter
      } else if (st[2] > 0) {
        self$state$why <- c("no change", "no best", "max iters")[st[2]]   # check_convergence_ keeps updating `why` during the post-warm-up checks
      }
    },
    record_sample = function() invisible(NULL),          # recorded on the device (bnmf_window)
    update_sample_metrics = function(update_trace = FALSE) invisible(NULL),
    run_block = function(n, converged) {
      met <- .Call("C_bnmf_run", self$handle, as.integer(n), as.logical(converged))
      self$state$iter <- self$state$iter + n
      private$bind_metrics(met); private$pull_state()
    },
    bind_metrics = function(met) {
      df <- as.data.frame(t(met)); names(df) <- .bnmf_metric_names
      self$state$sample_metrics <- rbind(self$state$sample_metrics, df[, names(self$state$sample_metrics)])
    },
    pull_state = function() {
      get <- function(nm, dim) { x <- .Call("C_bnmf_get_array", self$handle, .bnmf_ids[[nm]], as.double(prod(dim))); dim(x) <- dim; x }
      K <- self$dims$K; N <- self$dims$N; G <- self$dims$G
      self$params$P <- get("P", c(K, N)); self$params$E <- get("E", c(N, G)); self$params$A <- get("A", c(1, N))
      self$params$R <- get("R", 1)
      for (nm in names(self$prior_params)) if (nm %in% names(.bnmf_ids))
        self$prior_params[[nm]] <- get(nm, if (grepl("_p$", nm)) c(K, N) else c(N, G))
    },
    # samples[[name]][[i]] of the last n recorded iterations (record_sample, R/bayesNMF_sampler.R:651-672): every name the
    # reference records (params, prior_params, acceptance rates, sigmasq).  With save_all_samples the lists are indexed
    # by iteration (as in the reference) and MAP_idx is the last MAP_over iterations; otherwise positions 1..n.
    pull_window = function() {
      n <- min(self$specs$convergence_control$MAP_over, self$state$iter)
      K <- self$dims$K; N <- self$dims$N; G <- self$dims$G
      nms <- c("P", "E", "A", "R", names(self$prior_params))
      if (self$specs$MH) nms <- c(nms, "P_acceptance_rate", "E_acceptance_rate")
      if (self$specs$likelihood == "normal") nms <- c(nms, "sigmasq")
      first <- if (self$specs$save_all_samples) self$state$iter - n + 1 else 1
      for (nm in intersect(nms, names(.bnmf_ids))) {
        d <- if (nm == "A") c(1, N) else if (nm == "R") 1 else if (nm == "sigmasq") G else
             if (nm == "P" || grepl("_p$", nm) || nm == "P_acceptance_rate") c(K, N) else c(N, G)
        w <- .Call("C_bnmf_window", self$handle, .bnmf_ids[[nm]], as.integer(n), as.double(prod(d)))
        if (is.null(self$samples[[nm]])) self$samples[[nm]] <- list()
        for (i in seq_len(n)) self$samples[[nm]][[first + i - 1]] <- array(w[, i], dim = d)
      }
      self$state$MAP_idx <- seq(first, first + n - 1)
    }
  )
)

# readRDS of a bayesNMF_sampler_hip gives a sampler whose handle is a dead external pointer ("bnmf: handle was destroyed"): this
# reopens it.  The sampler must have been run with save_engine_state = TRUE.  The result is live: get_MAP(end_iter, n_samples),
# assign_signatures_ensemble, label_switching_df and run_gibbs_sampler() (resume, bit for bit as the uninterrupted chain) all reach
# the device again.
load_bayesNMF_hip <- function(output_dir, device = 0L) {
  sampler <- readRDS(file.path(output_dir, "sampler.rds"))
  sampler$.__enclos_env__$private$reopen(output_dir, device)
  sampler
}

# bayesNMF(rank = <range>, rank_method = "WAIC") on the HIP engine (not in the reference, whose fixed-rank criterion is "BIC",
# R/bayesNMF.R:66-126): the same per-rank sweep — one fixed-rank sampler per rank, the ranks below ncol(fixed_P) dropped — with
# get_WAIC() over each sampler's final MAP window.  The table carries elpd_waic, se_elpd, p_waic, n_high_var and BIC for comparison;
# best_rank is the largest elpd_waic.  rank_method = "BIC" gives the reference's choice from the same sweep.
bayesNMF_hip_ranks <- function(data, rank, rank_method = "WAIC", output_dir = "nmf_hip", fixed_P = NULL, ...) {
  if (!rank_method %in% c("BIC", "WAIC")) stop("Rank method must be BIC or WAIC for a per-rank sweep")
  if (!is.null(fixed_P)) {
    nf <- ncol(as.matrix(fixed_P))
    if (any(rank < nf)) message(glue::glue("fixed_P has {nf} columns: dropping ranks below {nf} from the {rank_method} sweep"))
    rank <- rank[rank >= nf]
    if (length(rank) == 0) stop(glue::glue("ERROR: fixed_P has {nf} columns, but the top of the rank range is below {nf}"))
  }
  samplers <- list(); rows <- list()
  for (k in rank) {
    s <- bayesNMF_sampler_hip$new(data = data, rank = k, output_dir = file.path(output_dir, paste0("rank_", k)), fixed_P = fixed_P, ...)
    s$run_gibbs_sampler()
    row <- data.frame(rank = k, dir = s$specs$output_dir, BIC = utils::tail(s$state$MAP_metrics$BIC, 1), time = as.numeric(s$time$total))
    if (rank_method == "WAIC") {
      w <- s$get_WAIC()
      row <- cbind(row, data.frame(elpd_waic = w$elpd_waic, se_elpd = w$se_elpd, p_waic = w$p_waic, n_high_var = w$n_high_var))
    }
    samplers[[as.character(k)]] <- s; rows[[length(rows) + 1]] <- row
  }
  results <- do.call(rbind, rows)
  best <- if (rank_method == "WAIC") results$rank[which.max(results$elpd_waic)] else results$rank[which.min(results$BIC)]
  results <- if (rank_method == "WAIC") results[order(-results$elpd_waic), ] else results[order(results$BIC), ]
  list(results = results, best_rank = best, sampler = samplers[[as.character(best)]])
}
