"""Host-side mirror of the reference's R interface for the Gibbs path: `bayesNMF()`
(R/bayesNMF.R:24-138) and the R6 class `bayesNMF_sampler` (R/bayesNMF_sampler.R:8-747) — same names,
argument meaning, defaults, field names and error messages — driving the HIP engine through the C ABI
(one call per block of <= MAP_every iterations instead of R-level work per iteration).

The sampling path is mirrored, and of the post-processing the reference assignment
(assign_signatures_ensemble), summary() and summarize_samplers() (R/postprocessing.R:18-152); the plots
are out of scope.  New optional trailing arguments: seed, chain_id, device, save_Z.
"""
import datetime
import os
import pickle
import shutil
import time
from collections import Counter

import numpy as np
import pandas as pd

from .convergence import check_convergence, new_convergence_control
from .engine import Engine
from .setup import apply_hyperprior_params

_PRIOR_PARAM_NAMES = {"truncnormal": ["Mu_p", "Sigmasq_p", "Mu_e", "Sigmasq_e"],
                      "exponential": ["Lambda_p", "Lambda_e"],
                      "gamma": ["Alpha_p", "Beta_p", "Alpha_e", "Beta_e"]}


def get_temp_sched_(length, n_temp, rng=None):
    """get_temp_sched_ (R/utils.R:307-332): 0, 1e-9..1e-5, 8 x 1e-4, (1..9.9)e-4..e-1, then 1."""
    nX = max(int(round(n_temp / 374)), 1)
    sched = [0.0] * nX
    for x in range(9, 4, -1):
        sched += [10.0 ** (-x)] * nX
    sched += [10.0 ** (-4)] * int(round(8 * nX))
    for y in range(4, 0, -1):
        for x in np.arange(0, 8.9 + 1e-9, 0.1):
            sched += [(1 + x) * 10.0 ** (-y)] * nX
    sched = np.array(sched)
    if len(sched) > n_temp:
        rng = rng or np.random.default_rng(0)
        sched = np.sort(rng.choice(sched, size=n_temp, replace=False))
    return np.concatenate([sched, np.ones(max(length - len(sched), 0))])


def renormalize(P, E):
    """renormalize (R/helpers.R:35-49): columns of P sum to 1, product P E unchanged."""
    cs = P.sum(axis=0)
    return P / cs[None, :], E * cs[:, None]


def get_mode(matrix_list):
    """get_mode (R/helpers.R:63-79): most frequent matrix by its pasted string."""
    keys = ["".join(str(int(v)) if float(v).is_integer() else str(v) for v in np.ravel(m, order="F")) for m in matrix_list]
    # sort(table(.), decreasing = TRUE): table() orders the patterns alphabetically and the sort is stable
    counts = sorted(Counter(keys).items(), key=lambda kv: (-kv[1], kv[0]))
    mode = counts[0][0]
    idx = [i for i, k in enumerate(keys) if k == mode]
    return dict(matrix=matrix_list[idx[0]], top_counts=counts[:5], idx=idx)


def contrast_labels(groups, G):
    """get_contrast's labels: groups (G labels of any hashable kind; None / NaN = left out) -> (int32 labels 0 .. C-1 in order of first
    appearance, -1 = left out; the C names)"""
    gl = list(groups.tolist()) if hasattr(groups, "tolist") else list(groups)
    if len(gl) != G:
        raise ValueError(f"groups has {len(gl)} labels for {G} tumours")
    number, labels = {}, np.full(G, -1, dtype=np.int32)
    for g, v in enumerate(gl):
        if v is None or v is pd.NA or (isinstance(v, float) and v != v):
            continue
        labels[g] = number.setdefault(v, len(number))
    return labels, list(number)


def regression_design(covariates, G, intercept=True, standardize=False):
    """get_regression's design: covariates (a G x Q0 array, or a mapping name -> column of G values; None / NaN = missing) ->
    (design G x Q float64, include: int32 0 / 1 flags of the tumours without a missing value or None when every tumour is complete,
    the Q column names).  intercept prepends the column of ones, "(Intercept)"; standardize centres and scales every other column by
    the mean and the standard deviation (n - 1 form) of the included rows."""
    def column(col):
        vals = list(col.tolist()) if hasattr(col, "tolist") else list(col)
        return np.array([np.nan if v is None or v is pd.NA else float(v) for v in vals], dtype=np.float64)
    if hasattr(covariates, "items"):
        names, cols = [str(k) for k, _ in covariates.items()], [column(c) for _, c in covariates.items()]
    else:
        arr = np.asarray(covariates, dtype=object)
        if arr.ndim == 1:
            arr = arr[:, None]
        if arr.ndim != 2:
            raise ValueError(f"covariates has {arr.ndim} dimensions: a G x Q array or a mapping name -> column is needed")
        cols = [column(arr[:, j]) for j in range(arr.shape[1])]
        names = [f"x{j + 1}" for j in range(len(cols))]
    for nm, c in zip(names, cols):
        if c.size != G:
            raise ValueError(f"covariate {nm} has {c.size} values for {G} tumours")
    X = np.stack(cols, axis=1) if cols else np.empty((G, 0))
    complete = ~np.isnan(X).any(axis=1)
    if standardize:
        for j, nm in enumerate(names):
            v = X[complete, j]
            sd = v.std(ddof=1) if v.size > 1 else 0.0
            if not sd > 0:
                raise ValueError(f"covariate {nm} is constant over the included tumours: it cannot be standardized")
            X[:, j] = (X[:, j] - v.mean()) / sd
    if intercept:
        X, names = np.concatenate([np.ones((G, 1)), X], axis=1), ["(Intercept)"] + names
    return np.asfortranarray(X), (None if complete.all() else complete.astype(np.int32)), names


def residual_candidate(vbar):
    """The candidate signature of get_residuals: the positive part of the component vbar (K), or of -vbar where the negative part has the
    larger sum of squares, normalised to sum 1 (all NaN where vbar is not finite or has no such part)."""
    v = np.asarray(vbar, dtype=np.float64)
    pos, neg = np.maximum(v, 0.0), np.maximum(-v, 0.0)
    part = neg if (neg * neg).sum() > (pos * pos).sum() else pos
    tot = part.sum()
    return part / tot if np.isfinite(tot) and tot > 0 else np.full(v.shape, np.nan)


def subtype_seeds(profiles, C, member=None):
    """The start of get_subtypes(n_subtypes = C): C tumours by a deterministic farthest-first walk over the share profiles (N x G; member:
    G flags of the tumours that may be chosen, None = all).  The first seed is the member nearest (squared Euclidean distance) to the
    members' mean profile; each next seed is the member farthest from its nearest chosen seed; the lower tumour wins a tie."""
    prof = np.asarray(profiles, dtype=np.float64)
    G = prof.shape[1]
    mem = np.ones(G, dtype=bool) if member is None else np.asarray(member, dtype=bool)
    if C < 1 or C > int(mem.sum()):
        raise ValueError(f"{C} seeds cannot be chosen among {int(mem.sum())} tumours")
    d = ((prof - prof[:, mem].mean(axis=1, keepdims=True)) ** 2).sum(axis=0)
    seeds = [int(np.argmin(np.where(mem, d, np.inf)))]                     # (argmin and argmax return the first of equals: the lower tumour)
    near = ((prof - prof[:, [seeds[0]]]) ** 2).sum(axis=0)
    while len(seeds) < C:
        g = int(np.argmax(np.where(mem, near, -np.inf)))
        seeds.append(g)
        near = np.minimum(near, ((prof - prof[:, [g]]) ** 2).sum(axis=0))
    return np.asarray(seeds, dtype=np.int32)


class bayesNMF_sampler:
    """Python mirror of the R6 class `bayesNMF_sampler` (public fields of R/bayesNMF_sampler.R:11-67)."""

    def __init__(self, data, rank, likelihood="poisson", prior="truncnormal", rank_method="SBFI",
                 MH=None, convergence_control=None, prop_temp=0.2, post_warmup=None,
                 output_dir=None, overwrite=False, hyperprior_params=None, init_prior_params=None,
                 init_params=None, verbosity=1, periodic_save=True, save_all_samples=False,
                 seed=1, chain_id=0, device=0, save_Z=False, engine_factory=None, intermediate_credible_intervals=False,
                 engine_side_convergence=True, save_engine_state=False, fixed_P=None):
        if MH is None:
            MH = likelihood == "poisson" and prior in ("truncnormal", "exponential")
        cc = dict(convergence_control) if convergence_control is not None else new_convergence_control()
        if post_warmup is None:
            post_warmup = 2 * cc["MAP_over"]
        if output_dir is None:
            output_dir = f"nmf_{likelihood}_{prior}"
        # output dir handling (R/bayesNMF_sampler.R:110-121)
        final_dir, tail = output_dir, 0
        while not overwrite and os.path.isdir(final_dir):
            tail += 1
            final_dir = f"{output_dir}_{tail}"
        if overwrite and os.path.isdir(final_dir):
            shutil.rmtree(final_dir)
        os.makedirs(final_dir, exist_ok=True)

        rank = np.atleast_1d(np.asarray(rank, dtype=int))
        learning_rank = rank.size > 1
        if learning_rank and rank.min() != 0:
            rank = np.arange(0, rank.max() + 1)
        display_rank = f"{rank.min()}:{rank.max()}" if learning_rank else int(rank[0])
        self.tumour_names = [str(c) for c in data.columns] if hasattr(data, "columns") else None   # (get_similarity's tables)
        data = np.asarray(data)
        n_iters = cc["maxiters"] + (post_warmup if MH else 0)
        if learning_rank:
            self.temperature_schedule = get_temp_sched_(n_iters, int(round(prop_temp * cc["maxiters"])),
                                                        rng=np.random.default_rng(seed))
        else:
            self.temperature_schedule = np.ones(n_iters)
        self.data = data
        self.dims = dict(K=data.shape[0], N=int(rank.max()), G=data.shape[1])
        self.specs = dict(rank=rank, likelihood=likelihood, prior=prior, MH=bool(MH), learning_rank=learning_rank,
                          convergence_control=cc, output_dir=final_dir, overwrite=overwrite, verbosity=verbosity,
                          periodic_save=periodic_save, save_all_samples=save_all_samples, save_Z=bool(save_Z),
                          intermediate_credible_intervals=intermediate_credible_intervals,
                          engine_side_convergence=engine_side_convergence)
        if learning_rank:
            self.specs["prop_temp"] = prop_temp
            self.specs["rank_method"] = rank_method
        if MH:
            self.specs["post_warmup"] = post_warmup
        window = n_iters if save_all_samples else cc["MAP_over"]
        if save_engine_state:
            # what load_sampler needs to rebuild the engine the saved state belongs to
            self.specs.update(save_engine_state=True, seed=seed, chain_id=chain_id, window=window, device=device,
                              engine_rank_method=rank_method if rank_method in ("SBFI", "BFI") else "SBFI")
        self.state = dict(iter=1, indent=0, converged=False)
        self.MAP = dict(assignment_res=None)
        self.credible_intervals = {}
        self.reference_comparison = dict(reference_P=None, assignments=None, keep_sigs=None, idxs=None, votes=None,
                                         summary=None, plots={}, label_switching_df=None)
        self.time = {}
        self._block_hook = None          # multi-chain launcher: called after every block (multichain.ChainSync.block)
        self.acceptance_rates = dict(P_acceptance_rate=None, E_acceptance_rate=None)
        self.log_con = open(os.path.join(final_dir, "log.txt"), "w")
        self.log("Initialized sampler", verbosity=1)
        self.state["indent"] = 1
        self.log(f"likelihood = {likelihood}, prior = {prior}, MH = {str(bool(MH)).upper()}", verbosity=1)
        self.log(f"learning_rank = {str(learning_rank).upper()}, rank = {display_rank}", verbosity=1)
        self.log(f"maxiters = {cc['maxiters']}", verbosity=1)
        self.log(f"MAP_over = {cc['MAP_over']}", verbosity=1)
        self.log(f"MAP_every = {cc['MAP_every']}", verbosity=1)
        cols = ["iter", "RMSE", "KL", "loglikelihood", "logposterior", "n_params", "BIC", "rank"]
        extra = ["P_mean_acceptance_rate", "E_mean_acceptance_rate"] if MH else []
        self.state["MAP_metrics"] = pd.DataFrame(columns=cols + ["MAP_A_counts", "mean_temp"] + extra, dtype=float)
        self.state["sample_metrics"] = pd.DataFrame(columns=cols + ["temp"] + extra, dtype=float)
        self.state["MAP_idx"] = np.arange(1, cc["MAP_over"] + 1)
        self.state["indent"] = 0
        self.log("Setup", verbosity=1)
        self.state["indent"] = 1
        self.log("Setting hyperprior parameters", verbosity=1)
        self._check_model()
        self.log("Model check passed", verbosity=1)
        fixed = self._check_fixed_P(fixed_P, init_params)
        if fixed is not None:
            self.specs["fixed_P"] = fixed                 # (kept by save_object: load_sampler rebuilds the same engine)
            self.log(f"fixed_P: columns 1..{fixed.shape[1]} of P held fixed" + (" (refit: only E is sampled)" if fixed.shape[1] == self.dims["N"] else ""),
                     verbosity=1)

        factory = engine_factory or Engine
        kw = dict(likelihood=likelihood, prior=prior, MH=bool(MH), learning_rank=learning_rank,
                  rank_method=rank_method if rank_method in ("SBFI", "BFI") else "SBFI",
                  seed=seed, chain_id=chain_id, temperature=self.temperature_schedule, save_Z=save_Z)
        if engine_factory is None:
            kw.update(window=window, device=device)
        # Normal: real-valued data as they are (float64); Poisson: counts (int32)
        dt = np.float64 if likelihood == "normal" else np.int32
        self._chain = factory(np.asfortranarray(data, dtype=dt), self.dims["N"], **kw)
        if save_engine_state and not hasattr(self._chain, "save_state"):
            self.close()
            raise ValueError("save_engine_state = TRUE needs an engine that can save its state (save_state); this engine_factory's cannot")
        if fixed is not None and not hasattr(self._chain, "set_fixed"):
            self.close()
            raise ValueError("fixed_P needs an engine that can hold columns of P fixed (set_fixed); this engine_factory's cannot")
        self.hyperprior_params = apply_hyperprior_params(self._chain, prior, data, self.dims["N"], hyperprior_params)
        self.log("Initializing prior parameters and parameters", verbosity=1)
        for name, val in (init_prior_params or {}).items():
            self._chain.set(name, val)
        for name, val in (init_params or {}).items():
            self._chain.set(name, val)
        if fixed is not None:
            F = fixed.shape[1]
            if "P" not in (init_params or {}):                 # the other columns: no value (NaN), drawn from the prior by init()
                P0 = np.full((self.dims["K"], self.dims["N"]), np.nan)
                P0[:, :F] = fixed
                self._chain.set("P", P0)
            mask = np.zeros(self.dims["N"], dtype=np.int32)
            mask[:F] = 1
            self._chain.set_fixed("P", mask)
        self.log("Sampling parameters from priors", verbosity=1)
        row = self._chain.init()
        self.log("Logging initial sample", verbosity=1)
        self.log("Logging initial sample metrics", verbosity=1)
        self._append_metrics(np.asarray(row)[None, :])
        self._sync_state()
        self.state["indent"] = 0

    # ---------------------------------------------------------------- helpers
    def _check_model(self):
        """check_model (R/bayesNMF_sampler.R:623-645): same messages."""
        lk, pr, MH = self.specs["likelihood"], self.specs["prior"], self.specs["MH"]
        if lk not in ("normal", "poisson"):
            self._error("likelihood must be one of normal, poisson")
        if lk == "normal":
            if pr not in ("truncnormal", "exponential"):
                self._error("prior must be one of c('truncnormal','exponential') with `likelihood = 'normal'`")
        else:
            if pr not in ("gamma", "exponential", "truncnormal"):
                self._error("prior must be one of c('gamma','exponential','truncnormal') with `likelihood = 'poisson'`")
            if pr == "gamma" and MH:
                self._error("gamma prior cannot be used in a MH-within-gibbs sampler")
            if pr == "truncnormal" and not MH:
                self._error("truncnormal prior can only be used in a MH-within-gibbs sampler")

    def _check_fixed_P(self, fixed_P, init_params):
        """fixed_P (K x F): known signatures that become columns 1..F of P and are never drawn.  Returns it as a float array, or None."""
        if fixed_P is None:
            return None
        K, N = self.dims["K"], self.dims["N"]
        fp = np.asarray(fixed_P, dtype=float)
        if fp.ndim == 1:
            fp = fp[:, None]
        if fp.ndim != 2 or fp.shape[0] != K:
            self._error(f"fixed_P has {fp.shape[0]} rows, but data has {K} rows.")
        F = fp.shape[1]
        if F < 1:
            self._error("fixed_P has no columns")
        if F > N:
            self._error(f"fixed_P has {F} columns, but the rank (or the top of the rank range) is {N}; it must be >= {F}")
        if np.isnan(fp).any():
            self._error(f"fixed_P has NaN entries (column {int(np.argwhere(np.isnan(fp))[0][1]) + 1})")
        bad = (fp < 0) | np.isinf(fp)
        if bad.any():
            self._error(f"fixed_P must be finite and non-negative (column {int(np.argwhere(bad)[0][1]) + 1})")
        zero = np.where(fp.sum(axis=0) == 0)[0]
        if zero.size:
            self._error(f"fixed_P column {int(zero[0]) + 1} sums to 0")
        ip = (init_params or {}).get("P")
        if ip is not None:
            ip = np.asarray(ip, dtype=float)
            if ip.shape != (K, N) or not np.array_equal(ip[:, :F], fp):
                self._error(f"init_params$P contradicts fixed_P: its columns 1..{F} must equal fixed_P")
        return np.ascontiguousarray(fp)

    def _error(self, msg):
        msg = "ERROR: " + msg
        if self.log_con is not None:
            ts = datetime.datetime.now().strftime("%Y-%m-%d %H:%M:%S")
            self.log_con.write(f"[{ts}] {msg}\n")
            self.log_con.flush()
        raise ValueError(msg)

    def log(self, msg, verbosity=5):
        """log (R/bayesNMF_sampler.R:423-455): `[timestamp] <tabs><msg>`."""
        if verbosity > self.specs["verbosity"] or msg is None or self.log_con is None:
            return
        lines = str(msg).split("\n")
        ts = datetime.datetime.now().strftime("%Y-%m-%d %H:%M:%S")
        indent = "\t" * self.state["indent"]
        out = [indent + lines[0]] + [indent + " " * (len(ts) + 1) + ln for ln in lines[1:]]
        out = [ln for ln in out if ln.strip() != ""]
        self.log_con.write(f"[{ts}] " + "\n".join(out) + "\n")
        self.log_con.flush()

    def _append_metrics(self, rows):
        cols = list(self.state["sample_metrics"].columns)
        names = ["iter", "RMSE", "KL", "loglikelihood", "logposterior", "n_params", "BIC", "rank", "temp",
                 "P_mean_acceptance_rate", "E_mean_acceptance_rate"]
        df = pd.DataFrame(rows, columns=names)[cols]
        self.state["sample_metrics"] = df if self.state["sample_metrics"].empty else \
            pd.concat([self.state["sample_metrics"], df], ignore_index=True)

    def _sync_state(self):
        """Materialise the device state into the R6-style fields (params, prior_params)."""
        names = ["P", "E", "A", "R"] + (["sigmasq"] if self.specs["likelihood"] == "normal" else [])
        self.params = {n: self._chain.get(n) for n in names}
        self.prior_params = {n: self._chain.get(n) for n in _PRIOR_PARAM_NAMES[self.specs["prior"]]}
        if self.specs["MH"]:
            self.acceptance_rates = {n: self._chain.get(n) for n in ("P_acceptance_rate", "E_acceptance_rate")}

    @property
    def samples(self):
        """samples[[name]][[i]] of the last min(iter, window) iterations (record_sample, :651-672)."""
        cc = self.specs["convergence_control"]
        n = min(self.state["iter"], len(self.temperature_schedule) if self.specs["save_all_samples"] else cc["MAP_over"])
        names = ["P", "E", "A", "R"] + _PRIOR_PARAM_NAMES[self.specs["prior"]]
        if self.specs["MH"]:
            names += ["P_acceptance_rate", "E_acceptance_rate"]
        if self.specs["likelihood"] == "normal":
            names += ["sigmasq"]
        out = {nm: self._chain.window(nm, n) for nm in names}
        if self.specs.get("save_Z"):
            try:
                out["Z"] = self._chain.window("Z", n)
            except Exception:  # noqa: BLE001  (Z history not kept: too large for the device ring)
                pass
        return out

    # ---------------------------------------------------------------- public utilities (R/utils.R)
    def get_Mhat(self, P=None, A=None, E=None):
        P = self.params["P"] if P is None else P
        A = self.params["A"] if A is None else A
        E = self.params["E"] if E is None else E
        return (P * np.ravel(A)[None, :]) @ E

    def get_loglik(self, P=None, A=None, E=None):
        from scipy.stats import poisson
        Mhat = np.maximum(self.get_Mhat(P, A, E), 1e-6)
        return float(poisson.logpmf(self.data, Mhat).sum())

    def _kept_range(self):
        """The recorded iterations the engine still keeps: [max(1, iter - window + 1), iter], window = all iterations with
        save_all_samples, else MAP_over (as `samples`)."""
        it = self.state["iter"]
        W = len(self.temperature_schedule) if self.specs["save_all_samples"] else self.specs["convergence_control"]["MAP_over"]
        return max(1, it - W + 1), it

    def get_MAP(self, end_iter=None, n_samples=None, final=False, credible_interval=0.95):
        """get_MAP_ (R/utils.R:194-288).  end_iter = iter (the default): over the window state$MAP_idx of recorded samples, whatever
        n_samples says (as the reference).  Any other end_iter (save_all_samples only): over iterations end_iter - n_samples + 1 ...
        end_iter, n_samples defaulting to MAP_over.  MAP["idx"]: the iterations of that range whose A is the mode."""
        cc = self.specs["convergence_control"]
        it = self.state["iter"]
        end_iter = it if end_iter is None else int(end_iter)
        if not self.specs["save_all_samples"] and end_iter != it:
            raise ValueError("end_iter cannot be provided unless self$specs$save_all_samples is TRUE")
        at = None
        if end_iter == it:
            n = min(cc["MAP_over"], it)
        else:
            n = cc["MAP_over"] if n_samples is None else int(n_samples)
            lo, hi = self._kept_range()
            if n < 1 or end_iter - n + 1 < lo or end_iter > hi:
                raise ValueError(f"iterations {end_iter - n + 1}..{end_iter} are not all recorded: the kept samples are iterations {lo}..{hi}")
            at = end_iter
        first_iter = end_iter - n + 1

        def window(name):                                  # the n samples of the range, oldest first
            return self._chain.window(name, n) if at is None else self._chain.window(name, it - first_iter + 1)[:n]
        if hasattr(self._chain, "map"):
            # on-device window statistics: one C-ABI call returns K*N + N*G means (+ credible bounds), no window copy
            try:
                r = self._chain.map(n, credible_interval) if at is None else self._chain.map(n, credible_interval, end_iter=at)
            except Exception as ex:     # e.g. a credible interval that needs more order statistics than the device keeps
                if "bnmf_window" not in str(ex):
                    raise
                r = None
            if r is not None:
                keep = np.where(np.ravel(r["A"]) == 1)[0] if final else np.arange(self.dims["N"])
                counts = [("".join(str(int(v)) for v in row), c) for row, c in zip(r["top_A"], r["top_counts"])]
                self.MAP = dict(P=r["P"][:, keep], A=r["A"][:, keep], E=r["E"][keep, :],
                                idx=[first_iter + i for i in np.where(r["used"])[0]], A_counts=counts, keep_sigs=keep,
                                RMSE=r["rmse"], KL=r["kl"])
                if r["P_lower"] is not None:
                    self.credible_intervals = dict(P=dict(lower=r["P_lower"][:, keep], upper=r["P_upper"][:, keep]),
                                                   E=dict(lower=r["E_lower"][keep, :], upper=r["E_upper"][keep, :]))
                return self.MAP
        A_list = window("A")
        mode = get_mode(A_list)
        idx = mode["idx"]
        keep = np.where(np.ravel(mode["matrix"]) == 1)[0] if final else np.arange(self.dims["N"])
        Ps, Es = window("P"), window("E")
        rs = [renormalize(Ps[i], Es[i]) for i in idx]
        Pm = np.mean([r[0][:, keep] for r in rs], axis=0)
        Em = np.mean([r[1][keep, :] for r in rs], axis=0)
        self.MAP = dict(P=Pm, A=np.asarray(mode["matrix"]).reshape(1, -1)[:, keep], E=Em,
                        idx=[first_iter + i for i in idx], A_counts=mode["top_counts"], keep_sigs=keep)
        if not credible_interval:
            return self.MAP
        probs = [0.5 - credible_interval / 2, 0.5 + credible_interval / 2]
        Parr = np.stack([r[0][:, keep] for r in rs], axis=2)
        Earr = np.stack([r[1][keep, :] for r in rs], axis=2)
        self.credible_intervals = dict(
            P=dict(lower=np.quantile(Parr, probs[0], axis=2), upper=np.quantile(Parr, probs[1], axis=2)),
            E=dict(lower=np.quantile(Earr, probs[0], axis=2), upper=np.quantile(Earr, probs[1], axis=2)))
        return self.MAP

    def _update_MAP_metrics(self, final=False):
        """update_MAP_metrics_ (R/utils.R:356-397)."""
        G, K = self.dims["G"], self.dims["K"]
        P, A, E = self.MAP["P"], self.MAP["A"], self.MAP["E"]
        if final:
            A = np.ones((1, P.shape[1]))
        sm = self.state["sample_metrics"]
        cc_ = self.specs["convergence_control"]
        n_win = min(cc_["MAP_over"], self.state["iter"])
        window = np.arange(self.state["iter"] - n_win + 1, self.state["iter"] + 1)   # state$MAP_idx: the whole window, not MAP$idx
        win = sm[sm["iter"].isin(window)]
        ll, lpost = float(win["loglikelihood"].mean()), float(win["logposterior"].mean())
        n_params = float(np.sum(A) * (G + K))
        if "RMSE" in self.MAP:                      # computed on the device with the window statistics
            rmse, kl = float(self.MAP["RMSE"]), float(self.MAP["KL"])
        else:
            Mhat = (P * np.ravel(A)[None, :]) @ E
            Mt, Mh = np.maximum(self.data, 1e-6), np.maximum(Mhat, 1e-6)
            rmse, kl = float(np.sqrt(np.mean((Mhat - self.data) ** 2))), float(np.sum(Mt * np.log(Mt / Mh)))
        row = dict(iter=self.state["iter"], RMSE=rmse, KL=kl, loglikelihood=ll, logposterior=lpost, n_params=n_params,
                   BIC=-2 * ll + n_params * np.log(G), rank=float(np.sum(self.MAP["A"])),
                   MAP_A_counts=float(self.MAP["A_counts"][0][1]),
                   mean_temp=float(np.mean(self.temperature_schedule[window - 1])))
        if self.specs["MH"]:                        # compute_metrics_ uses the CURRENT acceptance matrices (R/utils.R:444-452)
            row["P_mean_acceptance_rate"] = float(sm["P_mean_acceptance_rate"].iloc[-1])
            row["E_mean_acceptance_rate"] = float(sm["E_mean_acceptance_rate"].iloc[-1])
        df = pd.DataFrame([row])
        self.state["MAP_metrics"] = df if self.state["MAP_metrics"].empty else \
            pd.concat([self.state["MAP_metrics"], df], ignore_index=True)
        return row

    def _check(self, final=False):
        self.log(f"iter = {self.state['iter']}", verbosity=1)
        self.state["indent"] = 2
        self.log("Computing MAP", verbosity=1)
        # The reference recomputes the credible intervals at EVERY check (credible_intervals starts as list(), not NULL:
        # R/bayesNMF_sampler.R:49, R/utils.R:269) although nothing reads them before the final MAP.  Here they are
        # materialised at the final MAP and on every user call of get_MAP(); intermediate_credible_intervals=True
        # restores the reference's every-check behaviour.
        ci = 0.95 if (final or self.specs.get("intermediate_credible_intervals")) else None
        self.get_MAP(final=final, credible_interval=ci)
        if self.specs["learning_rank"]:
            self.log("\n".join(f"{k}  {v}" for k, v in self.MAP["A_counts"]), verbosity=1)
        self.log("Checking convergence", verbosity=1)
        row = self._update_MAP_metrics(final=final)
        cc = self.specs["convergence_control"]
        msg = check_convergence(self.state, cc, row[cc["metric"]], self.temperature_schedule)
        self.log(msg, verbosity=1)
        self.state["indent"] = 1
        return msg

    # ---------------------------------------------------------------- the sampling loop
    def run_gibbs_sampler(self):
        """run_gibbs_sampler (R/bayesNMF_sampler.R:265-408) with one engine call per block."""
        cc = self.specs["convergence_control"]
        self.log("Starting Gibbs sampler", verbosity=1)
        start = time.time()
        self.state["indent"] = 1
        if (hasattr(self._chain, "run_until") and self._block_hook is None and not self.specs["periodic_save"]
                and not self.specs["save_all_samples"] and self.specs.get("engine_side_convergence", True)):
            self._run_until_on_engine(cc)
        while not self.state["converged"] and self.state["iter"] < cc["maxiters"]:
            it = self.state["iter"]
            nxt = (it // cc["MAP_every"] + 1) * cc["MAP_every"]
            n = min(nxt, cc["maxiters"]) - it
            rows = self._chain.run(n, converged=False)
            self._append_metrics(rows)
            self.state["iter"] = it + n
            it = self.state["iter"]
            if (it % cc["MAP_every"] == 0 and it >= max(cc["MAP_over"], cc["MAP_every"])) or it >= cc["maxiters"]:
                if self.specs["save_all_samples"]:
                    self.state["MAP_idx"] = np.arange(it - cc["MAP_over"] + 1, it + 1)
                self._check()
                if self.state["converged"]:
                    self.state["converged_iter"] = it
                    self.log(f"Converged at {it} due to {self.state['why']}", verbosity=1)
                if self.specs["periodic_save"]:
                    self.log("Saving object", verbosity=1)
                    self.save_object()
            if self._block_hook is not None:
                self._block_hook(self, rows)
        if self.specs["MH"]:
            start_MH = time.time()
            self.time["warmup"] = (start_MH - start) / 60.0
            pw = self.specs["post_warmup"]
            self.log(f"Warmup done, sampling {pw} with MH for inference", verbosity=1)
            # a sampler resumed from a saved engine state (load_sampler) continues the tail where the save left it
            done = int(self.state.get("post_warmup_done", 0)) if self.specs.get("save_engine_state") else 0
            if (hasattr(self._chain, "run_post_warmup") and done == 0 and self._block_hook is None and not self.specs["periodic_save"]
                    and not self.specs["save_all_samples"] and self.specs.get("engine_side_convergence", True) and pw > 0):
                self._post_warmup_on_engine(cc, pw)      # the tail as one engine call (bnmf_run_post_warmup)
                done = pw
                if self.specs.get("save_engine_state"):
                    self.state["post_warmup_done"] = done
            while done < pw:
                it = self.state["iter"]
                nxt = (it // cc["MAP_every"] + 1) * cc["MAP_every"]
                n = min(nxt - it, pw - done)
                rows = self._chain.run(n, converged=True)
                self._append_metrics(rows)
                self.state["iter"] = it + n
                done += n
                if self.specs.get("save_engine_state"):
                    self.state["post_warmup_done"] = done
                if self.state["iter"] % cc["MAP_every"] == 0 or done == pw:
                    self._check(final=(done == pw))
                    if self.specs["periodic_save"]:
                        self.save_object()
                if self._block_hook is not None:
                    self._block_hook(self, rows)
            self.log(f"Additional {pw} MH samples done", verbosity=1)
            self.time["MH"] = (time.time() - start_MH) / 60.0
        else:
            self.get_MAP(final=True)
            self.log("Final MAP computed", verbosity=1)
        self._log_mixing()
        self._log_relabelling()
        self._sync_state()
        self.log("Sampler done", verbosity=1)
        self.time["total"] = (time.time() - start) / 60.0
        self.time["per_iter"] = self.time["total"] / self.state["iter"]
        self.log(f"Total time: {round(self.time['total'], 2)} minutes", verbosity=1)
        self.log("Saving final object", verbosity=1)
        self.save_object()
        return self

    def _cc_state(self):
        """state$prev_MAP_metric ... as the C-ABI's bnmf_convergence_state."""
        from .engine import BnmfConvergenceState, WHY
        st = BnmfConvergenceState()
        have = "prev_MAP_metric" in self.state
        st.have_prev = 1 if have else 0
        if have:
            st.prev_MAP_metric = self.state["prev_MAP_metric"]; st.best_MAP_metric = self.state["best_MAP_metric"]
            st.prev_percent_change = self.state.get("prev_percent_change", float("nan"))
            st.inarow_na = int(self.state.get("inarow_na", 0)); st.inarow_no_change = int(self.state.get("inarow_no_change", 0))
            st.inarow_no_best = int(self.state.get("inarow_no_best", 0)); st.best_iter = int(self.state.get("best_iter", 0) or 0)
        st.converged = 1 if self.state["converged"] else 0
        st.why = {v: k for k, v in WHY.items()}.get(self.state.get("why"), 0)
        return st

    def _absorb_map_rows(self, maps, cc):
        """state$MAP_metrics rows and the log lines of the MAP checks an engine-side loop has made."""
        names = ["iter", "RMSE", "KL", "loglikelihood", "logposterior", "n_params", "BIC", "rank", "MAP_A_counts", "mean_temp",
                 "P_mean_acceptance_rate", "E_mean_acceptance_rate"]
        flip = -1 if cc["metric"] in ("loglikelihood", "logposterior") else 1
        for r in maps:
            row = dict(zip(names, r[:12]))
            if not self.specs["MH"]:
                row.pop("P_mean_acceptance_rate"); row.pop("E_mean_acceptance_rate")
            df = pd.DataFrame([row])
            self.state["MAP_metrics"] = df if self.state["MAP_metrics"].empty else pd.concat([self.state["MAP_metrics"], df], ignore_index=True)
            m = flip * row[cc["metric"]]
            pcs = "NA" if np.isnan(r[12]) else f"{flip * round(r[12] * 100, 2)}"
            self.log(f"iter = {int(r[0])}", verbosity=1)
            self.state["indent"] = 2
            self.log("Computing MAP", verbosity=1)
            self.log("Checking convergence", verbosity=1)
            self.log(f"{cc['metric']} = {round(m, 2)} | {pcs}% change | {int(r[13])} no change | {int(r[14])} no best | {int(r[15])} NA", verbosity=1)
            self.state["indent"] = 1

    def _absorb_cc_state(self, st):
        if st.have_prev:
            self.state.update(prev_MAP_metric=st.prev_MAP_metric, best_MAP_metric=st.best_MAP_metric,
                              prev_percent_change=st.prev_percent_change, inarow_na=st.inarow_na,
                              inarow_no_change=st.inarow_no_change, inarow_no_best=st.inarow_no_best)
            if st.best_iter:
                self.state["best_iter"] = st.best_iter
        from .engine import WHY
        if st.why in WHY and WHY[st.why] is not None:      # check_convergence_ keeps updating `why` during the post-warm-up checks too
            self.state["why"] = WHY[st.why]

    def _post_warmup_on_engine(self, cc, pw):
        """The MH models' post-warm-up iterations (R/bayesNMF_sampler.R:332-384) as one engine call; the final MAP (kept
        signatures, credible intervals) is then taken from the device window as after the reference's last check."""
        # The reference's LAST check is get_MAP(final = TRUE) + check_convergence(final = TRUE): MAP metrics AND convergence bookkeeping on
        # the KEPT signatures (R/bayesNMF_sampler.R:364-375).  The engine's checks are over all N (bnmf_map), which is what every check
        # but the last wants — so the engine runs up to the last regular check before the end, the rest of the iterations are one plain
        # bnmf_run, and the final check is made here, exactly as the reference makes it (rounds 3-4 rebuilt the last
        # MAP-metrics row but kept the all-N bookkeeping).
        me = cc["MAP_every"]
        it0 = int(self.state["iter"])
        end = it0 + int(pw)
        n1 = max(((end - 1) // me) * me - it0, 0)
        if n1 > 0:
            rows, maps, st = self._chain.run_post_warmup(cc, self._cc_state(), n1)
            if len(rows):
                self._append_metrics(rows)
                self.state["iter"] = int(rows[-1, 0])
            self._absorb_map_rows(maps, cc)
            self._absorb_cc_state(st)
        n2 = end - int(self.state["iter"])
        if n2 > 0:
            self._append_metrics(self._chain.run(n2, converged=True))
            self.state["iter"] = end
        self._check(final=True)

    def _run_until_on_engine(self, cc):
        """The warm-up loop (blocks, MAP, MAP metrics, convergence bookkeeping) as one engine call;
        the R6-style state, both metric tables and the log lines are rebuilt from what it returns."""
        from .engine import WHY
        rows, maps, st = self._chain.run_until(cc)
        if len(rows):
            self._append_metrics(rows)
            self.state["iter"] = int(rows[-1, 0])
        self._absorb_map_rows(maps, cc)
        self._absorb_cc_state(st)
        if st.converged:
            self.state["converged"] = True
            self.state["why"] = WHY[st.why]
            self.state["converged_iter"] = self.state["iter"]
            self.log(f"Converged at {self.state['iter']} due to {self.state['why']}", verbosity=1)

    def assign_signatures_ensemble(self, reference_P, reference_names=None, idxs="MAP_idx", credible_interval=0.95):
        """assign_signatures_ensemble_ (R/postprocessing.R:175-341): every posterior sample of the MAP window (or of the recorded
        iterations `idxs`) votes, with its cosine similarity as weight, for the Hungarian assignment of its included signatures to
        the reference catalogue `reference_P` (K x R matrix; the reference's default is its bundled COSMIC v3.3.1 SBS table).
        Returns dict(assignments, votes) (data frames with the reference's columns) and stores them in
        self.reference_comparison (fields reference_P, idxs, keep_sigs, assignments, votes)."""
        ref = np.asarray(reference_P, dtype=float)
        if ref.shape[0] != self.dims["K"]:
            raise ValueError(f"Reference matrix has {ref.shape[0]} rows, but data has {self.dims['K']} rows.")
        names = list(reference_names) if reference_names is not None else list(range(1, ref.shape[1] + 1))
        cc = self.specs["convergence_control"]
        n = min(cc["MAP_over"], self.state["iter"])
        first_iter = self.state["iter"] - n + 1
        idx = self.MAP["idx"] if isinstance(idxs, str) else list(idxs)
        ia = np.asarray(idx, dtype=int)
        lo, hi = self._kept_range()
        if ia.size and (ia.min() < lo or ia.max() > hi):
            raise ValueError(f"idxs must be recorded iterations that are still kept: {lo}..{hi}")
        at = None
        if ia.size and ia.min() < first_iter:          # past the last window: the samples min(idxs) ... max(idxs) (bnmf_assign_at)
            at, first_iter = int(ia.max()), int(ia.min())
            n = at - first_iter + 1
        used = np.zeros(n, dtype=np.int32)
        used[ia - first_iter] = 1
        N = self.dims["N"]
        A = np.ravel(self.MAP["A"])
        if len(self.MAP["keep_sigs"]) == N and (A == 0).any():      # get_MAP(final = FALSE): only included signatures
            keep_sigs = np.where(A == 1)[0]
            self.MAP["sig_idx"] = keep_sigs
        else:
            keep_sigs = np.asarray(self.MAP["keep_sigs"])
            self.MAP["sig_idx"] = np.arange(len(keep_sigs))
        keep = np.zeros(N, dtype=np.int32); keep[keep_sigs] = 1
        MAP_full = np.zeros((self.dims["K"], N)); MAP_full[:, keep_sigs] = np.asarray(self.MAP["P"])[:, self.MAP["sig_idx"]]
        kw = {} if at is None else dict(end_iter=at)
        r = self._chain.assign(n, ref, used=used, keep=keep, MAP_P=MAP_full, credible_interval=credible_interval, **kw)
        rows = []
        for i in keep_sigs:
            tot = r["votes"][i].sum()
            for j in np.argsort(-r["votes"][i], kind="stable"):
                if r["votes"][i, j] > 0:
                    rows.append(dict(sig_est=int(i) + 1, sig_ref=names[j], prop_votes=r["votes"][i, j] / tot))
        votes = pd.DataFrame(rows, columns=["sig_est", "sig_ref", "prop_votes"])
        assignments = pd.DataFrame([dict(sig_est=int(i) + 1, sig_ref=names[r["assigned"][i]], MAP_cosine=r["MAP_cosine"][i],
                                         lower_cosine=r["lower_cosine"][i], upper_cosine=r["upper_cosine"][i]) for i in keep_sigs])
        self.reference_comparison.update(reference_P=ref, idxs=idx, keep_sigs=keep_sigs, assignments=assignments, votes=votes)
        return dict(assignments=assignments, votes=votes)

    def get_WAIC(self, end_iter=None, n_samples=None, idx="MAP_idx", pointwise=False):
        """The Watanabe-Akaike criterion over recorded samples, on the device (bnmf_waic_at): over iterations end_iter - n_samples + 1
        ... end_iter (defaults as get_MAP: the last MAP_over samples), restricted to `idx` — "MAP_idx": those whose A equals the mode
        of the range, so that the samples are all of one rank; None: every sample of the range; else a vector of recorded iterations.
        Returns dict(n_used, n_high_var, lppd, p_waic, elpd_waic, waic, se_elpd, mean_loglik); with pointwise also the per-column
        and per-cell arrays (Engine.waic)."""
        if not hasattr(self._chain, "waic"):
            raise ValueError("get_WAIC needs an engine that computes WAIC over its recorded samples (waic); this engine_factory's cannot")
        n, used, _, kw = self._recorded_range(end_iter, n_samples, idx)
        return self._chain.waic(n, used=used, pointwise=pointwise, **kw)

    def get_PPC(self, end_iter=None, n_samples=None, idx="MAP_idx", pointwise=False):
        """Posterior predictive checks of the recorded samples, on the device (bnmf_ppc_at; not in the reference): over iterations
        end_iter - n_samples + 1 ... end_iter (defaults as get_WAIC: the last MAP_over samples), restricted to `idx` ("MAP_idx": those
        whose A equals the mode of the range; None: every sample; else a vector of recorded iterations), a replicate of the data is
        drawn from every sample's own fit and compared with the data through two discrepancies (Poisson: Freeman-Tukey and the number
        of zero cells; Normal: the sum of squared standardised residuals and the largest one).
        Returns dict(n_used, n_tail_cells, p_T1, p_T2, mean_T1_obs, mean_T1_rep, mean_T2_obs, mean_T2_rep; col: a data frame with one
        row per column of the data — T1_obs, T1_rep, p_T1, T2_obs, T2_rep, p_T2: a p_T1 near 0 marks a column the model reconstructs
        worse than its own replicates; series: a data frame with one row per used sample — T1_obs, T1_rep, T2_obs, T2_rep over the
        whole matrix); with pointwise also mean_cell, var_cell, p_less_cell, p_equal_cell and pit = p_less + 0.5 p_equal (K x G)."""
        if not hasattr(self._chain, "ppc"):
            raise ValueError("get_PPC needs an engine that computes posterior predictive checks over its recorded samples (ppc); this engine_factory's cannot")
        n, used, _, kw = self._recorded_range(end_iter, n_samples, idx)
        r = self._chain.ppc(n, used=used, pointwise=pointwise, **kw)
        out = {k: r[k] for k in ("n_used", "n_tail_cells", "p_T1", "p_T2", "mean_T1_obs", "mean_T1_rep", "mean_T2_obs", "mean_T2_rep")}
        out["col"] = pd.DataFrame({k[:-4]: r[k] for k in ("T1_obs_col", "T1_rep_col", "p_T1_col", "T2_obs_col", "T2_rep_col", "p_T2_col")})
        out["series"] = pd.DataFrame({k: r[k] for k in ("T1_obs", "T1_rep", "T2_obs", "T2_rep")})
        if pointwise:
            out.update({k: r[k] for k in ("mean_cell", "var_cell", "p_less_cell", "p_equal_cell", "pit")})
        return out

    def get_attribution(self, end_iter=None, n_samples=None, idx="MAP_idx", min_load=1.0, credible_interval=0.95, prob=False):
        """Which signature produced the mutations of which tumour, on the device (bnmf_attribution_at; not in the reference): over
        iterations end_iter - n_samples + 1 ... end_iter (defaults as get_WAIC: the last MAP_over samples), restricted to `idx`
        ("MAP_idx": those whose A equals the mode of the range; None: every sample; else a vector of recorded iterations), every
        sample allocates the count of every cell to the factors in proportion to their parts of the fit.
        Returns dict(load_mean, load_sd, share, p_present: N x G arrays — the mean and standard deviation over the samples of the
        mutations of tumour g attributed to signature n, its mean share of the tumour, and the fraction of samples in which it
        carries at least min_load mutations; cohort: a data frame with one row per signature — the mean and the credible_interval
        bounds (quantile type 7) of its load over the whole cohort; n_used, n_present: the (n, g) with p_present >= 0.5, total: the
        mean load of the cohort); with prob also prob (K x N x G), the probability that a mutation of type k in tumour g came from
        signature n.  Factor n is taken to be the same signature in every sample, as get_MAP takes it."""
        if not hasattr(self._chain, "attribution"):
            raise ValueError("get_attribution needs an engine that computes the attribution over its recorded samples (attribution); this engine_factory's cannot")
        n, used, _, kw = self._recorded_range(end_iter, n_samples, idx)
        r = self._chain.attribution(n, used=used, min_load=min_load, prob=prob, **kw)
        ser = np.asarray(r["series"], dtype=float)
        a = (1.0 - float(credible_interval)) / 2.0
        out = dict(load_mean=r["load_mean"], load_sd=np.sqrt(r["load_var"]), share=r["share"], p_present=r["p_present"],
                   cohort=pd.DataFrame(dict(signature=np.arange(1, ser.shape[1] + 1), mean=ser.mean(axis=0),
                                            lower=np.quantile(ser, a, axis=0), upper=np.quantile(ser, 1.0 - a, axis=0))),
                   n_used=r["n_used"], n_present=r["n_present"], total=r["total"])
        if prob:
            out["prob"] = r["prob"]
        return out

    def get_projection(self, new_data, end_iter=None, n_samples=None, idx="MAP_idx", n_steps=200, min_load=1.0, credible_interval=0.95):
        """Exposures of new tumours under the recorded signatures, on the device (bnmf_project_at; not in the reference): new_data is
        a K x J matrix of counts (or other non-negative values) of tumours the chain has not seen — a validation cohort, one patient,
        a bootstrap.  Over iterations end_iter - n_samples + 1 ... end_iter (defaults as get_WAIC: the last MAP_over samples),
        restricted to `idx` ("MAP_idx": those whose A equals the mode of the range; None: every sample; else a vector of recorded
        iterations), every column is refitted to every sample's renormalised signatures by n_steps steps of the KL multiplicative
        update, so the uncertainty of the signatures reaches the exposures.
        Returns dict(exposure_mean, exposure_sd, share, p_present, lower, upper: N x J arrays — the mean and standard deviation over
        the samples of the exposure of tumour j to signature n, its mean share of the tumour, the fraction of samples in which it
        carries at least min_load mutations, and the credible_interval bounds (quantile type 7, computed here from the per-sample
        exposures); fit: a data frame with one row per new tumour — cosine, rel_l1 (the means over the samples of the cosine and the
        relative L1 error of the fit) and max_rel_change (how far the last step still moved the exposures, relative to the tumour's
        total); n_used, n_steps, n_present, total, max_rel_change, min_cosine, min_cosine_at).  n_steps = 200 is a convention;
        max_rel_change is how to judge it.  Factor n is taken to be the same signature in every sample, as get_MAP takes it."""
        if not hasattr(self._chain, "project"):
            raise ValueError("get_projection needs an engine that refits new data to its recorded samples (project); this engine_factory's cannot")
        n, used, _, kw = self._recorded_range(end_iter, n_samples, idx)
        r = self._chain.project(n, np.asarray(new_data, dtype=float), used=used, n_steps=n_steps, min_load=min_load, exposures=True, **kw)
        ex = np.asarray(r["exposures"], dtype=float)
        a = (1.0 - float(credible_interval)) / 2.0
        out = dict(exposure_mean=r["load_mean"], exposure_sd=np.sqrt(r["load_var"]), share=r["share"], p_present=r["p_present"],
                   lower=np.quantile(ex, a, axis=0), upper=np.quantile(ex, 1.0 - a, axis=0),
                   fit=pd.DataFrame(dict(cosine=r["cosine"], rel_l1=r["rel_l1"], max_rel_change=r["rel_change"])))
        out.update({k: r[k] for k in ("n_used", "n_steps", "n_present", "total", "max_rel_change", "min_cosine", "min_cosine_at")})
        self.log(f"Projection: J = {ex.shape[2]}, {r['n_steps']} steps, max_rel_change {r['max_rel_change']:.3g}, min_cosine {r['min_cosine']:.4f}", verbosity=1)
        return out

    def get_decomposition(self, reference_P, end_iter=None, n_samples=None, idx="MAP_idx", n_steps=200, min_share=0.05, keep=None,
                          credible_interval=0.95, reference_names=None):
        """Is a discovered signature a mixture of known ones?  On the device (bnmf_decompose_at; not in the reference): reference_P is
        a K x R catalogue (a data frame's column names become the reference names unless reference_names is given).  Over iterations
        end_iter - n_samples + 1 ... end_iter (defaults as get_WAIC: the last MAP_over samples), restricted to `idx` ("MAP_idx": those
        whose A equals the mode of the range, so that the samples are all of one rank pattern — a sample that excludes a factor enters
        its means with 0; None: every sample; else a vector of recorded iterations), every renormalised column of every sample's P is
        refitted to the normalised catalogue by n_steps steps of the KL multiplicative update, the references below min_share of the
        column are dropped, and n_steps more steps refit the rest: the uncertainty of the signatures reaches the mixture weights.
        keep: the factors to decompose (0 / 1 flags of length N; None = all).
        Returns dict(weight_mean, weight_sd, share, p_present, lower, upper: R x N arrays — the mean and standard deviation over the
        samples of the weight of reference r in signature n (a signature's weights sum to 1), its mean share, the fraction of samples
        in which it holds at least min_share, and the credible_interval bounds (quantile type 7, computed here from the per-sample
        weights); fit: a data frame with one row per signature — cosine, rel_l1 (the means over the samples of the cosine and the
        relative L1 error of the mixture) and max_rel_change; nactive (S x N), included (N); components: per signature the list of
        (reference, p_present, weight_mean) with p_present >= 0.5, the largest weight first, the reference by name when names are
        known, else by 0-based column; n_used, n_steps, R, n_present, min_share, max_rel_change, min_cosine, min_cosine_at)."""
        if not hasattr(self._chain, "decompose"):
            raise ValueError("get_decomposition needs an engine that decomposes its recorded samples into a catalogue (decompose); this engine_factory's cannot")
        if reference_names is None and hasattr(reference_P, "columns"):
            reference_names = [str(c) for c in reference_P.columns]
        ref = np.asarray(reference_P, dtype=float)
        if reference_names is not None and len(reference_names) != ref.shape[1]:
            raise ValueError(f"reference_names has {len(reference_names)} entries for {ref.shape[1]} references")
        n, used, _, kw = self._recorded_range(end_iter, n_samples, idx)
        r = self._chain.decompose(n, ref, used=used, keep=keep, n_steps=n_steps, min_share=min_share, weights=True, **kw)
        ws = np.asarray(r["weights"], dtype=float)
        a = (1.0 - float(credible_interval)) / 2.0
        out = dict(weight_mean=r["weight_mean"], weight_sd=np.sqrt(r["weight_var"]), share=r["share"], p_present=r["p_present"],
                   lower=np.quantile(ws, a, axis=0), upper=np.quantile(ws, 1.0 - a, axis=0),
                   fit=pd.DataFrame(dict(cosine=r["cosine"], rel_l1=r["rel_l1"], max_rel_change=r["rel_change"])),
                   nactive=r["nactive"], included=r["included"])
        comp = []
        for j in range(ws.shape[2]):
            rs = [i for i in np.argsort(-r["weight_mean"][:, j], kind="stable") if r["p_present"][i, j] >= 0.5]
            comp.append([(reference_names[i] if reference_names is not None else int(i), float(r["p_present"][i, j]), float(r["weight_mean"][i, j])) for i in rs])
        out["components"] = comp
        out.update({k: r[k] for k in ("n_used", "n_steps", "R", "n_present", "min_share", "max_rel_change", "min_cosine", "min_cosine_at")})
        self.log(f"Decomposition: R = {r['R']}, {r['n_steps']} steps, min_share {r['min_share']:g}, min_cosine {r['min_cosine']:.4f}, "
                 f"max_rel_change {r['max_rel_change']:.3g}", verbosity=1)
        return out

    def get_contrast(self, groups, end_iter=None, n_samples=None, idx="MAP_idx", min_load=1.0, credible_interval=0.95, series=False):
        """Does the activity of a signature differ between groups of tumours?  On the device (bnmf_contrast_at; not in the reference):
        groups is a vector of G labels of any hashable kind, one per tumour (None / NaN: the tumour is left out); they are numbered
        0 .. C-1 in order of first appearance.  Over iterations end_iter - n_samples + 1 ... end_iter (defaults as get_WAIC: the last
        MAP_over samples), restricted to `idx` ("MAP_idx": those whose A equals the mode of the range; None: every sample; else a
        vector of recorded iterations), every sample gives one draw of each group's mean load of every signature (the renormalised
        exposure of get_MAP), mean share of the tumour's total and prevalence (the fraction of the group's tumours in which the
        signature carries at least min_load mutations); the difference of two groups then has a posterior of its own.
        Returns dict(names: the C group names, pair_names: the NP pairs (a, b) of names, a before b; per statistic "load", "share",
        "prevalence" a dict(mean, var, lower, upper: N x C arrays over the samples, quantile type 7 at credible_interval;
        diff_mean, diff_var, diff_lower, diff_upper, p_greater, p_less: N x NP arrays of the difference a - b); sizes (C),
        n_used, n_groups, n_pairs, n_left_out, n_credible: per statistic the (signature, pair) whose interval excludes 0, min_load,
        credible_interval); with series also series (3 x S x N x C), every sample's values.  Factor n is taken to be the same signature in
        every sample, as get_MAP takes it; no multiple-testing adjustment is made."""
        if not hasattr(self._chain, "contrast"):
            raise ValueError("get_contrast needs an engine that contrasts groups over its recorded samples (contrast); this engine_factory's cannot")
        labels, names = contrast_labels(groups, self.dims["G"])
        n, used, _, kw = self._recorded_range(end_iter, n_samples, idx)
        r = self._chain.contrast(n, labels, used=used, min_load=min_load, credible_interval=credible_interval, series=series, **kw)
        out = dict(names=names, pair_names=[(names[a], names[b]) for a, b in r["pairs"]])
        for q, stat in enumerate(("load", "share", "prevalence")):
            out[stat] = dict(zip(("mean", "var", "lower", "upper"), r["group"][q]))
            out[stat].update(zip(("diff_mean", "diff_var", "diff_lower", "diff_upper", "p_greater", "p_less"), r["pair"][q]))
        out.update({k: r[k] for k in ("sizes", "n_used", "n_groups", "n_pairs", "n_left_out", "n_credible", "min_load", "credible_interval")})
        if series:
            out["series"] = r["series"]
        self.log(f"Contrast: groups {', '.join(f'{nm} ({int(m)})' for nm, m in zip(names, r['sizes']))}; {r['n_pairs']} pair"
                 f"{'' if r['n_pairs'] == 1 else 's'} {', '.join(f'{a} - {b}' for a, b in out['pair_names'])}; n_credible load {r['n_credible'][0]}, "
                 f"share {r['n_credible'][1]}, prevalence {r['n_credible'][2]}", verbosity=1)
        return out

    def get_regression(self, covariates, end_iter=None, n_samples=None, idx="MAP_idx", intercept=True, standardize=False, credible_interval=0.95,
                       series=False):
        """Does the activity of a signature follow a covariate of the tumours (age, dose, purity), and is a group difference still
        there once other covariates are in the model?  On the device (bnmf_regress_at; not in the reference): covariates is a G x Q0
        array or a mapping name -> column of G values (a data frame); a tumour with a None / NaN is left out; intercept prepends the
        column of ones; standardize centres and scales the other columns by the included tumours' mean and standard deviation.  Over
        iterations end_iter - n_samples + 1 ... end_iter (defaults as get_WAIC), restricted to `idx` (as get_contrast), every sample
        gives one least-squares fit per signature of its load (the renormalised exposure of get_MAP), of its share of the tumour's total
        and of the square root of its load on the design: the coefficients over the samples are draws from the posterior of the
        cohort's own coefficient (the tumours' sampling error as a sample of a population is not added).
        Returns dict(names: the Q column names; per response "load", "share", "sqrt_load" a dict(mean, var, lower, upper, p_greater,
        p_less: N x Q arrays over the samples, quantile type 7 at credible_interval; r2_mean, r2_lower, r2_upper, r2_samples,
        sigma2_mean: N); include (G flags, None = all), n_used, Q, n_included, n_left_out, n_blocks, min_pivot_ratio, min_pivot_at (how
        close to collinear the design is), n_credible (3 x Q: the signatures whose interval for a column excludes 0),
        credible_interval); with series also coef_series (3 x S x N x Q) and r2_series (3 x S x N).  No multiple-testing adjustment."""
        if not hasattr(self._chain, "regress"):
            raise ValueError("get_regression needs an engine that regresses over its recorded samples (regress); this engine_factory's cannot")
        design, include, names = regression_design(covariates, self.dims["G"], intercept=intercept, standardize=standardize)
        n, used, _, kw = self._recorded_range(end_iter, n_samples, idx)
        r = self._chain.regress(n, design, include=include, used=used, credible_interval=credible_interval, series=series, **kw)
        out = dict(names=names, include=include)
        for q, stat in enumerate(("load", "share", "sqrt_load")):
            out[stat] = dict(zip(("mean", "var", "lower", "upper", "p_greater", "p_less"), r["coef"][q]))
            out[stat].update(zip(("r2_mean", "r2_lower", "r2_upper", "r2_samples", "sigma2_mean"), r["fit"][q]))
        out.update({k: r[k] for k in ("n_used", "Q", "n_included", "n_left_out", "n_blocks", "min_pivot_ratio", "min_pivot_at", "n_credible",
                                      "credible_interval")})
        if series:
            out.update(coef_series=r["coef_series"], r2_series=r["r2_series"])
        self.log(f"Regression: {r['n_included']} tumours included, {r['n_left_out']} left out; Q = {r['Q']}, min_pivot_ratio "
                 f"{r['min_pivot_ratio']:.3g} (column {names[r['min_pivot_at']]}); n_credible for the load "
                 f"{', '.join(f'{nm} {int(c)}' for nm, c in zip(names, r['n_credible'][0]))}", verbosity=1)
        return out

    def get_coactivity(self, include=None, min_load=1.0, credible_interval=0.95, series=False, end_iter=None, n_samples=None, idx="MAP_idx"):
        """Do two signatures act in the same tumours or exclude each other, and is a signature split into two factors (a high cosine of
        two columns of P whose exposures are negatively correlated)?  On the device (bnmf_coactivity_at; not in the reference): over
        iterations end_iter - n_samples + 1 ... end_iter (defaults as get_WAIC), restricted to `idx` (as get_contrast), every sample
        gives per pair of signatures the Pearson and the Spearman (midrank) correlation of their loads (the renormalised exposures of
        get_MAP) across the included tumours, the phi coefficient of their presence (load >= min_load) and the cosine of their two
        columns of P.  include (G flags; None = all): a tumour with a 0, None or NaN is left out, as get_regression leaves out a tumour
        with a missing covariate.
        Returns dict(per statistic "pearson", "spearman", "copresence", "cosine" a dict(mean, lower, upper, p_greater, n_valid: N x N
        symmetric matrices with a NaN diagonal, over the samples whose value is not NaN; quantile type 7 at credible_interval); pairs
        (the NP pairs (a, b)), pair (4 x 7 x NP: every row of the call), include, n_used, n_included, n_left_out, n_pairs, n_blocks,
        n_credible (per statistic but the cosine: the pairs whose interval excludes 0), max_cosine, max_cosine_at, min_load,
        credible_interval); with series also series (4 x S x NP).  No multiple-testing adjustment."""
        if not hasattr(self._chain, "coactivity"):
            raise ValueError("get_coactivity needs an engine that correlates over its recorded samples (coactivity); this engine_factory's cannot")
        G, N = self.dims["G"], self.dims["N"]
        inc = None
        if include is not None:
            vals = list(include.tolist()) if hasattr(include, "tolist") else list(include)
            v = np.array([np.nan if x is None or x is pd.NA else float(x) for x in vals], dtype=np.float64)
            if v.size != G:
                raise ValueError(f"include has {v.size} values for {G} tumours")
            if (~np.isnan(v) & (v != 0) & (v != 1)).any():
                raise ValueError("include holds a value other than 0, 1 and None / NaN")
            inc = (v == 1).astype(np.int32)
        n, used, _, kw = self._recorded_range(end_iter, n_samples, idx)
        r = self._chain.coactivity(n, include=inc, used=used, min_load=min_load, credible_interval=credible_interval, series=series, **kw)
        out = dict(pairs=r["pairs"], pair=r["pair"], include=inc)
        ia, ib = [a for a, _ in r["pairs"]], [b for _, b in r["pairs"]]
        for q, stat in enumerate(("pearson", "spearman", "copresence", "cosine")):
            out[stat] = {}
            for row, name in ((0, "mean"), (2, "lower"), (3, "upper"), (4, "p_greater"), (6, "n_valid")):
                mat = np.full((N, N), np.nan)
                mat[ia, ib] = mat[ib, ia] = r["pair"][q, row]
                out[stat][name] = mat
        out.update({k: r[k] for k in ("n_used", "n_included", "n_left_out", "n_pairs", "n_blocks", "n_credible", "max_cosine", "max_cosine_at",
                                      "min_load", "credible_interval")})
        if series:
            out["series"] = r["series"]
        at = r["max_cosine_at"]
        self.log(f"Co-activity: {r['n_included']} tumours included, {r['n_left_out']} left out; {r['n_pairs']} pairs, n_credible pearson "
                 f"{r['n_credible'][0]}, spearman {r['n_credible'][1]}, copresence {r['n_credible'][2]}; largest mean cosine "
                 f"{r['max_cosine']:.3g}" + (f" (pair {r['pairs'][at]})" if at >= 0 else ""), verbosity=1)
        return out

    def get_stability(self, end_iter=None, n_samples=None, relabel=True, extra_P=None, extra_label=None, idx="MAP_idx"):
        """Are the N signatures well-separated, reproducible objects?  On the device (bnmf_stability_at; not in the reference): over
        iterations end_iter - n_samples + 1 ... end_iter (defaults as get_WAIC), restricted to `idx` (as get_contrast), every recorded
        column of P is a point, the distance is the cosine distance and the cluster of a point is its factor; the silhouette of each
        point and the mean silhouette of each cluster (the "stability" of NMF-based extractors) follow.  With relabel the range is
        first aligned by get_relabelling() and every point's cluster is the label it received; an unmatched sample is left out.
        extra_P (K x X) with extra_label (X labels) adds further columns, e.g. the aligned samples of other chains.
        Returns dict(stability, min_silhouette, members, mean_a, mean_b, share_negative (length N), silhouette, a, b, nearest (S x N
        over the used samples; NaN / -1 where a point is left out), extra (4 x X: the same rows for the extra columns), between (N x
        N), medoid (K x N consensus signatures), medoid_at, n_used, n_points, n_extra, n_left_out, n_clusters, n_negative,
        mean_silhouette, min_stability, min_stability_at)."""
        if not hasattr(self._chain, "stability"):
            raise ValueError("get_stability needs an engine that takes distances over its recorded samples (stability); this engine_factory's cannot")
        N = self.dims["N"]
        n, used, _, kw = self._recorded_range(end_iter, n_samples, idx)
        labels = None
        if relabel:
            perm = np.asarray(self.get_relabelling(end_iter=end_iter, n_samples=n_samples, idx=idx)["perm"], dtype=np.int32)
            labels = np.full((n, N), -1, dtype=np.int32)                 # perm has a row per used sample: scattered into the range's rows
            labels[slice(None) if used is None else np.asarray(used) != 0] = perm
        r = self._chain.stability(n, labels=labels, used=used, extra_P=extra_P, extra_label=extra_label, **kw)
        S = r["n_used"]
        out = {name: r["factor"][i] for i, name in enumerate(("members", "stability", "min_silhouette", "mean_a", "mean_b", "share_negative"))}
        out.update({name: r["point"][i, :S * N].reshape(S, N) for i, name in enumerate(("silhouette", "a", "b", "nearest"))})
        out.update(extra=r["point"][:, S * N:], labels=labels, between=r["between"], medoid=r["medoid"], medoid_at=r["medoid_at"])
        out.update({k: r[k] for k in ("n_used", "n_points", "n_extra", "n_left_out", "n_clusters", "n_negative", "mean_silhouette", "min_stability",
                                      "min_stability_at")})
        self.log(f"Stability: {r['n_points']} points in {r['n_clusters']} clusters, {r['n_left_out']} left out; mean silhouette "
                 f"{r['mean_silhouette']:.3g}, least stable signature {r['min_stability_at']} at {r['min_stability']:.3g}, "
                 f"{r['n_negative']} points nearer to another cluster", verbosity=1)
        return out

    def get_reconstruction(self, end_iter=None, n_samples=None, idx="MAP_idx", min_cosine=0.9, min_drop=0.01):
        """How well is every tumour of the cohort reconstructed, and which signatures does it need?  On the device
        (bnmf_reconstruction_at; not in the reference): over iterations end_iter - n_samples + 1 ... end_iter (defaults as get_WAIC:
        the last MAP_over samples), restricted to `idx` ("MAP_idx": those whose A equals the mode of the range; None: every sample;
        else a vector of recorded iterations), every sample gives per tumour the cosine between its data and its fit, the relative L1
        error and the RMSE, and per signature the cosine of the fit without it.  The remaining exposures are not refitted after the
        removal, so the drop is an upper bound of what removing the signature costs the tumour.
        Returns dict(tumour (6 x G: the mean, variance and smallest value over the samples of the cosine, the mean relative L1 error,
        the mean RMSE, the fraction of samples with cosine >= min_cosine; NaN for an all-zero tumour) with its rows also as cosine,
        cosine_var, min_cosine_sample, rel_l1, rmse, p_good; drop (4 x N x G: the mean and variance of the drop, the mean
        leave-one-out cosine, the fraction of samples with drop >= min_drop: the probability that the tumour needs the signature)
        with its rows as drop_mean, drop_var, loo_cosine, p_needed; series (S: the cohort's mean cosine per used sample); signature
        (3 x N: the tumours that need the signature, the mean and the largest mean drop); n_used, n_undefined, n_poor, n_needed,
        min_cosine, min_drop, worst_cosine, worst_at)."""
        if not hasattr(self._chain, "reconstruction"):
            raise ValueError("get_reconstruction needs an engine that computes the fit over its recorded samples (reconstruction); this engine_factory's cannot")
        n, used, _, kw = self._recorded_range(end_iter, n_samples, idx)
        r = self._chain.reconstruction(n, used=used, min_cosine=min_cosine, min_drop=min_drop, **kw)
        G, N = self.dims["G"], self.dims["N"]
        tum, drop = np.asarray(r["tumour"]).reshape(6, G), np.asarray(r["drop"]).reshape(4, N, G)
        out = dict(tumour=tum, drop=drop, series=np.asarray(r["series"]).reshape(-1), signature=np.asarray(r["signature"]).reshape(3, N))
        out.update({name: tum[i] for i, name in enumerate(("cosine", "cosine_var", "min_cosine_sample", "rel_l1", "rmse", "p_good"))})
        out.update({name: drop[i] for i, name in enumerate(("drop_mean", "drop_var", "loo_cosine", "p_needed"))})
        out.update({k: r[k] for k in ("n_used", "n_undefined", "n_poor", "n_needed", "min_cosine", "min_drop", "worst_cosine", "worst_at")})
        self.log(f"Reconstruction: {r['n_poor']} of {G - r['n_undefined']} tumours below cosine {r['min_cosine']:g}, worst {r['worst_cosine']:.3g} "
                 f"(tumour {r['worst_at']}); {r['n_needed']} (signature, tumour) pairs with a drop >= {r['min_drop']:g}", verbosity=1)
        return out

    def get_similarity(self, include=None, query=None, top_k=10, min_cosine=0.9, end_iter=None, n_samples=None, idx="MAP_idx"):
        """Which tumours have the exposure profile of this one, does the cohort fall into subtypes, which tumours resemble nobody?  On
        the device (bnmf_similarity_at; not in the reference): over iterations end_iter - n_samples + 1 ... end_iter (defaults as
        get_WAIC), restricted to `idx` (as get_contrast), every sample gives for every pair of included tumours the cosine of their
        renormalised exposure vectors (the loads of get_MAP).  The cosine is a sum over the factors, so label switching does not touch
        it.  include (G flags; None = all): a tumour with a 0, None or NaN is left out, as in get_coactivity.  query: tumours (indices,
        or names where the data had column names) whose similarity to every tumour is returned in full.
        Returns dict(neighbours (a data frame: tumour, rank (1 = nearest), neighbour, mean, sd, p_similar: per included tumour the top_k
        others with the largest mean cosine; p_similar is the share of samples with cosine >= min_cosine), dense (3 x Q x G: mean,
        variance and p_similar of every query against every tumour, NaN on itself and on left-out tumours) with query, tumours (a
        data frame: tumour, typicality (the mean over the other tumours of the mean cosine), nearest_mean, degree (the other tumours
        with p_similar >= 0.5), included), neighbour_at, neighbour, tumour (the arrays of the call), n_used, n_included, n_left_out,
        top_k, n_query, n_pairs, n_similar_pairs, n_isolated, mean_similarity, least_typical, least_typical_at, min_cosine)."""
        if not hasattr(self._chain, "similarity"):
            raise ValueError("get_similarity needs an engine that compares tumours over its recorded samples (similarity); this engine_factory's cannot")
        G = self.dims["G"]
        names = self.tumour_names if getattr(self, "tumour_names", None) else None
        inc = None
        if include is not None:
            vals = list(include.tolist()) if hasattr(include, "tolist") else list(include)
            v = np.array([np.nan if x is None or x is pd.NA else float(x) for x in vals], dtype=np.float64)
            if v.size != G:
                raise ValueError(f"include has {v.size} values for {G} tumours")
            if (~np.isnan(v) & (v != 0) & (v != 1)).any():
                raise ValueError("include holds a value other than 0, 1 and None / NaN")
            inc = (v == 1).astype(np.int32)
        qv = None
        if query is not None:
            qs = list(np.atleast_1d(query).tolist())
            if names is not None and all(isinstance(q, str) for q in qs):
                missing = [q for q in qs if q not in names]
                if missing:
                    raise ValueError(f"query names no tumour of the data: {missing[:5]}")
                qs = [names.index(q) for q in qs]
            qv = np.asarray(qs, dtype=np.int32)
        n, used, _, kw = self._recorded_range(end_iter, n_samples, idx)
        r = self._chain.similarity(n, include=inc, query=qv, top_k=top_k, min_cosine=min_cosine, used=used, **kw)
        label = (lambda g: names[g]) if names is not None else (lambda g: int(g))
        k = int(r["top_k"])
        nat = np.asarray(r["neighbour_at"]).reshape(G, k) if k > 0 else np.empty((G, 0), dtype=np.int32)
        nb = np.asarray(r["neighbour"]).reshape(3, G, k) if k > 0 else np.empty((3, G, 0))
        rows = [(label(g), j + 1, label(nat[g, j]), nb[0, g, j], float(np.sqrt(nb[1, g, j])), nb[2, g, j])
                for g in range(G) for j in range(k) if nat[g, j] >= 0]
        out = dict(neighbours=pd.DataFrame(rows, columns=["tumour", "rank", "neighbour", "mean", "sd", "p_similar"]), neighbour_at=nat, neighbour=nb)
        tum = np.asarray(r["tumour"]).reshape(3, G)
        included = np.ones(G, dtype=bool) if inc is None else inc.astype(bool)
        out["tumour"] = tum
        out["tumours"] = pd.DataFrame(dict(tumour=[label(g) for g in range(G)], typicality=tum[0], nearest_mean=tum[1], degree=tum[2], included=included))
        if qv is not None:
            out.update(dense=np.asarray(r["dense"]).reshape(3, qv.size, G), query=[label(g) for g in qv])
        out.update({key: r[key] for key in ("n_used", "n_included", "n_left_out", "top_k", "n_query", "n_pairs", "n_similar_pairs", "n_isolated",
                                            "mean_similarity", "least_typical", "least_typical_at", "min_cosine")})
        self.log(f"Similarity: {r['n_included']} tumours included, {r['n_left_out']} left out; {r['n_similar_pairs']} of {r['n_pairs']} pairs similar "
                 f"(cosine >= {r['min_cosine']:g} in at least half of the samples), {r['n_isolated']} tumours resemble nobody; mean similarity "
                 f"{r['mean_similarity']:.3g}, least typical {r['least_typical']:.3g} (tumour {r['least_typical_at']})", verbosity=1)
        return out

    def get_subtypes(self, n_subtypes=None, centres=None, seeds=None, include=None, query=None, relabel=True, n_steps=50, min_certainty=0.9,
                     end_iter=None, n_samples=None, idx="MAP_idx", labels=False):
        """Does the cohort fall into subtypes, and how certain is the grouping?  On the device (bnmf_subtypes_at; not in the reference):
        over iterations end_iter - n_samples + 1 ... end_iter (defaults as get_WAIC), restricted to `idx` (as get_contrast), every
        sample's share profiles (each tumour's renormalised exposures divided by their sum) are clustered by at most n_steps Lloyd steps
        from one common start, so subtype c means the same in every sample; a tumour's membership of c is the share of samples in which
        it carries label c.  With relabel the range is first aligned by get_relabelling() and its perm is handed on; an unmatched
        sample is left out.  The start: centres (N x C share profiles), or seeds (C tumours, indices or names: their posterior-mean
        share profiles), or n_subtypes alone: seeds chosen by a deterministic farthest-first walk over the posterior-mean share profiles
        (subtype_seeds).  include and query as in get_similarity.
        Returns dict(tumours (a data frame: tumour, label, certainty, runner_up, assigned, included, membership_0 ...), subtypes (a data
        frame: subtype, size, size_sd, size_lower, size_upper), centres (a data frame: subtype, factor, mean, sd, lower, upper),
        consensus (a data frame: query, tumour, together; only with query), centres0, seeds, membership, label, tumour, centre, size,
        series, together, labels (the arrays of the call) and its info fields)."""
        if not hasattr(self._chain, "subtypes"):
            raise ValueError("get_subtypes needs an engine that clusters tumours over its recorded samples (subtypes); this engine_factory's cannot")
        G, N = self.dims["G"], self.dims["N"]
        names = self.tumour_names if getattr(self, "tumour_names", None) else None

        def tumours(v, what):
            vs = list(np.atleast_1d(v).tolist())
            if names is not None and all(isinstance(q, str) for q in vs):
                missing = [q for q in vs if q not in names]
                if missing:
                    raise ValueError(f"{what} names no tumour of the data: {missing[:5]}")
                vs = [names.index(q) for q in vs]
            return np.asarray(vs, dtype=np.int32)

        inc = None
        if include is not None:
            vals = list(include.tolist()) if hasattr(include, "tolist") else list(include)
            v = np.array([np.nan if x is None or x is pd.NA else float(x) for x in vals], dtype=np.float64)
            if v.size != G:
                raise ValueError(f"include has {v.size} values for {G} tumours")
            if (~np.isnan(v) & (v != 0) & (v != 1)).any():
                raise ValueError("include holds a value other than 0, 1 and None / NaN")
            inc = (v == 1).astype(np.int32)
        qv = None if query is None else tumours(query, "query")
        n, used, _, kw = self._recorded_range(end_iter, n_samples, idx)
        perm = None
        if relabel:
            rows = np.asarray(self.get_relabelling(end_iter=end_iter, n_samples=n_samples, idx=idx)["perm"], dtype=np.int32)
            perm = np.full((n, N), -1, dtype=np.int32)                   # perm has a row per used sample: scattered into the range's rows
            perm[slice(None) if used is None else np.asarray(used) != 0] = rows
        seed_at = None
        if centres is not None:
            c0 = np.asarray(centres, dtype=np.float64)
            if c0.ndim != 2 or c0.shape[0] != N:
                raise ValueError(f"centres is {c0.shape}, but a start is N = {N} rows by C columns")
        else:
            if seeds is None and n_subtypes is None:
                raise ValueError("get_subtypes needs one of n_subtypes, centres and seeds")
            prof = self._mean_share_profiles(n, used, perm, kw)
            member = np.ones(G, dtype=bool) if inc is None else inc.astype(bool)
            seed_at = tumours(seeds, "seeds") if seeds is not None else subtype_seeds(prof, int(n_subtypes), member)
            if (~member[seed_at]).any():
                raise ValueError("a seed is a tumour that include leaves out")
            c0 = prof[:, seed_at]
        if n_subtypes is not None and c0.shape[1] != int(n_subtypes):
            raise ValueError(f"n_subtypes = {n_subtypes}, but the start has {c0.shape[1]} columns")
        r = self._chain.subtypes(n, c0, include=inc, perm=perm, n_steps=n_steps, query=qv, min_certainty=min_certainty, used=used, labels=labels, **kw)
        label = (lambda g: names[g]) if names is not None else (lambda g: int(g))
        Cn = int(r["C"])
        tum, mem = np.asarray(r["tumour"]).reshape(3, G), np.asarray(r["membership"]).reshape(Cn, G)
        included = np.ones(G, dtype=bool) if inc is None else inc.astype(bool)
        frame = dict(tumour=[label(g) for g in range(G)], label=np.asarray(r["label"]), certainty=tum[0], runner_up=tum[2], assigned=tum[1], included=included)
        frame.update({f"membership_{c}": mem[c] for c in range(Cn)})
        size, cen = np.asarray(r["size"]).reshape(4, Cn), np.asarray(r["centre"]).reshape(4, N, Cn)
        out = dict(r)
        out.update(tumours=pd.DataFrame(frame),
                   subtypes=pd.DataFrame(dict(subtype=np.arange(Cn), size=size[0], size_sd=np.sqrt(size[1]), size_lower=size[2], size_upper=size[3])),
                   centres=pd.DataFrame([(c, j, cen[0, j, c], float(np.sqrt(cen[1, j, c])), cen[2, j, c], cen[3, j, c]) for c in range(Cn) for j in range(N)],
                                        columns=["subtype", "factor", "mean", "sd", "lower", "upper"]),
                   centres0=np.asarray(c0), seeds=None if seed_at is None else [label(g) for g in seed_at])
        if qv is not None:
            tog = np.asarray(r["together"]).reshape(qv.size, G)
            out["consensus"] = pd.DataFrame([(label(g), label(t), tog[i, t]) for i, g in enumerate(qv) for t in range(G)], columns=["query", "tumour", "together"])
            out["query"] = [label(g) for g in qv]
        self.log(f"Subtypes: {Cn} subtypes of {r['n_included']} tumours over {r['n_matched']} samples ({r['n_unmatched']} unmatched, {r['n_not_converged']} not "
                 f"converged in {r['n_steps']} steps); {r['n_certain']} tumours with certainty >= {r['min_certainty']:g}, mean certainty "
                 f"{r['mean_certainty']:.3g}, least certain {r['least_certain']:.3g} (tumour {r['least_certain_at']}); smallest subtype "
                 f"{r['smallest_subtype_at']} with {r['smallest_subtype']:.3g} tumours", verbosity=1)
        return out

    def get_residuals(self, include=None, n_steps=100, max_dispersion=2.0, reference_P=None, end_iter=None, n_samples=None, idx="MAP_idx"):
        """What does the model leave unexplained: is there a process in the leftovers?  On the device (bnmf_residuals_at; not in the
        reference): over iterations end_iter - n_samples + 1 ... end_iter (defaults as get_WAIC), restricted to `idx` (as get_contrast),
        every sample's standardised residuals, their second-moment matrix over the included tumours along the mutation types, its leading
        component (n_steps power steps) and every tumour's score on it.  A direction that the misfits of many tumours share is what a
        missing signature looks like: a rank that is too low.  include as in get_similarity.  max_dispersion = 2.0 is a reporting
        convention like min_cosine = 0.9 (it only sets the count n_overdispersed), not a test.
        Returns dict(types (a data frame: type, bias, bias_sd, p_positive, dispersion, dispersion_sd, component, component_mean,
        component_sd), tumours (a data frame: tumour, score, score_sd, chi, included), candidate (K: the positive part of the mean
        matrix's component, or of its negative where that part has the larger sum of squares, normalised to sum 1),
        candidate_cosine (N: with the columns of the range's mean renormalised P); with reference_P (K x R, a data frame's columns name
        the signatures) reference_cosine (R), best_reference and best_reference_cosine; gram, type, component, tumour, series (the arrays
        of the call) and its info fields)."""
        if not hasattr(self._chain, "residuals"):
            raise ValueError("get_residuals needs an engine that forms residuals over its recorded samples (residuals); this engine_factory's cannot")
        K, G, N = self.dims["K"], self.dims["G"], self.dims["N"]
        inc = None
        if include is not None:
            vals = list(include.tolist()) if hasattr(include, "tolist") else list(include)
            v = np.array([np.nan if x is None or x is pd.NA else float(x) for x in vals], dtype=np.float64)
            if v.size != G:
                raise ValueError(f"include has {v.size} values for {G} tumours")
            if (~np.isnan(v) & (v != 0) & (v != 1)).any():
                raise ValueError("include holds a value other than 0, 1 and None / NaN")
            inc = (v == 1).astype(np.int32)
        n, used, _, kw = self._recorded_range(end_iter, n_samples, idx)
        r = self._chain.residuals(n, include=inc, n_steps=n_steps, max_dispersion=max_dispersion, used=used, **kw)
        out = dict(r)
        typ, comp, tum = np.asarray(r["type"]).reshape(5, K), np.asarray(r["component"]).reshape(4, K), np.asarray(r["tumour"]).reshape(3, G)
        out["candidate"] = cand = residual_candidate(comp[0])

        def cosines(cols):
            den = np.sqrt((cols * cols).sum(axis=0) * (cand * cand).sum())
            return np.where(den > 0, (cols * cand[:, None]).sum(axis=0) / np.where(den > 0, den, 1.0), np.nan)

        it = self.state["iter"]
        back = it - (kw.get("end_iter", it) - n + 1) + 1
        Ps = [np.asarray(p, dtype=float) for s, p in enumerate(self._chain.window("P", back)[:n]) if used is None or used[s]]
        Pm = np.mean([p / np.where(p.sum(axis=0) > 0, p.sum(axis=0), 1.0) for p in Ps], axis=0)
        out["candidate_cosine"] = cosines(Pm)
        if reference_P is not None:
            ref = np.asarray(reference_P, dtype=np.float64)
            if ref.ndim != 2 or ref.shape[0] != K:
                raise ValueError(f"reference_P is {ref.shape}, but a catalogue has K = {K} rows")
            rc = cosines(ref)
            best = int(np.nanargmax(rc)) if not np.isnan(rc).all() else -1
            cols = list(reference_P.columns) if hasattr(reference_P, "columns") else list(range(ref.shape[1]))
            out.update(reference_cosine=rc, best_reference=cols[best] if best >= 0 else None, best_reference_cosine=float(rc[best]) if best >= 0 else float("nan"))
        names = self.tumour_names if getattr(self, "tumour_names", None) else None
        included = np.ones(G, dtype=bool) if inc is None else inc.astype(bool)
        out.update(types=pd.DataFrame(dict(type=np.arange(K), bias=typ[0], bias_sd=np.sqrt(typ[1]), p_positive=typ[2], dispersion=typ[3],
                                           dispersion_sd=np.sqrt(typ[4]), component=comp[0], component_mean=comp[1], component_sd=np.sqrt(comp[2]))),
                   tumours=pd.DataFrame(dict(tumour=[names[g] if names is not None else g for g in range(G)], score=tum[0], score_sd=np.sqrt(tum[1]), chi=tum[2],
                                             included=included)))
        self.log(f"Residuals: {r['n_included']} tumours over {r['n_used'] - r['n_flat']} samples ({r['n_flat']} flat); the leading component carries "
                 f"{r['share']:.3g} of the mean matrix's trace (per sample {r['mean_share']:.3g} on average, smallest agreement {r['min_agreement']:.3g}); "
                 f"{r['n_overdispersed']} types with dispersion > {r['max_dispersion']:g} (worst: type {r['worst_type_at']} at {r['worst_type']:.3g}), "
                 f"{r['n_biased']} biased", verbosity=1)
        return out

    def get_tradeoff(self, sets=None, query=None, include=None, relabel=True, min_corr=0.5, end_iter=None, n_samples=None, idx="MAP_idx"):
        """Which signatures trade mutations within a tumour, and how uncertain is a SUM of exposures?  On the device (bnmf_tradeoff_at;
        not in the reference): over iterations end_iter - n_samples + 1 ... end_iter (defaults as get_WAIC), restricted to `idx` (as
        get_contrast), per tumour the N x N covariance of its renormalised exposures over the samples and the correlations.  Flat or
        similar signatures exchange mutations from sample to sample: each marginal interval is wide while the sum is sharply determined,
        and adding two marginal SDs overstates the uncertainty of the sum.  With relabel the range is first aligned by get_relabelling()
        and its perm is handed on; an unmatched sample is left out.  sets: a label per signature (0 .. C-1, -1 = in no set) or a dict
        name -> list of signature indices; query: tumours (indices or names) whose whole matrices are wanted; include as in
        get_similarity.  min_corr = 0.5 is a reporting convention like min_cosine = 0.9 (it only sets the counts), not a test.
        Returns dict(tumours (a data frame: tumour, min_corr, pair_j, pair_l, n_defined, total_ratio, included), pairs (a data frame:
        j, l, mean_corr, n_defined, p_negative, p_positive, mean_cov for j > l), sets (a data frame: set, tumour, mean, sd_sum,
        sd_if_independent, ratio; only with sets), set_names, tumour, pair_at, pair, setstat, dense (the arrays of the call) and its
        info fields)."""
        if not hasattr(self._chain, "tradeoff"):
            raise ValueError("get_tradeoff needs an engine that forms covariances over its recorded samples (tradeoff); this engine_factory's cannot")
        G, N = self.dims["G"], self.dims["N"]
        names = self.tumour_names if getattr(self, "tumour_names", None) else None
        inc = None
        if include is not None:
            vals = list(include.tolist()) if hasattr(include, "tolist") else list(include)
            v = np.array([np.nan if x is None or x is pd.NA else float(x) for x in vals], dtype=np.float64)
            if v.size != G:
                raise ValueError(f"include has {v.size} values for {G} tumours")
            if (~np.isnan(v) & (v != 0) & (v != 1)).any():
                raise ValueError("include holds a value other than 0, 1 and None / NaN")
            inc = (v == 1).astype(np.int32)
        st, set_names = None, None
        if isinstance(sets, dict):
            st, set_names = np.full(N, -1, dtype=np.int32), list(sets)
            for c, nm in enumerate(set_names):
                at = np.asarray(sets[nm], dtype=np.int64).reshape(-1)
                if at.size == 0 or (at < 0).any() or (at >= N).any():
                    raise ValueError(f"set {nm!r} is empty or names a signature outside 0 .. {N - 1}")
                if (st[at] >= 0).any():
                    raise ValueError(f"set {nm!r} holds a signature that another set holds")
                st[at] = c
        elif sets is not None:
            st = np.asarray(sets, dtype=np.int32).reshape(-1)
            if st.size != N:
                raise ValueError(f"sets has {st.size} labels for {N} signatures")
            set_names = list(range(int(st.max()) + 1))
        qv = None
        if query is not None:
            vs = list(np.atleast_1d(query).tolist())
            if names is not None and all(isinstance(q, str) for q in vs):
                missing = [q for q in vs if q not in names]
                if missing:
                    raise ValueError(f"query names no tumour of the data: {missing[:5]}")
                vs = [names.index(q) for q in vs]
            qv = np.asarray(vs, dtype=np.int32)
        n, used, _, kw = self._recorded_range(end_iter, n_samples, idx)
        perm = None
        if relabel:
            rows = np.asarray(self.get_relabelling(end_iter=end_iter, n_samples=n_samples, idx=idx)["perm"], dtype=np.int32)
            perm = np.full((n, N), -1, dtype=np.int32)                   # perm has a row per used sample: scattered into the range's rows
            perm[slice(None) if used is None else np.asarray(used) != 0] = rows
        r = self._chain.tradeoff(n, include=inc, perm=perm, sets=st, query=qv, min_corr=min_corr, used=used, **kw)
        label = (lambda g: names[g]) if names is not None else (lambda g: int(g))
        tum, pat, par = np.asarray(r["tumour"]).reshape(3, G), np.asarray(r["pair_at"]).reshape(G), np.asarray(r["pair"]).reshape(5, N, N)
        included = np.ones(G, dtype=bool) if inc is None else inc.astype(bool)
        out = dict(r)
        out.update(tumours=pd.DataFrame(dict(tumour=[label(g) for g in range(G)], min_corr=tum[0], pair_j=np.where(pat >= 0, pat // N, -1),
                                             pair_l=np.where(pat >= 0, pat % N, -1), n_defined=tum[1], total_ratio=tum[2], included=included)),
                   pairs=pd.DataFrame([(j, l) + tuple(par[:, j, l]) for j in range(N) for l in range(j)],
                                      columns=["j", "l", "mean_corr", "n_defined", "p_negative", "p_positive", "mean_cov"]),
                   set_names=set_names)
        if st is not None and set_names:
            sst = np.asarray(r["setstat"]).reshape(4, len(set_names), G)
            out["sets"] = pd.DataFrame([(nm, label(g), sst[0, c, g], float(np.sqrt(sst[1, c, g])), float(np.sqrt(sst[2, c, g])), sst[3, c, g])
                                        for c, nm in enumerate(set_names) for g in range(G)],
                                       columns=["set", "tumour", "mean", "sd_sum", "sd_if_independent", "ratio"])
        if qv is not None:
            out["query"] = [label(g) for g in qv]
        sp = int(r["strongest_pair_at"])
        self.log(f"Trade-offs: {r['n_included']} tumours over {r['n_matched']} samples ({r['n_unmatched']} unmatched); {r['n_traded']} tumours with a "
                 f"correlation <= -{r['min_corr']:g}; mean variance ratio of the total {r['mean_ratio']:.3g}; strongest pair "
                 f"{(sp // N, sp % N) if sp >= 0 else None} with mean correlation {r['strongest_pair']:.3g}", verbosity=1)
        return out

    def get_sparse_assignment(self, max_loss=0.01, n_steps=20, include=None, end_iter=None, n_samples=None, exposures=False, idx="MAP_idx"):
        """Which signatures does each tumour keep, and how large are they once the others are gone?  On the device (bnmf_prune_at; not
        in the reference): over iterations end_iter - n_samples + 1 ... end_iter (defaults as get_WAIC), restricted to `idx` (as
        get_contrast), per sample and tumour backward elimination of the sample's signatures with a refit of the remaining exposures
        after every removal (n_steps KL steps), while the cosine of the fit stays within max_loss of the full refit's: the refit that
        get_reconstruction's drop leaves out.  Over the samples this gives the probability p_kept that a tumour keeps a signature.
        include as in get_similarity.  max_loss = 0.01 and n_steps = 20 are reporting conventions like min_cosine = 0.9, not tests;
        rel_change tells whether n_steps sufficed.  Returns dict(assignment (a data frame: tumour, signature, load, p_kept for every
        pair with p_kept >= 0.5), tumours (a data frame: tumour, cos_0, cos_f, n_kept, n_kept_min, n_kept_max, rel_change, mean_trials,
        included), load, tumour, series, signature, exposures (the arrays of the call) and its info fields)."""
        if not hasattr(self._chain, "prune"):
            raise ValueError("get_sparse_assignment needs an engine that refits its recorded samples (prune); this engine_factory's cannot")
        G, N = self.dims["G"], self.dims["N"]
        if not np.isfinite(max_loss):
            raise ValueError(f"max_loss = {max_loss} is not a finite number")
        if int(n_steps) != n_steps or n_steps < 1:
            raise ValueError(f"n_steps = {n_steps} is not a whole number >= 1")
        names = self.tumour_names if getattr(self, "tumour_names", None) else None
        inc = None
        if include is not None:
            vals = list(include.tolist()) if hasattr(include, "tolist") else list(include)
            v = np.array([np.nan if x is None or x is pd.NA else float(x) for x in vals], dtype=np.float64)
            if v.size != G:
                raise ValueError(f"include has {v.size} values for {G} tumours")
            if (~np.isnan(v) & (v != 0) & (v != 1)).any():
                raise ValueError("include holds a value other than 0, 1 and None / NaN")
            inc = (v == 1).astype(np.int32)
        n, used, _, kw = self._recorded_range(end_iter, n_samples, idx)
        r = self._chain.prune(n, include=inc, n_steps=int(n_steps), max_loss=float(max_loss), used=used, exposures=bool(exposures), **kw)
        label = (lambda g: names[g]) if names is not None else (lambda g: int(g))
        load, tum = np.asarray(r["load"]).reshape(4, N, G), np.asarray(r["tumour"]).reshape(7, G)
        included = np.ones(G, dtype=bool) if inc is None else inc.astype(bool)
        out = dict(r)
        out.update(assignment=pd.DataFrame([(label(g), nn, load[0, nn, g], load[3, nn, g]) for g in range(G) for nn in range(N) if load[3, nn, g] >= 0.5],
                                           columns=["tumour", "signature", "load", "p_kept"]),
                   tumours=pd.DataFrame(dict(tumour=[label(g) for g in range(G)], cos_0=tum[0], cos_f=tum[1], n_kept=tum[2], n_kept_min=tum[3], n_kept_max=tum[4],
                                             rel_change=tum[5], mean_trials=tum[6], included=included)))
        self.log(f"Sparse assignment: {r['n_included']} tumours ({r['n_undefined']} all-zero) over {r['n_used']} samples, max_loss {r['max_loss']:g}, "
                 f"{r['n_steps']} steps; {len(out['assignment'])} (tumour, signature) pairs kept with p >= 0.5; {r['n_single']} tumours with one signature; "
                 f"{r['trials']} trials; largest last-step change {r['max_change']:.3g}", verbosity=1)
        return out

    def get_summary(self, probs=(0.05, 0.25, 0.5, 0.75, 0.95), min_load=1.0, include=None, relabel=True, credible_interval=0.95, series=False,
                    end_iter=None, n_samples=None, idx="MAP_idx"):
        """How is a signature's load distributed across the cohort?  On the device (bnmf_summary_at; the reference's summary() reports
        the carriers' median and the prevalence of the MAP point estimate alone): over iterations end_iter - n_samples + 1 ... end_iter
        (defaults as get_WAIC), restricted to `idx` (as get_contrast), per sample and signature the prevalence (tumours with a load >=
        min_load), the total load, its fraction of the cohort's, the carriers' mean and, at every level of probs, the exact quantile of
        all loads (load_all_<p>), of the carriers' loads (load_present_<p>) and of the shares (share_all_<p>): each a posterior with an
        interval.  With relabel the range is first aligned by get_relabelling() and its perm is handed on; an unmatched sample is left
        out.  include as in get_similarity.  Returns a dict per statistic name of dict(mean, var, lower, upper, n_valid), each of
        length N, plus names, probs, stat, the info fields and with series the series (NSTAT x S x N)."""
        if not hasattr(self._chain, "summary"):
            raise ValueError("get_summary needs an engine that sorts the loads of its recorded samples (summary); this engine_factory's cannot")
        G, N = self.dims["G"], self.dims["N"]
        inc = None
        if include is not None:
            vals = list(include.tolist()) if hasattr(include, "tolist") else list(include)
            v = np.array([np.nan if x is None or x is pd.NA else float(x) for x in vals], dtype=np.float64)
            if v.size != G:
                raise ValueError(f"include has {v.size} values for {G} tumours")
            if (~np.isnan(v) & (v != 0) & (v != 1)).any():
                raise ValueError("include holds a value other than 0, 1 and None / NaN")
            inc = (v == 1).astype(np.int32)
        n, used, _, kw = self._recorded_range(end_iter, n_samples, idx)
        perm = None
        if relabel:
            rows = np.asarray(self.get_relabelling(end_iter=end_iter, n_samples=n_samples, idx=idx)["perm"], dtype=np.int32)
            perm = np.full((n, N), -1, dtype=np.int32)                   # perm has a row per used sample: scattered into the range's rows
            perm[slice(None) if used is None else np.asarray(used) != 0] = rows
        r = self._chain.summary(n, probs=probs, include=inc, perm=perm, min_load=float(min_load), credible_interval=credible_interval, used=used,
                                series=bool(series), **kw)
        st = np.asarray(r["stat"])
        out = dict(r)
        for q, name in enumerate(r["names"]):
            out[name] = dict(mean=st[q, 0], var=st[q, 1], lower=st[q, 2], upper=st[q, 3], n_valid=st[q, 4])
        self._summary_posterior = dict(out, min_load=float(min_load))
        self.reference_comparison["summary"] = None                      # the frame gains the posterior columns: made again on demand
        prev = out["prevalence"]["mean"]
        self.log(f"Summary: {r['n_included']} tumours over {r['n_aligned']} of {r['n_used']} samples, {r['n_levels']} levels, min_load {r['min_load']:g}; "
                 f"mean prevalence {np.nanmin(prev):.3g} .. {np.nanmax(prev):.3g}; {r['n_nonfinite']} (sample, signature) with a load that is not finite",
                 verbosity=1)
        return out

    def summary(self, reference_P=None, reference_names=None):
        """summary.bayesNMF_sampler (R/postprocessing.R:18-91): one row per signature of the MAP with G, N, K, Signature,
        Med_Contribution (the median load among the tumours with a load >= 1) and Prop_atleast_1 (their share); with reference_P (K x R;
        no catalogue is bundled, so "cosmic" is not a default) also Reference_Signature and Cosine_Similarity through
        assign_signatures_ensemble.  Kept in self.reference_comparison["summary"] and returned from there until the reference changes.
        After a get_summary() whose probs hold 0.5 and whose min_load is 1 the frame also has Med_Contribution_post, _lower, _upper,
        Prop_atleast_1_post, _lower and _upper: the device's posterior of the same two quantities."""
        K = self.dims["K"]
        if isinstance(reference_P, str):
            raise ValueError("Parameter `reference_P` must be a matrix or None: no catalogue is bundled")
        ref = None if reference_P is None else np.asarray(reference_P, dtype=float)
        if ref is not None and ref.shape[0] != K:
            self.log(f"Reference matrix has {ref.shape[0]} rows, but data has {K} rows. Setting `reference_P` to NULL.", verbosity=1)
            ref = None
        rc = self.reference_comparison
        if ref is not None:
            same = rc.get("reference_P") is not None and np.array_equal(np.asarray(rc["reference_P"]), ref) and rc.get("assignments") is not None
            if not same:                                                  # only reassigns signatures if the reference set has changed
                self.assign_signatures_ensemble(ref, reference_names=reference_names)
                rc["summary"] = None
            asg = rc["assignments"]
            sig_est, sig_ref, cos = list(asg["sig_est"]), list(asg["sig_ref"]), list(asg["MAP_cosine"])
        else:
            sig_est = list(range(1, np.asarray(self.MAP["P"]).shape[1] + 1))
            sig_ref, cos = sig_est, None
        if rc.get("summary") is not None and (("Reference_Signature" in rc["summary"].columns) == (ref is not None)):
            return rc["summary"]
        E = np.asarray(self.MAP["E"], dtype=float)
        # the row of MAP["E"] of every summary row (MAP$sig_idx) and the factor it is among the chain's N (the place in get_summary's arrays)
        if ref is not None:
            rows_at, factor = np.asarray(self.MAP["sig_idx"], dtype=int), np.asarray(rc["keep_sigs"], dtype=int)
        else:
            rows_at = np.arange(len(sig_est))
            ks = np.asarray(self.MAP.get("keep_sigs", rows_at), dtype=int)
            factor = ks if len(ks) == len(rows_at) else rows_at
        post = getattr(self, "_summary_posterior", None)
        lvl = None
        if post is not None and post["min_load"] == 1.0 and (np.asarray(post["probs"]) == 0.5).any():
            lvl = f"load_present_{0.5:g}"
        rows = []
        for i, est in enumerate(sig_est):
            row = E[rows_at[i]]
            one = row >= 1
            d = dict(G=self.dims["G"], N=self.dims["N"], K=K, Signature=est, Med_Contribution=float(np.median(row[one])) if one.any() else float("nan"),
                     Prop_atleast_1=float(one.mean()))
            if ref is not None:
                d.update(Reference_Signature=sig_ref[i], Cosine_Similarity=cos[i])
            if lvl is not None:
                lab = int(factor[i])
                med, prv = post[lvl], post["prevalence"]
                d.update(Med_Contribution_post=med["mean"][lab], Med_Contribution_lower=med["lower"][lab], Med_Contribution_upper=med["upper"][lab],
                         Prop_atleast_1_post=prv["mean"][lab], Prop_atleast_1_lower=prv["lower"][lab], Prop_atleast_1_upper=prv["upper"][lab])
            rows.append(d)
        rc["summary"] = pd.DataFrame(rows)
        return rc["summary"]

    def _mean_share_profiles(self, n, used, perm, kw):
        """N x G: the mean over the used, matched samples of the range of every tumour's aligned share profile (the host's start of
        get_subtypes; a sample in which a tumour has no exposure does not enter its mean)."""
        it = self.state["iter"]
        end = kw.get("end_iter", it)
        back = it - (end - n + 1) + 1
        win = {nm: self._chain.window(nm, back)[:n] for nm in ("P", "E", "A")}
        N, G = self.dims["N"], self.dims["G"]
        tot, cnt = np.zeros((N, G)), np.zeros(G)
        for s in range(n):
            if (used is not None and not used[s]) or (perm is not None and (perm[s] < 0).all()):
                continue
            x = np.asarray(win["E"][s], dtype=float) * np.asarray(win["P"][s], dtype=float).sum(axis=0)[:, None] * (np.ravel(win["A"][s]) != 0)[:, None]
            t = x.sum(axis=0)
            ok = (t > 0) & np.isfinite(t)
            q = np.zeros((N, G))
            q[np.arange(N) if perm is None else perm[s]] = np.where(ok, x / np.where(ok, t, 1.0), 0.0)
            tot += q
            cnt += ok
        return tot / np.where(cnt > 0, cnt, 1.0)

    def _recorded_range(self, end_iter, n_samples, idx, want_mode=False):
        """The range and sample selection of get_WAIC / get_mixing / get_PPC / get_attribution / get_projection / get_decomposition / get_contrast / get_regression / get_coactivity / get_stability / get_reconstruction / get_similarity / get_subtypes / get_residuals / get_tradeoff / get_sparse_assignment: (n, used flags or None, mode of A over the range as 0 / 1 flags of
        the N factors if want_mode, end_iter keyword of the engine call)."""
        cc = self.specs["convergence_control"]
        it = self.state["iter"]
        default = end_iter is None and n_samples is None
        end_iter = it if end_iter is None else int(end_iter)
        n = min(cc["MAP_over"], it) if n_samples is None else int(n_samples)
        first_iter = end_iter - n + 1
        lo, hi = self._kept_range()
        if n < 1 or first_iter < lo or end_iter > hi:
            raise ValueError(f"iterations {first_iter}..{end_iter} are not all recorded: the kept samples are iterations {lo}..{hi}")
        N = self.dims["N"]
        mode_used = mode_A = None
        have_map = default and "idx" in self.MAP
        if (isinstance(idx, str) and idx == "MAP_idx" and not have_map) or (want_mode and not (default and "keep_sigs" in self.MAP)):
            if hasattr(self._chain, "map"):
                r = self._chain.map(n, None, end_iter=end_iter)
                mode_used, mode_A = np.asarray(r["used"], dtype=np.int32), (np.ravel(r["A"]) != 0).astype(np.int32)
            else:
                mode = get_mode(self._chain.window("A", it - first_iter + 1)[:n])
                mode_used = np.zeros(n, dtype=np.int32)
                mode_used[mode["idx"]] = 1
                mode_A = (np.ravel(mode["matrix"]) != 0).astype(np.int32)
        if want_mode and mode_A is None:                   # the last MAP's: its kept factors, or those its A includes
            A, ks = np.ravel(self.MAP["A"]), np.asarray(self.MAP["keep_sigs"], dtype=int)
            mode_A = np.zeros(N, dtype=np.int32)
            mode_A[ks[A != 0] if len(ks) == len(A) else ks] = 1
        if idx is None:
            used = None
        elif isinstance(idx, str):
            if idx != "MAP_idx":
                raise ValueError("Parameter `idx` must be 'MAP_idx', None or a vector of recorded iterations")
            if have_map:
                ia = np.asarray(self.MAP["idx"], dtype=int)
                ia = ia[(ia >= first_iter) & (ia <= end_iter)]
                used = np.zeros(n, dtype=np.int32)
                used[ia - first_iter] = 1
            else:
                used = mode_used
        else:
            ia = np.asarray(idx, dtype=int).ravel()
            if ia.size and (ia.min() < first_iter or ia.max() > end_iter):
                raise ValueError(f"idx must lie in the iterations {first_iter}..{end_iter}")
            used = np.zeros(n, dtype=np.int32)
            used[ia - first_iter] = 1
        return n, used, mode_A, ({} if end_iter == it else dict(end_iter=end_iter))

    def get_mixing(self, end_iter=None, n_samples=None, idx="MAP_idx", arrays=True):
        """Mixing diagnostics of the recorded samples, on the device (bnmf_mixing_at; not in the reference): for every element of the
        renormalised P and E over iterations end_iter - n_samples + 1 ... end_iter (defaults as get_WAIC: the last MAP_over samples),
        restricted to `idx` ("MAP_idx": those whose A equals the mode of the range; None: every sample; else a vector of recorded
        iterations) — the mean and variance, Geyer's effective sample size, the Monte-Carlo standard error of the mean, split R-hat and
        the halves' moments (Engine.mixing: name_P is K x N, name_E is N x G, over all N factors), with a summary over the factors of
        the mode of A: n_const, n_ran_out, n_low_ess (< 100), n_high_rhat (> 1.01), the smallest ESS and largest R-hat of each side.
        Caveat: a lag counts USED samples, not iterations.  Where `idx` leaves gaps in the range (samples whose A is not the mode),
        the samples that remain are treated as one contiguous series, as get_MAP's idx is; autocorrelations across a gap are then
        those of the thinned series."""
        if not hasattr(self._chain, "mixing"):
            raise ValueError("get_mixing needs an engine that computes mixing diagnostics over its recorded samples (mixing); this engine_factory's cannot")
        n, used, keep, kw = self._recorded_range(end_iter, n_samples, idx, want_mode=True)
        return self._chain.mixing(n, used=used, keep=keep, arrays=arrays, **kw)

    def _log_mixing(self):
        """one line after the final MAP: how many independent draws the summaries rest on"""
        if not hasattr(self._chain, "mixing"):
            return
        try:
            m = self.get_mixing(arrays=False)
        except Exception as ex:  # noqa: BLE001  (e.g. fewer than 4 samples share the mode of A)
            self.log(f"Mixing not computed: {ex}", verbosity=1)
            return
        self.log(f"Mixing over {m['n_used']} samples: min ESS P {m['min_ess_P']:.1f} E {m['min_ess_E']:.1f} | max split R-hat P {m['max_rhat_P']:.4f} "
                 f"E {m['max_rhat_E']:.4f} | {m['n_low_ess']} ESS < 100 | {m['n_high_rhat']} R-hat > 1.01 | {m['n_const']} constant | "
                 f"{m['n_ran_out']} ran out of lags", verbosity=1)

    def get_relabelling(self, end_iter=None, n_samples=None, idx="MAP_idx", pivot="MAP", max_rounds=10, aligned=False):
        """Label-switching correction of the recorded samples, on the device (bnmf_relabel_at; not in the reference): over iterations
        end_iter - n_samples + 1 ... end_iter (defaults as get_WAIC: the last MAP_over samples), restricted to `idx` ("MAP_idx": those
        whose A equals the mode of the range; None: every sample; else a vector of recorded iterations), every sample's factors are
        permuted to the labels of a pivot so that the total cosine between its signatures and the pivot's is largest, and the pivot
        is iterated to the aligned mean (at most max_rounds rounds).  pivot: "MAP" — the MAP's P, the factors it dropped put back
        from the last sample; "last" — the newest used sample's P; or a K x N matrix.
        Returns Engine.relabel's dict over all N factors (perm: S x N, the label factor n of sample s receives, -1 for a sample that
        could not be matched; cosine; confusion; P_mean, P_var, E_mean, E_var of the aligned, renormalised samples; rounds, converged,
        n_switched, n_unmatched, mean_cosine, min_cosine, min_cosine_at; with aligned also aligned_P, aligned_E), plus P (K x kept) and
        E (kept x G): the aligned means restricted to the MAP's kept factors, and keep_sigs, their indices."""
        if not hasattr(self._chain, "relabel"):
            raise ValueError("get_relabelling needs an engine that aligns its recorded samples (relabel); this engine_factory's cannot")
        n, used, _, kw = self._recorded_range(end_iter, n_samples, idx)
        K, N = self.dims["K"], self.dims["N"]
        ks = np.asarray(self.MAP["keep_sigs"], dtype=int) if "keep_sigs" in self.MAP else np.arange(N)
        if isinstance(pivot, str):
            if pivot == "last":
                piv = None
            elif pivot == "MAP":
                if "P" not in self.MAP:
                    raise ValueError("get_relabelling(pivot = 'MAP') needs a MAP: call get_MAP first, or pass pivot = 'last' or a matrix")
                piv = np.array(self._chain.get("P"), dtype=float)          # the dropped factors: the last sample's columns
                MP = np.asarray(self.MAP["P"], dtype=float)
                piv[:, ks] = MP if MP.shape[1] == len(ks) else MP[:, ks]
            else:
                raise ValueError("Parameter `pivot` must be 'MAP', 'last' or a K x N matrix")
        else:
            piv = np.asarray(pivot, dtype=float)
            if piv.shape != (K, N):
                raise ValueError(f"pivot is {piv.shape}, but P is {(K, N)}")
        r = self._chain.relabel(n, used=used, pivot_P=piv, max_rounds=max_rounds, aligned=aligned, **kw)
        out = dict(r)
        out.update(P=r["P_mean"][:, ks], E=r["E_mean"][ks, :], keep_sigs=ks)
        return out

    def _log_relabelling(self):
        """one line after the mixing line: whether the labels moved inside the range the summaries rest on"""
        if not hasattr(self._chain, "relabel"):
            return
        try:
            r = self.get_relabelling()
        except Exception as ex:  # noqa: BLE001  (e.g. fewer than 2 samples share the mode of A)
            self.log(f"Relabelling not computed: {ex}", verbosity=1)
            return
        self.log(f"Relabelling over {r['n_used']} samples: {r['rounds']} round{'' if r['rounds'] == 1 else 's'}"
                 f"{'' if r['converged'] else ' (not converged)'} | {r['n_switched']} samples switched | {r['n_unmatched']} unmatched | "
                 f"smallest cosine {r['min_cosine']:.4f}", verbosity=1)

    def label_switching(self, reference_P, reference_names=None, idx="all"):
        """The data frame plot_label_switching (R/postprocessing_visualizations.R:598-669) builds before combine_below: for every
        recorded iteration in `idx` ("all": every kept sample) the diagonal of hungarian_assignment(P_t, reference_P,
        return_mat = TRUE, keep_all_est = TRUE) over all N latent factors, computed on the device (bnmf_label_switching).
        Columns iter, estimated ("Est<k>"), assigned (reference name, "None" without a partner), cosine_sim, k, included
        ("Included" / "Excluded"), ordered by iter then k.  With idx = "all" it is kept in reference_comparison["label_switching_df"]."""
        ref = np.asarray(reference_P, dtype=float)
        if ref.shape[0] != self.dims["K"]:
            raise ValueError(f"Reference matrix has {ref.shape[0]} rows, but data has {self.dims['K']} rows.")
        names = list(reference_names) if reference_names is not None else [f"Ref{j}" for j in range(1, ref.shape[1] + 1)]
        lo, hi = self._kept_range()
        save = isinstance(idx, str)
        if save:
            if idx != "all":
                raise ValueError("Parameter `idx` must be a vector of indices or 'all'")
            iters = np.arange(lo, hi + 1)
        else:
            iters = np.sort(np.asarray(idx, dtype=int).ravel(), kind="stable")
            if iters.size and iters.min() > self.state["iter"]:
                raise ValueError("Parameter `idx` must be a vector of indices less than or equal to the total number of iterations: "
                                 f"{self.state['iter']}")
            if iters.size and (iters.min() < lo or iters.max() > hi):
                raise ValueError(f"idx must be recorded iterations that are still kept: {lo}..{hi}")
        N = self.dims["N"]
        r = self._chain.label_switching(iters, ref)
        a = r["assigned"].ravel()
        df = pd.DataFrame(dict(iter=np.repeat(iters, N), estimated=[f"Est{k}" for k in range(1, N + 1)] * len(iters),
                               assigned=["None" if j < 0 else names[j] for j in a], cosine_sim=r["cosine"].ravel(),
                               k=np.tile(np.arange(1.0, N + 1), len(iters)),
                               included=np.where(r["included"].ravel(), "Included", "Excluded")))
        if save:
            self.reference_comparison["label_switching_df"] = df
        return df

    def save_object(self):
        """save_object (R/bayesNMF_sampler.R:414-416): sampler.rds -> sampler.pkl (fields, not the device handle).  With
        save_engine_state the device state goes to engine_state.bin beside it: a full record at the first save, then a delta since
        the previous save (load_sampler reopens both)."""
        eng = self.specs.get("save_engine_state")
        if eng:
            since, it = int(self.state.get("engine_state_iter", 0)), int(self.state["iter"])
            self.state["engine_state_iter"] = it               # (the pickle below describes the chain as the file will end)
        keep = {k: v for k, v in self.__dict__.items() if k not in ("_chain", "log_con", "_block_hook")}
        with open(os.path.join(self.specs["output_dir"], "sampler.pkl"), "wb") as f:
            pickle.dump(keep, f)
        if eng:
            path = os.path.join(self.specs["output_dir"], ENGINE_STATE_FILE)
            if since == 0 or not os.path.exists(path):
                self._chain.save_state(path)
            elif since < it:                                    # (since == it: the file already ends at this iteration)
                self._chain.save_state(path, since_iter=since)

    def close(self):
        if getattr(self, "log_con", None) is not None:
            self.log_con.write("[INFO] Finalizing and closing log file\n")
            self.log_con.close()
            self.log_con = None
        if getattr(self, "_chain", None) is not None:
            self._chain.close()
            self._chain = None


def summarize_samplers(sampler_dict, reference_P=None):
    """summarize_samplers (R/postprocessing.R:114-152): the summary() frames of a dict name -> sampler under one another, each with a
    Name column "name (G)".  A sampler that has not finished (state["converged"] unset or false; the reference tests is.null) is
    reported and skipped; samplers of differing K are refused.  No catalogue is bundled, so reference_P is a matrix or None."""
    if isinstance(reference_P, str):
        raise ValueError("Parameter `reference_P` must be a matrix or None: no catalogue is bundled")
    rows = [s.dims["K"] for s in sampler_dict.values()]
    if len(set(rows)) > 1:
        raise ValueError("All samplers must have the same number of variables.")
    frames = []
    for name, s in sampler_dict.items():
        if not s.state.get("converged"):
            print(f"not done: {name}")
            continue
        df = s.summary(reference_P).copy()
        df["Name"] = f"{name} ({s.dims['G']})"
        frames.append(df)
    return pd.concat(frames, ignore_index=True) if frames else None


ENGINE_STATE_FILE = "engine_state.bin"


def load_sampler(output_dir, device=None):
    """A live sampler from a directory that bayesNMF_sampler(save_engine_state=True) saved into: sampler.pkl unpickled, an Engine made
    with the saved config (on `device`, default the saved one) and engine_state.bin replayed into it, log.txt reopened for append.
    samples, get_MAP(end_iter, n_samples), assign_signatures_ensemble, label_switching and run_gibbs_sampler() (resume) all work."""
    pkl, st = os.path.join(output_dir, "sampler.pkl"), os.path.join(output_dir, ENGINE_STATE_FILE)
    if not os.path.exists(st):
        raise FileNotFoundError(f"load_sampler: {st} does not exist (was the sampler run with save_engine_state=True?)")
    if not os.path.exists(pkl):
        raise FileNotFoundError(f"load_sampler: {pkl} does not exist")
    with open(pkl, "rb") as f:
        fields = pickle.load(f)
    s = bayesNMF_sampler.__new__(bayesNMF_sampler)
    s.__dict__.update(fields)
    sp = s.specs
    if not sp.get("save_engine_state"):
        raise ValueError(f"load_sampler: {pkl} was not saved with save_engine_state=True")
    dev = sp["device"] if device is None else int(device)
    normal = sp["likelihood"] == "normal"
    s._chain = Engine(np.asfortranarray(s.data, dtype=np.float64 if normal else np.int32), s.dims["N"], likelihood=sp["likelihood"],
                      prior=sp["prior"], MH=sp["MH"], learning_rank=sp["learning_rank"], rank_method=sp["engine_rank_method"],
                      seed=sp["seed"], chain_id=sp["chain_id"], temperature=s.temperature_schedule, save_Z=sp["save_Z"],
                      window=sp["window"], device=dev)
    if sp.get("fixed_P") is not None:                        # (the state file carries the mask too: load_state checks the two agree)
        mask = np.zeros(s.dims["N"], dtype=np.int32)
        mask[:np.asarray(sp["fixed_P"]).shape[1]] = 1
        s._chain.set_fixed("P", mask)
    it = s._chain.load_state(st)
    if it != int(s.state["iter"]):
        s._chain.close()
        raise RuntimeError(f"load_sampler: {st} ends at iteration {it}, {pkl} at iteration {int(s.state['iter'])}")
    sp["output_dir"], sp["device"] = output_dir, dev
    s._block_hook = None
    s.log_con = open(os.path.join(output_dir, "log.txt"), "a")
    return s


def bayesNMF(data, rank, likelihood="poisson", prior="truncnormal", rank_method="SBFI", MH=None,
             convergence_control=None, prop_temp=0.2, post_warmup=None, output_dir=None, overwrite=False,
             hyperprior_params=None, init_prior_params=None, init_params=None, periodic_save=True,
             save_all_samples=True, seed=1, chain_id=0, device=0, save_Z=False, engine_factory=None,
             intermediate_credible_intervals=False, n_chains=1, devices=None, engine_side_convergence=True, save_engine_state=False,
             fixed_P=None):
    """bayesNMF() (R/bayesNMF.R:24-138): build the sampler and run it; with rank_method = "BIC" run one
    fixed-rank sampler per rank and return dict(results, best_rank, sampler).  rank_method = "WAIC" (not in the reference) runs the
    same per-rank sweep, adds elpd_waic, se_elpd, p_waic and n_high_var (get_WAIC over each sampler's final MAP window) to the
    results beside BIC, and picks the largest elpd_waic.

    New optional trailing arguments: seed, chain_id, device, save_Z, and n_chains / devices:
    n_chains > 1 runs independent replicas (chain_id = 0..n_chains-1 in the Philox key), chain c on
    devices[c % len(devices)], and returns the list of samplers (multichain.run_chains).

    fixed_P (K x F): known signatures held fixed as columns 1..F of P (never drawn); the rank, or the top of a rank range, must
    be >= F.  F == rank is a refit (only E is sampled); with a rank range SBFI / BFI learn which of the known signatures are
    present; with rank_method = "BIC" the ranks below F are dropped."""
    if n_chains and n_chains > 1:
        from .multichain import run_chains
        kw = dict(likelihood=likelihood, prior=prior, rank_method=rank_method, MH=MH, convergence_control=convergence_control,
                  prop_temp=prop_temp, post_warmup=post_warmup, output_dir=output_dir, overwrite=overwrite,
                  hyperprior_params=hyperprior_params, init_prior_params=init_prior_params, init_params=init_params,
                  periodic_save=periodic_save, save_all_samples=save_all_samples, seed=seed, save_Z=save_Z,
                  engine_factory=engine_factory, intermediate_credible_intervals=intermediate_credible_intervals,
                  engine_side_convergence=engine_side_convergence, save_engine_state=save_engine_state, fixed_P=fixed_P)
        return run_chains(data, rank, n_chains=n_chains, devices=devices, **kw)
    if output_dir is None:
        output_dir = f"nmf_{likelihood}_{prior}"
    common = dict(likelihood=likelihood, prior=prior, rank_method=rank_method, MH=MH,
                  convergence_control=convergence_control, prop_temp=prop_temp, post_warmup=post_warmup,
                  overwrite=overwrite, hyperprior_params=hyperprior_params, init_prior_params=init_prior_params,
                  init_params=init_params, verbosity=1, periodic_save=periodic_save,
                  save_all_samples=save_all_samples, seed=seed, chain_id=chain_id, device=device, save_Z=save_Z,
                  engine_factory=engine_factory, intermediate_credible_intervals=intermediate_credible_intervals,
                  engine_side_convergence=engine_side_convergence, save_engine_state=save_engine_state, fixed_P=fixed_P)
    ranks = np.atleast_1d(np.asarray(rank, dtype=int))
    if ranks.size > 1 and rank_method in ("BIC", "WAIC"):
        waic = rank_method == "WAIC"
        if fixed_P is not None:
            F = np.asarray(fixed_P).shape[1] if np.ndim(fixed_P) > 1 else 1
            if (ranks < F).any():
                print(f"fixed_P has {F} columns: dropping ranks {[int(k) for k in ranks[ranks < F]]} (below {F}) from the {rank_method} sweep")
                ranks = ranks[ranks >= F]
            if ranks.size == 0:
                raise ValueError(f"ERROR: fixed_P has {F} columns, but the top of the rank range is below {F}")
        # One fixed-rank sampler per rank (R/bayesNMF.R:66-126).  The reference runs them one after the other; they are
        # independent, so here they run concurrently, one host thread per sampler, spread over the visible GPUs
        # (SURVEY.md 8 f2); `devices` picks the GPUs, default all of them.
        import concurrent.futures as cf
        if devices is None:
            try:
                from .engine import device_count
                devices = list(range(max(1, device_count()))) if engine_factory is None else [device]
            except Exception:  # noqa: BLE001
                devices = [device]
        common.pop("device")

        def one(i_k):
            i, k = i_k
            s = bayesNMF_sampler(data, int(k), output_dir=os.path.join(output_dir, f"rank_{k}"), device=devices[i % len(devices)], **common)
            if waic and not hasattr(s._chain, "waic"):
                s.close()
                raise ValueError("rank_method = 'WAIC' needs an engine that computes WAIC over its recorded samples (waic); this engine_factory's cannot")
            s.run_gibbs_sampler()
            bic = float(s.state["MAP_metrics"].iloc[-1]["BIC"])
            row = dict(rank=int(k), dir=s.specs["output_dir"], BIC=bic, time=s.time["total"], sampler=s)
            if waic:                                     # over the final MAP window, the samples whose A is its mode (MAP$idx)
                w = s.get_WAIC()
                row.update({c: w[c] for c in ("elpd_waic", "se_elpd", "p_waic", "n_high_var")})
            return row

        with cf.ThreadPoolExecutor(max_workers=max(1, min(len(ranks), 4 * len(devices)))) as ex:
            results = list(ex.map(one, enumerate(ranks)))
        table = pd.DataFrame([{k: v for k, v in r.items() if k != "sampler"} for r in results])
        if waic:                                         # the largest expected log pointwise predictive density
            best = max(results, key=lambda r: r["elpd_waic"])
            return dict(results=table.sort_values("elpd_waic", ascending=False), best_rank=best["rank"], sampler=best["sampler"])
        best = min(results, key=lambda r: r["BIC"])
        return dict(results=table.sort_values("BIC"), best_rank=best["rank"], sampler=best["sampler"])
    if ranks.size > 1 and rank_method not in ("SBFI", "BFI"):
        raise ValueError("Rank method must be SBFI, BFI, BIC, or WAIC")
    sampler = bayesNMF_sampler(data, rank, output_dir=output_dir, **common)
    sampler.run_gibbs_sampler()
    return sampler
