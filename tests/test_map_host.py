"""The numpy restatement of bnmf_map and bnmf_assign (tests/map_ref.py), pinned on the CPU: fed with the samples of the CPU oracle, one
run(1) at a time, for the chains and ranges of tests/test_gpu_map_bits.py and tests/test_gpu_assign_bits.py (tests/map_cases.py), and
compared with independent plain numpy / scipy evaluations under bounds derived next to each assertion (u = 2^-53, gamma(n) = n u /
(1 - n u): the relative error of n roundings).  The restatement's own order of operations is what the device is held to bit for bit; these
checks show that it is a correct get_MAP_ / assign_signatures_ensemble_ to within rounding.

What the rehearsal on the oracle showed (asserted in test_the_chains_hold_what_the_gpu_tests_rely_on; the device's rings are the
oracle's bits, so tests/test_gpu_map_bits.py asserts the same from e.window):
  rank_n3 (seed 3, K = 12, G = 8, N = 3, temperature 1 for 20 iterations, 0 for 3, then a ramp from 1e-6): iterations 27 .. 38 hold 5
      patterns with counts [3, 3, 3, 2, 1] (a three-way tie: the alphabetical rule picks 010), used = 000010010001; iterations 31 .. 40
      hold 5 with counts [3, 3, 2, 1, 1], used = 1001000100: n_used = 3 < n_samples, a slot list with gaps, across the ring's wrap
  sbfi (seed 14, N = 20): every sample of either range has a pattern of its own (12 and 10 patterns, n_used = 1), the mode is the
      alphabetically first, all zeros (iteration 31): top_A is cut at 5 of them, and bnmf_assign with keep = A_mode keeps nothing
  normal: 13 of the 120 cells of the data are negative
  fix1: every element of column 1 of P holds one value in all samples (12 and 10 repeats); no other element repeats
  fixall_mh (seed 4, truncnormal prior, converged = True, P = 0.1 sqrt(mean(M) K / N) Dirichlet(1) columns): 20 of the 21 elements of E
      (19 of 21 in the last 10) hold a repeated value inside the range, several one value in every sample
  route (K = 5, G = 3, N = 2, 2,150 iterations): one pattern; no repeated value at all
  the assignment: the optimum was unique in every sample of every case but the tied catalogue (see test_assign_restatement_against_scipy,
      which prints the counts), so the lowest-column rule decides there alone."""
import numpy as np
import pytest

import map_cases as MC
import map_ref as R
import relabel_ref

U = 2.0 ** -53
LD = np.longdouble


def gamma(n):
    return n * U / (1.0 - n * U)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


_ORC = {}


def _samples(case):
    if case not in _ORC:
        _ORC[case] = MC.oracle_samples(case, MC.ROUTE_END if case == "route" else MC.T_END)
    return _ORC[case]


def _range(case, end, n):
    P, E, A, M = _samples(case)
    return P[end - n:end], E[end - n:end], A[end - n:end], M


def _check_map(Pw, Ew, Aw, M, ci, fit=True):
    r = R.map_reference(Pw, Ew, Aw, M, ci)
    last_n, K, N = Pw.shape
    G = Ew.shape[2]
    # the mode of A: np.unique sorts the patterns alphabetically, a stable sort by falling count keeps that order among equals
    keys = np.array(["".join(str(int(v != 0)) for v in a) for a in Aw])
    names, counts = np.unique(keys, return_counts=True)
    order = np.argsort(-counts, kind="stable")
    used = keys == names[order[0]]
    assert np.array_equal(r["used"], used.astype(np.int32)) and r["n_used"] == used.sum() and r["n_patterns"] == len(names)
    assert r["top_counts"] == (list(counts[order][:5]) + [0] * 5)[:5]
    assert ["".join(str(int(v)) for v in row) for row in r["top_A"][:min(5, len(names))]] == list(names[order][:5])
    assert np.isnan(r["top_A"][len(names):]).all() and "".join(str(int(v)) for v in r["A"]) == names[order[0]]
    nu = int(used.sum())
    Pu, Eu = Pw[used], Ew[used]
    # the column sums: a value passes ceil(K / 64) - 1 additions in its lane (the first, to +0.0, is exact) and the 6 levels of the tree
    cs_ld = Pu.astype(LD).sum(axis=1)
    assert (np.abs(r["cs"] - cs_ld) <= (gamma((K + 63) // 64 - 1 + 6) + K * 2.0 ** -63) * cs_ld).all()
    cs, x, e = R.renormalised(Pu, Eu)
    for nm, ser in (("P", x), ("E", e)):
        # the mean: a sequential sum of nu non-negative terms is within (nu - 1) u relative, the division adds one rounding: gamma(nu);
        # the longdouble sum it is compared with is itself within nu 2^-64
        ld = ser.astype(LD).sum(axis=0) / LD(nu)
        assert (np.abs(r[nm] - ld) <= (gamma(nu) + nu * 2.0 ** -63) * ld).all(), nm
        if not ci:
            assert r[nm + "_lower"] is None and r[nm + "_upper"] is None
            continue
        srt = np.sort(ser, axis=0)
        for side, p in (("_lower", 0.5 - ci / 2.0), ("_upper", 0.5 + ci / 2.0)):
            # (1 - g) a + g b makes 3 roundings on the way to a sum of non-negative terms: gamma(3) b; numpy's a + (b - a) g makes 3
            # and, from g = 0.5 on, b - (b - a)(1 - g) makes 4, on terms no larger than b: gamma(4) b
            j, _ = R.type7(nu, p)
            b = srt[min(j + 1, nu - 1)]
            q = np.quantile(ser, p, axis=0, method="linear")
            assert (np.abs(r[nm + side] - q) <= (gamma(3) + gamma(4)) * b).all(), (nm, side)
            assert (srt[j] <= r[nm + side] * (1 + 2 * U)).all() and (r[nm + side] <= b * (1 + 2 * U)).all()
            tie = srt[j] == b                                  # equal neighbours: that value's bits
            assert np.array_equal(_bits(r[nm + side][tie]), _bits(b[tie]))
        const = (ser == ser[0]).all(axis=0)                    # a constant series: mean, lower and upper are the constant's bits
        for k in (nm, nm + "_lower", nm + "_upper"):
            assert np.array_equal(_bits(r[k][const]), _bits(ser[0][const])), k
    if not fit:
        return r
    # the fit, against longdouble sums over the restatement's own means.  c = sum_n (P A) E: two products and N - 1 additions on
    # non-negative terms: dc = gamma(N + 1) c.  d = c - m adds u |d|; d^2 then has 2 |d| dd + dd^2 + u d^2; the sum of the K G terms
    # passes ceil(K / 64) - 1 + 6 + G roundings.  rmse = sqrt(sse / (K G)): half the relative error of sse (plus its square), one
    # rounding each for the division and the root
    Pm, Em, Am, m = r["P"].astype(LD), r["E"].astype(LD), r["A"].astype(LD), np.asarray(M, dtype=np.float64).astype(LD)
    c = (Pm * Am[None, :]) @ Em
    d = c - m
    dd = gamma(N + 1) * c + U * np.abs(d)
    nsum = (K + 63) // 64 - 1 + 6 + G
    sse = (d * d).sum()
    sse_err = float((2 * np.abs(d) * dd + dd * dd + U * d * d).sum() + gamma(nsum) * sse)
    rel = sse_err / float(sse)
    rmse = np.sqrt(sse / LD(K * G))
    assert abs(r["rmse"] - rmse) <= (0.5 * rel + rel * rel + 3 * U) * rmse, (r["rmse"], float(rmse), rel)
    # kl = sum mt log(mt / mh): mh carries c's gamma(N + 1), the quotient one more rounding, so the logarithm moves by gamma(N + 3)
    # (second order included); the project's log is within 1 ulp (oracle/orc_math.h), at most 2 u |log|; the product adds u |term|
    mt, mh = np.where(m < 1e-6, LD(1e-6), m), np.where(c < 1e-6, LD(1e-6), c)
    L = np.log(mt / mh)
    mt64, mh64 = np.where(np.asarray(M, dtype=np.float64) < 1e-6, 1e-6, M), np.where(c.astype(np.float64) < 1e-6, 1e-6, c.astype(np.float64))
    arg = mt64 / mh64
    assert (np.abs(R.oracle_log(arg) - np.log(arg.astype(LD))) <= 2 * U * np.abs(np.log(arg.astype(LD))) + 2.0 ** -1074).all()
    term = mt * L
    kl_err = float((mt * (gamma(N + 3) + 2 * U * np.abs(L)) + U * np.abs(term)).sum() + gamma(nsum) * np.abs(term).sum())
    assert abs(r["kl"] - term.sum()) <= kl_err, (r["kl"], float(term.sum()), kl_err)
    return r


@pytest.mark.parametrize("case", MC.MAP_CASES)
def test_map_restatement_against_plain_numpy(case, oracle_lib):
    for end, n in ((MC.T_END - 2, MC.N_RANGE), (MC.T_END, 10)):
        for ci in (0.95, None):
            _check_map(*_range(case, end, n), ci)


ROUTE_RANGES = ((1, 2150), (2, 2102), (3, 2103), (63, 2120), (64, 2150), (65, 2100), (1023, 2150), (1024, 2150), (1025, 2140),
                (2047, 2149), (2048, 2150), (2049, 2150), (2100, 2150))
ROUTE_CI = (0.95, 0.5, 0.999, 0.002)


def test_route_ranges_against_plain_numpy(oracle_lib):
    for n, end in ROUTE_RANGES:
        for ci in ROUTE_CI:
            _check_map(*_range("route", end, n), ci, fit=ci == 0.95)
    # the two chains of draws of k_map_quant cross at ci = 0.002 up to 65 samples (nlo + nhi > nu): each end then draws order
    # statistics the other has already drawn
    for n in (2, 3, 63, 64, 65):
        jlo, _, jhi, _, _ = R.order_stats(n, 0.002)
        assert min(jlo + 1, n - 1) + 1 + n - jhi > n


def test_the_chains_hold_what_the_gpu_tests_rely_on(oracle_lib):
    for (end, n), counts, used in (((38, 12), [3, 3, 3, 2, 1], "000010010001"), ((40, 10), [3, 3, 2, 1, 1], "1001000100")):
        Pw, Ew, Aw, M = _range("rank_n3", end, n)
        r = R.map_reference(Pw, Ew, Aw, M)
        assert r["n_patterns"] == 5 and r["top_counts"] == counts and "".join(map(str, r["used"])) == used and list(r["A"]) == [0.0, 1.0, 0.0]
        assert 2 <= r["n_used"] < n and (np.diff(np.where(r["used"])[0]) > 1).any()
    for end, n in ((38, 12), (40, 10)):
        Pw, Ew, Aw, M = _range("sbfi", end, n)
        r = R.map_reference(Pw, Ew, Aw, M)
        assert r["n_patterns"] == n and r["n_used"] == 1 and not r["A"].any() and not np.isnan(r["top_A"]).any()
    assert (np.asarray(_samples("normal")[3]) < 0).sum() == 13
    for end, n in ((38, 12), (40, 10)):
        Pw, Ew, Aw, M = _range("fix1", end, n)
        _, x, e = R.renormalised(Pw, Ew)
        rep = np.array([[len(np.unique(x[:, k, c])) for c in range(3)] for k in range(8)])
        assert (rep[:, 1] == 1).all() and (rep[:, [0, 2]] == n).all()
        Pw, Ew, Aw, M = _range("fixall_mh", end, n)
        _, x, e = R.renormalised(Pw, Ew)
        share, most = MC.repeated_values(e.reshape(n, -1))
        distinct = sorted(len(np.unique(e[:, i, g])) for i in range(3) for g in range(7))
        print(f"fixall_mh {end - n + 1}..{end}: {share:.3f} of the E elements repeat a value, one holds a value {most} times; distinct values per element {distinct}")
        assert share >= 0.25 and most >= 3 and distinct[-1] > 1
        assert share == (20 if n == 12 else 19) / 21.0
    P, E, A, M = _samples("route")
    assert (A == 1.0).all() and MC.repeated_values(np.stack([(P[s] / P[s].sum(0)).ravel() for s in range(50, 2150)]))[1] == 1


def test_neighbouring_expressions_give_other_bits(oracle_lib):
    """np.quantile for the bounds, np.sum (pairwise) or a mean in another order for the means: each differs from the restatement in
    some bit on these chains, so the device's bit comparison would notice a kernel that computed them"""
    n_q = n_m = 0
    for n, end in ((65, 2100), (1025, 2140), (2048, 2150)):
        Pw, Ew, Aw, M = _range("route", end, n)
        r = R.map_reference(Pw, Ew, Aw, M, 0.95)
        _, x, e = R.renormalised(Pw, Ew)
        n_q += int((_bits(np.quantile(x, 0.025, axis=0, method="linear")) != _bits(r["P_lower"])).sum() + (_bits(np.quantile(e, 0.975, axis=0, method="linear")) != _bits(r["E_upper"])).sum())
        # (np.sum along axis 0 of the [n][K][N] stack adds sample by sample, the restatement's order; an element's own series, contiguous,
        # is summed pairwise)
        psum = lambda a: np.ascontiguousarray(a.reshape(n, -1).T).sum(axis=1) / float(n)   # noqa: E731
        n_m += int((_bits(psum(x)) != _bits(r["P"].ravel())).sum() + (_bits(psum(e)) != _bits(r["E"].ravel())).sum())
    print(f"elements whose bits differ under np.quantile: {n_q}; under np.sum: {n_m}")
    assert n_q > 0 and n_m > 0
    # the small shapes too: some case tells the interpolation (1 - g) a + g b from a + (b - a) g
    diff = 0
    for case in ("pg_k8", "k7", "normal"):
        Pw, Ew, Aw, M = _range(case, 38, 12)
        r = R.map_reference(Pw, Ew, Aw, M, 0.95)
        _, x, e = R.renormalised(Pw, Ew)
        diff += int((_bits(np.quantile(e, 0.025, axis=0, method="linear")) != _bits(r["E_lower"])).sum())
    assert diff > 0


def _highest_column(C):
    """the solver with the other tie rule: the columns in falling order, so the highest wins among equals"""
    C = np.asarray(C)
    return (C.shape[1] - 1 - R.hungarian(C[:, ::-1])).astype(np.int32)


ASSIGN_CASES = [("pg_k8", R_, keep) for R_ in (1, 2, 3, 7) for keep in ("all", "gap")] + [("n70", 3, "gap"), ("n70", 150, "gap"), ("n70", 150, "all"),
                                                                                          ("rank_n3", 4, "mode"), ("sbfi", 25, "mode"), ("pg_k8", "tied", "all")]


def assign_inputs(case, Rn, keep, Pw, Aw, M):
    """ref, keep, used of an assignment case from the range's samples (shared with tests/test_gpu_assign_bits.py)"""
    K, N = Pw.shape[1:]
    ref = MC.tied_catalogue(Pw[-1]) if Rn == "tied" else MC.catalogue(K, Rn)
    if keep == "mode":
        tab, used = R.mode_of_A(Aw)
        return ref, np.array([int(ch) for ch in tab[0][0]], dtype=np.int32), used.astype(np.int32)
    return ref, (MC.keep_mask(N) if keep == "gap" else np.ones(N, dtype=np.int32)), MC.USED


@pytest.mark.parametrize("case,Rn,keep", ASSIGN_CASES)
def test_assign_restatement_against_scipy(case, Rn, keep, oracle_lib):
    from scipy.optimize import linear_sum_assignment
    Pw, Ew, Aw, M = _range(case, MC.T_END - 2, MC.N_RANGE)
    ref, kp, used = assign_inputs(case, Rn, keep, Pw, Aw, M)
    Pu = Pw[used == 1]
    MAP_P = R.series_mean(R.renormalised(Pu, Ew[used == 1])[1])
    r = R.assign_reference(Pu, ref, kp, MAP_P, 0.9)
    S, nk, Rr = r["cosines"].shape
    N = Pw.shape[2]
    if nk == 0:                                                # sbfi: the mode keeps nothing
        assert case == "sbfi" and not r["votes"].any() and (r["assigned"] == -1).all() and np.isnan(r["MAP_cosine"]).all()
        return
    sig = np.where(kp)[0]
    tr = nk > Rr
    n = min(nk, Rr)
    votes = np.zeros((N, Rr), dtype=LD)
    unique = 0
    for s in range(S):
        C = r["cosines"][s]
        # the cosines: dot and nn are sums of K non-negative products, the quotient and the root add 4 roundings: gamma(K + 5) in all
        Pk = Pu[s][:, sig].astype(LD)
        exact = (Pk.T @ ref.astype(LD)) / np.sqrt((Pk * Pk).sum(0)[:, None] * (ref.astype(LD) ** 2).sum(0)[None, :])
        assert (np.abs(C - exact) <= gamma(K_ := Pu.shape[1] + 5) * exact).all(), K_
        a = r["cols"][s]
        rows, cols = (np.arange(n), a) if not tr else (a, np.arange(n))
        assert len(set(a)) == n
        got = C[rows, cols].astype(LD).sum()
        ri, ci = linear_sum_assignment(-C)
        best = C[ri, ci].astype(LD).sum()
        # |cosine| <= 1; a potential is the result of at most n^2 additions of values below n, each rounding below n u: its error stays
        # below n^3 u, a reduced cost's below 3 n^3 u; complementary slackness up to that on the n chosen pairs and feasibility up to that
        # on the n pairs of any other assignment bound the gap by 6 n^4 u
        gap = 6.0 * n ** 4 * U
        assert abs(got - best) <= gap, (s, float(got), float(best))
        # unique: forbidding any one chosen pair lowers the optimum by more than the gap, so perturbing no cosine by a rounding changes it
        uniq = True
        for i, j in zip(ri, ci):
            D = C.copy()
            D[i, j] = -1e9
            r2, c2 = linear_sum_assignment(-D)
            uniq = uniq and D[r2, c2].astype(LD).sum() < best - gap
        if uniq:
            unique += 1
            assert set(zip(np.asarray(rows).tolist(), np.asarray(cols).tolist())) == set(zip(ri.tolist(), ci.tolist())), s
        votes[sig[rows], cols] += C[rows, cols]
    print(f"assign[{case}, R = {Rn}, keep = {keep}]: {S} samples, {nk} x {Rr}, the optimum unique in {unique}")
    assert unique == (0 if Rn == "tied" else S)
    # the votes: S additions in sample order of values in [0, 1]
    assert (np.abs(r["votes"] - votes) <= gamma(S) * votes).all()
    for nn_ in range(N):
        v = r["votes"][nn_]
        assert r["assigned"][nn_] == (int(np.argmax(v)) if (v > 0).any() else -1)
        if r["assigned"][nn_] >= 0:
            j, i = r["assigned"][nn_], list(sig).index(nn_)
            p = MAP_P[:, nn_].astype(LD)
            q = ref[:, j].astype(LD)
            mc = (p @ q) / np.sqrt((p @ p) * (q @ q))
            assert abs(r["MAP_cosine"][nn_] - mc) <= gamma(Pu.shape[1] + 5) * mc
            xs = r["cosines"][:, i, j]
            lo, hi = np.quantile(xs, [0.05, 0.95], method="linear")
            b = gamma(3) + gamma(4)                            # as for the bounds of bnmf_map; 1 - (1 - ci) / 2 is 0.95 to a rounding: one more u
            assert abs(r["lower_cosine"][nn_] - lo) <= b * xs.max() and abs(r["upper_cosine"][nn_] - hi) <= (b + S * U) * xs.max()
        else:
            assert np.isnan(r["MAP_cosine"][nn_]) and np.isnan(r["lower_cosine"][nn_])
    if Rn == "tied":
        # the duplicate with the lower index receives the votes, the other none; with the other rule it is the other way round
        assert r["votes"][:, [0, 1]].any() and not r["votes"][:, [2, 3]].any()
        hi = R.assign_reference(Pu, ref, kp, MAP_P, 0.9, solver=_highest_column)
        assert not np.array_equal(_bits(hi["votes"]), _bits(r["votes"])) and hi["votes"][:, [2, 3]].any()


def test_the_rectangular_solver_in_both_forms():
    from scipy.optimize import linear_sum_assignment
    rng = np.random.default_rng(2)
    mats = [rng.uniform(0, 1, size=s) for s in ((1, 1), (1, 7), (2, 3), (3, 70), (5, 150), (64, 65), (70, 150))]
    mats += [np.round(rng.uniform(0, 1, size=(4, 9)), 1), np.ones((3, 6)), np.eye(4)[:, [0, 0, 1, 1, 2, 3]]]
    for C in mats:
        a, b = R.hungarian(C), relabel_ref.hungarian_scalar(C)
        n = C.shape[0]
        assert np.array_equal(a, b) and len(set(a)) == n
        ri, ci = linear_sum_assignment(-C)
        assert abs(C[np.arange(n), a].sum() - C[ri, ci].sum()) <= 6.0 * n ** 4 * U + gamma(n) * n
    assert np.array_equal(R.hungarian(np.ones((3, 6))), [0, 1, 2])
    assert np.array_equal(R.hungarian(np.eye(4)[:, [0, 0, 1, 1, 2, 3]]), [0, 2, 4, 5])


def test_quantile7_is_the_bound_of_bnmf_map():
    x = np.random.default_rng(1).uniform(size=37)
    for ci in (0.9, 0.5):
        jlo, glo, jhi, ghi, _ = R.order_stats(37, ci)
        xs = np.sort(x)
        assert R.quantile7(x, 0.5 - ci / 2.0) == R.interpolate(xs, jlo, glo) and R.quantile7(x, 0.5 + ci / 2.0) == R.interpolate(xs, jhi, ghi)
    assert R.quantile7([3.0], 0.975) == 3.0 and R.quantile7([1.0, 2.0], 0.5) == 1.5
