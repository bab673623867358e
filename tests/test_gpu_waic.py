"""WAIC of a recorded range on the device (bnmf_waic / bnmf_waic_at, csrc/waic.h) against its numerical spec restated in numpy
(tests/waic_ref.py, evaluated in longdouble), the fixed order of its reductions, its equivalences and its refusals.

Every case keeps window = 16 samples and runs to iteration 40, so the kept range wraps the ring; the range is the 12 samples that end
2 iterations before `iter`, with a `used` mask that has gaps.

Tolerance (per quantity): 16 x |reference in float64 - reference in longdouble|, with a floor of 64 eps x the sum, over the cells and
samples that enter the quantity, of the magnitudes of the terms of l_s (|m log mh| + mh + lgamma(m + 1); Normal: |log sd| +
log sqrt(2 pi) + z^2 / 2): the device's dlog is within 1 ulp and its lgamma table within 6e-15 of libm (dmath.h).  se_elpd is a
function of the cells' elpd with |d se / d elpd_kg| <= sqrt(n / (n - 1)), so the total's tolerance bounds it too; n_high_var must lie
between the counts of the reference's p_kg -+ its tolerance above 0.4.  The measured errors are printed (run with -s) and recorded in
DESIGN.md 12."""
import ctypes as C

import numpy as np
import pytest

from waic_ref import waic_reference, canon64_colsum, seq_sum

pytestmark = pytest.mark.gpu

W, T_END, N_RANGE = 16, 40, 12
USED = np.array([1, 1, 0, 1, 1, 1, 0, 0, 1, 1, 1, 1], dtype=np.int32)
EPS = np.finfo(np.float64).eps
INFO = ("lppd", "p_waic", "elpd_waic", "waic", "se_elpd", "mean_loglik")

# name: K, G, N, likelihood, prior, MH, learning_rank
CASES = {
    "pg_k8": (8, 7, 3, "poisson", "gamma", False, False),             # K < 64; odd G: a lone last column
    "pg_k96": (96, 6, 5, "poisson", "gamma", False, False),           # a last pass of 32 rows
    "pg_k130": (130, 5, 2, "poisson", "gamma", False, False),         # three passes: a second chunk of rows, 2 of them
    "sbfi": (12, 10, 4, "poisson", "gamma", False, True),             # samples with A[n] = 0; a data column of zeros
    "normal": (12, 10, 3, "normal", "exponential", False, False),     # real-valued data, negative cells: the sigmasq ring
    "ptn_mh": (96, 6, 5, "poisson", "truncnormal", True, False),      # rings recorded by the MH sweep
    "pg_k1536": (1536, 4, 2, "poisson", "gamma", False, False),       # twelve chunks of rows
}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _data(case):
    from bayesnmf_amd.setup import synth_counts
    K, G, N, lk, *_ = CASES[case]
    if lk == "normal":
        rng = np.random.default_rng(11)
        return np.asfortranarray(rng.gamma(1.0, 1.0, size=(K, 3)) @ rng.gamma(2.0, 2.0, size=(3, G)) + rng.normal(0.0, 0.5, size=(K, G)))
    M, _, _ = synth_counts(K, G, min(3, N), 21, mean_total=1500)
    if case == "sbfi":
        M[:, 7] = 0
    return M


def _temps():
    return np.concatenate([np.zeros(3), 10.0 ** np.linspace(-6, 0, 60), np.ones(100)])


def _create(case):
    from bayesnmf_amd import Engine
    K, G, N, lk, prior, MH, lr = CASES[case]
    M = _data(case)
    return Engine(M, N, likelihood=lk, prior=prior, MH=MH, learning_rank=lr, seed=4, window=W, temperature=_temps() if lr else None), M


def _fresh(case):
    from bayesnmf_amd.setup import apply_hyperprior_params
    e, M = _create(case)
    apply_hyperprior_params(e, CASES[case][4], M, CASES[case][2])
    row1 = e.init()
    return e, M, row1


_RUNS = {}


def _run(case):
    """the chain at iteration 40, its metric rows, the device's WAIC of the range and both references: made once per case"""
    if case in _RUNS:
        return _RUNS[case]
    K, G, N, lk, prior, MH, lr = CASES[case]
    e, M, row1 = _fresh(case)
    rows = np.vstack([row1[None, :], e.run(T_END - 1, converged=MH)])
    assert e.iter == T_END
    end = T_END - 2
    first = end - N_RANGE + 1
    back = T_END - first + 1
    sel = np.where(USED == 1)[0]
    win = {nm: np.stack([e.window(nm, back)[i] for i in sel]) for nm in ("P", "E", "A") + (("sigmasq",) if lk == "normal" else ())}
    samples = (win["P"], win["E"], win["A"].reshape(len(sel), N), win.get("sigmasq"))
    ref64 = waic_reference(*samples, M, lk, np.float64)
    refld = waic_reference(*samples, M, lk, np.longdouble)
    dev = e.waic(N_RANGE, used=USED, end_iter=end, pointwise=True)
    _RUNS[case] = dict(e=e, M=M, rows=rows, end=end, first=first, samples=samples, ref64=ref64, refld=refld, dev=dev)
    return _RUNS[case]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for r in _RUNS.values():
        r["e"].close()
    _RUNS.clear()


def _tol(r64, rld, mag):
    return np.maximum(16.0 * np.abs(np.asarray(r64, dtype=np.longdouble) - rld).astype(np.float64), 64.0 * EPS * np.asarray(mag, dtype=np.float64))


@pytest.mark.parametrize("case", list(CASES))
def test_against_the_longdouble_reference(case):
    r = _run(case)
    K, G, N, lk, *_ = CASES[case]
    dev, r64, rld = r["dev"], r["ref64"], r["refld"]
    mag = np.asarray(rld["mag"], dtype=np.float64)
    if case == "sbfi":
        assert (r["samples"][2] == 0).any(), "no used sample excludes a factor: the case does not exercise A[n] = 0"
    checks = [("lppd_cell", dev["lppd_cell"], "lppd_cell", mag), ("p_cell", dev["p_waic_cell"], "p_cell", mag),
              ("lppd_col", dev["lppd_col"], "lppd_col", mag.sum(0)), ("p_col", dev["p_waic_col"], "p_col", mag.sum(0)),
              ("mean_col", dev["mean_loglik_col"], "mean_col", mag.sum(0))]
    checks += [(k, dev[k], k, mag.sum()) for k in ("lppd", "p_waic", "elpd_waic", "mean_loglik", "se_elpd")]
    bad = []
    for name, got, key, m in checks:
        tol = _tol(r64[key], rld[key], m)
        err = np.abs(np.asarray(got, dtype=np.longdouble) - rld[key]).astype(np.float64)
        print(f"waic[{case}] {name}: max err {np.max(err):.3e}, max err/tol {np.max(err / tol):.3e}, "
              f"max |float64 - longdouble| {np.max(np.abs(np.asarray(r64[key], dtype=np.longdouble) - rld[key]).astype(np.float64)):.3e}")
        if not (err <= tol).all():
            bad.append(name)
    assert not bad, bad
    assert dev["waic"] == -2.0 * dev["elpd_waic"] and dev["n_used"] == int(USED.sum())
    ptol = _tol(r64["p_cell"], rld["p_cell"], mag)
    p = np.asarray(rld["p_cell"], dtype=np.float64)
    assert int((p - ptol > 0.4).sum()) <= dev["n_high_var"] <= int((p + ptol > 0.4).sum())
    print(f"waic[{case}] n_high_var {dev['n_high_var']} of {K * G}, cells clipped at 1e-6 in some sample: "
          f"{int((np.einsum('skn,sn,sng->skg', r['samples'][0], r['samples'][2], r['samples'][1]) < 1e-6).any(0).sum()) if lk == 'poisson' else 0}")


@pytest.mark.parametrize("case", list(CASES))
def test_reductions_are_in_the_canonical_order(case):
    """col is the canonical W = 64 reduction of cell and the totals the sequential sums of col, bit for bit: whatever the tiling"""
    dev = _run(case)["dev"]
    K, G = CASES[case][:2]
    assert np.array_equal(_bits(dev["lppd_col"]), _bits(canon64_colsum(dev["lppd_cell"])))
    assert np.array_equal(_bits(dev["p_waic_col"]), _bits(canon64_colsum(dev["p_waic_cell"])))
    assert _bits(dev["lppd"]) == _bits(seq_sum(dev["lppd_col"])) and _bits(dev["p_waic"]) == _bits(seq_sum(dev["p_waic_col"]))
    assert _bits(dev["mean_loglik"]) == _bits(seq_sum(dev["mean_loglik_col"]))
    elpd = dev["lppd_cell"] - dev["p_waic_cell"]
    t3, t4, n = seq_sum(canon64_colsum(elpd)), seq_sum(canon64_colsum(elpd * elpd)), float(K) * float(G)
    assert _bits(dev["elpd_waic"]) == _bits(t3)
    var = (t4 - t3 * (t3 / n)) / (n - 1.0)
    assert _bits(dev["se_elpd"]) == _bits(np.sqrt(n * max(var, 0.0)))
    assert dev["n_high_var"] == int((dev["p_waic_cell"] > 0.4).sum())


def _same(a, b, pointwise=True):
    for k in INFO:
        assert _bits(a[k]) == _bits(b[k]), k
    assert a["n_used"] == b["n_used"] and a["n_high_var"] == b["n_high_var"]
    if pointwise:
        for k in ("lppd_col", "p_waic_col", "mean_loglik_col", "lppd_cell", "p_waic_cell"):
            assert np.array_equal(_bits(a[k]), _bits(b[k])), k


@pytest.mark.parametrize("case", ["pg_k96", "sbfi", "normal"])
def test_equivalent_calls_give_the_same_bits(case):
    r = _run(case)
    e = r["e"]
    _same(r["dev"], e.waic(N_RANGE, used=USED, end_iter=r["end"], pointwise=True))              # a second call
    _same(r["dev"], e.waic(N_RANGE, used=USED, end_iter=r["end"], pointwise=False), False)      # pointwise off
    _same(e.waic(10, pointwise=True), e.waic(10, end_iter=e.iter, pointwise=True))              # bnmf_waic is bnmf_waic_at(iter)
    _same(e.waic(10, pointwise=True), e.waic(10, used=np.ones(10, dtype=np.int32), pointwise=True))   # NULL is all ones
    _same(e.waic(N_RANGE, end_iter=r["end"], pointwise=True),
          e.waic(N_RANGE, used=np.ones(N_RANGE, dtype=np.int32), end_iter=r["end"], pointwise=True))


@pytest.mark.parametrize("case", ["pg_k96", "normal"])
def test_a_reopened_chain_gives_the_same_waic(case, tmp_path):
    r = _run(case)
    path = str(tmp_path / "state.bin")
    r["e"].save_state(path)
    c, _ = _create(case)
    assert c.load_state(path) == T_END
    _same(r["dev"], c.waic(N_RANGE, used=USED, end_iter=r["end"], pointwise=True))
    c.close()


@pytest.mark.parametrize("case", list(CASES))
def test_mean_loglik_is_the_mean_of_the_metric_rows(case):
    """info.mean_loglik against code that exists today: the mean, over the used iterations, of the loglikelihood column of the
    bnmf_run metric rows (row i is iteration i + 1), under the tolerance rule of the reference test"""
    r = _run(case)
    its = r["first"] + np.where(USED == 1)[0]
    assert np.array_equal(r["rows"][its - 1, 0], its)
    ll = r["rows"][its - 1, 3]
    want = np.mean(ll.astype(np.longdouble))
    tol = float(_tol(r["ref64"]["mean_loglik"], r["refld"]["mean_loglik"], np.asarray(r["refld"]["mag"], dtype=np.float64).sum()))
    err = float(abs(np.longdouble(r["dev"]["mean_loglik"]) - want))
    print(f"waic[{case}] mean_loglik {r['dev']['mean_loglik']!r} metric rows {float(want)!r} err {err:.3e} tol {tol:.3e}")
    assert err <= tol


def test_refusals():
    from bayesnmf_amd import Engine
    from bayesnmf_amd.engine import lib, BnmfWaicInfo, BnmfError
    from bayesnmf_amd.setup import apply_hyperprior_params
    r = _run("pg_k8")
    e, M, L = r["e"], r["M"], lib()
    info = BnmfWaicInfo()
    ip = C.POINTER(C.c_int32)

    def err():
        msg = L.bnmf_last_error().decode()
        assert msg
        return msg
    assert L.bnmf_waic(e._h, 10, None, None, None, None) == -1 and "null" in err()                       # BNMF_EINVAL
    assert L.bnmf_waic_at(e._h, e.iter, 10, None, None, None, None) == -1 and "null" in err()
    u = np.ones(10, dtype=np.int32); u[6] = 2
    assert L.bnmf_waic(e._h, 10, u.ctypes.data_as(ip), None, None, C.byref(info)) == -1 and "used[6] = 2" in err()
    u[6] = -1
    assert L.bnmf_waic_at(e._h, e.iter, 10, u.ctypes.data_as(ip), None, None, C.byref(info)) == -1 and "used[6] = -1" in err()
    u = np.zeros(10, dtype=np.int32); u[3] = 1
    assert L.bnmf_waic(e._h, 10, u.ctypes.data_as(ip), None, None, C.byref(info)) == -2 and "1 used sample" in err()   # BNMF_ESIZE
    assert L.bnmf_waic(e._h, 1, None, None, None, C.byref(info)) == -2 and err()
    # the range rule of bnmf_map_at: iterations [max(1, iter - window + 1), iter]
    assert L.bnmf_waic_at(e._h, e.iter + 1, 5, None, None, None, C.byref(info)) == -2 and "are kept" in err()
    assert L.bnmf_waic_at(e._h, e.iter, W + 1, None, None, None, C.byref(info)) == -2 and "are kept" in err()
    assert L.bnmf_waic_at(e._h, e.iter - W + 1, 3, None, None, None, C.byref(info)) == -2 and "are kept" in err()
    assert L.bnmf_waic(e._h, W + 1, None, None, None, C.byref(info)) == -2 and err()
    with pytest.raises(BnmfError, match="used has 3 entries"):
        e.waic(10, used=[1, 1, 1])
    # window = 0: BNMF_ESTATE
    z = Engine(M, 3, prior="gamma", seed=4, window=0)
    apply_hyperprior_params(z, "gamma", M, 3)
    z.init(); z.run(5)
    assert L.bnmf_waic(z._h, 3, None, None, None, C.byref(info)) == -7 and "window = 0" in err()
    assert L.bnmf_waic_at(z._h, z.iter, 3, None, None, None, C.byref(info)) == -7 and "window = 0" in err()
    z.close()
    # the handle is usable afterwards: the same bits as before the refusals
    _same(r["dev"], e.waic(N_RANGE, used=USED, end_iter=r["end"], pointwise=True))


@pytest.mark.parametrize("case", ["pg_k96", "ptn_mh", "sbfi"])
def test_the_call_is_read_only_for_the_chain(case):
    """a chain that calls waic mid-run continues with the bits of one that does not; a chain saved and reopened gives the same WAIC"""
    r = _run(case)
    MH = CASES[case][5]
    b, _, row1 = _fresh(case)
    rows_b = np.vstack([row1[None, :], b.run(T_END - 1, converged=MH)])
    assert np.array_equal(_bits(rows_b), _bits(r["rows"]))
    more_a, more_b = r["e"].run(10, converged=MH), b.run(10, converged=MH)       # a called waic at iteration 40, b never did
    assert np.array_equal(_bits(more_a), _bits(more_b))
    for nm in ("P", "E", "A"):
        assert np.array_equal(_bits(r["e"].get(nm)), _bits(b.get(nm))), nm
    b.close()
    _RUNS.pop(case)["e"].close()                                                 # (this case's chain has moved on)
