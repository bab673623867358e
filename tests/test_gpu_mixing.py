"""Mixing diagnostics of a recorded range on the device (bnmf_mixing / bnmf_mixing_at, csrc/mixing.h) against the numerical spec restated
in numpy (tests/mixing_ref.py), BIT FOR BIT: the spec uses only correctly rounded operations in a fixed order, so there is no tolerance.
The reference is computed from bnmf_window of the same range.  Then the equivalences of the call and its refusals.

The cases (chains_for_mixing below builds the same chains from the CPU oracle, which is how their seeds and shapes were chosen: over
them the reference alone shows exit == 0, exit == 1 and a Gamma changed by the monotone clamp):
  s9      S = 9 < 64; lenP = lenE = 21 is no multiple of the 8-element tile; the range wraps the ring (window 16, iteration 40)
  s130    S = 130 of a 150-sample range: lanes with 3, 2 and a partial term
  k96     two-pass column sums      sbfi    used = bnmf_map's, keep = A_mode: the summary skips an excluded factor
  fixed   a fixed_P column: constant series (S = 9: for some the mean does not round back), NaN rows      normal  negative real data      ptn_mh  rings of the MH sweep      s4  the minimum"""
import ctypes as C

import numpy as np
import pytest

from mixing_ref import mixing_reference, mixing_summary, renormalised_series, ROWS

pytestmark = pytest.mark.gpu

USED12 = np.array([1, 1, 0, 1, 1, 1, 0, 0, 1, 1, 1, 1], dtype=np.int32)          # the gapped mask of the WAIC tests: 9 used
USED4 = np.array([0, 1, 0, 0, 1, 0, 0, 0, 1, 0, 0, 1], dtype=np.int32)
USED150 = np.array([0 if i % 15 in (3, 9) else 1 for i in range(150)], dtype=np.int32)   # 130 used
INFO = ("n_used", "n_half", "n_const", "n_ran_out", "n_low_ess", "n_high_rhat", "min_ess_P_at", "min_ess_E_at", "max_rhat_P_at", "max_rhat_E_at")
INFO_F = ("min_ess_P", "min_ess_E", "max_rhat_P", "max_rhat_E")

# name: K, G, N, likelihood, prior, MH, learning_rank, window, iterations, range length, used (None: bnmf_map's), fixed column
CASES = {
    "s9": (7, 7, 3, "poisson", "gamma", False, False, 16, 40, 12, USED12, None),
    "s130": (12, 10, 4, "poisson", "gamma", False, False, 160, 200, 150, USED150, None),
    "k96": (96, 6, 5, "poisson", "gamma", False, False, 16, 40, 12, USED12, None),
    "sbfi": (12, 10, 4, "poisson", "gamma", False, True, 16, 50, 12, None, None),     # iterations 37 .. 48: 7 share the mode of A, 0010
    "fixed": (12, 10, 3, "poisson", "gamma", False, False, 16, 40, 12, USED12, 1),
    "normal": (12, 10, 3, "normal", "exponential", False, False, 16, 40, 12, USED12, None),
    "ptn_mh": (96, 6, 5, "poisson", "truncnormal", True, False, 16, 40, 12, USED12, None),
    "s4": (7, 7, 3, "poisson", "gamma", False, False, 16, 40, 12, USED4, None),
}
BACK = 2          # every range ends 2 iterations before `iter`


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _data(case):
    from bayesnmf_amd.setup import synth_counts
    K, G, N, lk = CASES[case][:4]
    if lk == "normal":
        rng = np.random.default_rng(11)
        return np.asfortranarray(rng.gamma(1.0, 1.0, size=(K, 3)) @ rng.gamma(2.0, 2.0, size=(3, G)) + rng.normal(0.0, 0.5, size=(K, G)))
    M, _, _ = synth_counts(K, G, min(3, N), 21, mean_total=1500)
    if case == "sbfi":
        M[:, 7] = 0
    return M


def _temps():
    return np.concatenate([np.zeros(3), 10.0 ** np.linspace(-6, 0, 60), np.ones(100)])


def _create(case, cls=None, **kw):
    """the case's chain on the engine (or, cls = oracle.Oracle, on the CPU oracle: the same bits), before init"""
    from bayesnmf_amd.setup import apply_hyperprior_params
    K, G, N, lk, prior, MH, lr, W, T, n, used, fixed = CASES[case]
    M = _data(case)
    if cls is None:
        from bayesnmf_amd import Engine
        cls, kw = Engine, dict(window=W, **kw)
    c = cls(M, N, likelihood=lk, prior=prior, MH=MH, learning_rank=lr, seed=4, temperature=_temps() if lr else None, **kw)
    apply_hyperprior_params(c, prior, M, N)
    if fixed is not None and hasattr(c, "set_fixed"):
        P0 = np.asfortranarray(np.random.default_rng(17).gamma(1.0, 1.0, size=(K, N)))
        c.set("P", P0)
        c.set_fixed("P", (np.arange(N) == fixed).astype(np.int32))
    return c, M


def chains_for_mixing(case):
    """The case's used samples from the CPU oracle (no device): (Pw [S][K][N], Ew [S][N][G], Aw [S][N]).  Not for the fixed case: the
    oracle holds no column fixed by itself."""
    import oracle as O
    K, G, N, lk, prior, MH, lr, W, T, n, used, fixed = CASES[case]
    assert fixed is None
    o, _ = _create(case, O.Oracle, nthreads=4)
    o.init()
    P, E, A = [o.get("P")], [o.get("E")], [o.get("A").ravel()]
    for _ in range(T - 1):
        o.run(1, converged=MH)
        P.append(o.get("P")); E.append(o.get("E")); A.append(o.get("A").ravel())
    end = T - BACK
    its = np.arange(end - n + 1, end + 1)
    if used is None:
        keys = ["".join("1" if v else "0" for v in A[i - 1]) for i in its]
        tab = {k: keys.count(k) for k in sorted(set(keys))}
        mode = max(tab, key=lambda k: tab[k])                   # most frequent, ties in alphabetical order (get_mode)
        used = np.array([k == mode for k in keys], dtype=np.int32)
    sel = its[used == 1]
    return np.stack([P[i - 1] for i in sel]), np.stack([E[i - 1] for i in sel]), np.stack([A[i - 1] for i in sel])


_RUNS = {}


def _run(case):
    """the chain at its last iteration, its metric rows, the device's diagnostics of the range and the reference: made once per case"""
    if case in _RUNS:
        return _RUNS[case]
    K, G, N, lk, prior, MH, lr, W, T, n, used, fixed = CASES[case]
    e, M = _create(case)
    row1 = e.init()
    rows = np.vstack([row1[None, :], e.run(T - 1, converged=MH)])
    assert e.iter == T
    end = T - BACK
    keep = None
    if used is None:
        mp = e.map(n, None, end_iter=end)
        used, keep = mp["used"].astype(np.int32), (np.ravel(mp["A"]) != 0).astype(np.int32)
    first = end - n + 1
    sel = np.where(used == 1)[0]
    back = T - first + 1
    Pw, Ew = (np.stack([e.window(nm, back)[i] for i in sel]) for nm in ("P", "E"))
    xP, xE = renormalised_series(Pw, Ew)
    rP, rE = mixing_reference(xP), mixing_reference(xE)
    info = mixing_summary(rP["rows"], rE["rows"], K, N, len(sel), keep)
    dev = e.mixing(n, used=used, end_iter=end, keep=keep)
    _RUNS[case] = dict(e=e, M=M, rows=rows, end=end, n=n, used=used, keep=keep, refP=rP, refE=rE, info=info, dev=dev, S=len(sel))
    return _RUNS[case]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for r in _RUNS.values():
        r["e"].close()
    _RUNS.clear()


def _same(a, b, arrays=True):
    for k in INFO:
        assert a[k] == b[k], k
    for k in INFO_F:
        assert _bits(a[k]) == _bits(b[k]), k
    if arrays:
        for k in ROWS:
            for side in "PE":
                assert np.array_equal(_bits(a[f"{k}_{side}"]), _bits(b[f"{k}_{side}"])), (k, side)


@pytest.mark.parametrize("case", list(CASES))
def test_device_equals_the_restated_spec_bit_for_bit(case):
    r = _run(case)
    K, G, N = CASES[case][:3]
    dev = r["dev"]
    bad = []
    for side, ref, shp in (("P", r["refP"], (K, N)), ("E", r["refE"], (N, G))):
        for k in ROWS:
            want, got = ref[k].reshape(shp, order="F"), dev[f"{k}_{side}"]
            same = _bits(want) == _bits(got)
            same |= np.isnan(want) & np.isnan(got)
            if not same.all():
                with np.errstate(invalid="ignore", divide="ignore"):
                    bad.append((k, side, int((~same).sum()), float(np.nanmax(np.abs(got - want) / np.abs(want)))))
    print(f"mixing[{case}] S = {r['S']}: pairs P {sorted(set(r['refP']['pairs']))} E {sorted(set(r['refE']['pairs']))}, "
          f"exits {sorted(set(r['refP']['exit']) | set(r['refE']['exit']))}, clamped {r['refP']['n_clamped'] + r['refE']['n_clamped']}, mismatches {bad}")
    assert not bad, bad
    for k in INFO:
        assert dev[k] == r["info"][k], (k, dev[k], r["info"][k])
    for k in INFO_F:
        assert _bits(dev[k]) == _bits(r["info"][k]) or (np.isnan(dev[k]) and np.isnan(r["info"][k])), (k, dev[k], r["info"][k])
    assert dev["n_used"] == r["S"] and dev["n_half"] == r["S"] // 2


def test_the_cases_cover_both_exits_and_the_clamp():
    exits, clamped = set(), 0
    for case in CASES:
        r = _run(case)
        for ref in (r["refP"], r["refE"]):
            exits |= set(ref["exit"][ref["pairs"] > 0])
            clamped += ref["n_clamped"]
    assert exits == {0.0, 1.0} and clamped > 0


def test_sbfi_summary_skips_the_excluded_factor():
    r = _run("sbfi")
    K, G, N = CASES["sbfi"][:3]
    assert r["keep"] is not None and (r["keep"] == 0).sum() >= 1, "no factor is excluded: the case does not exercise keep"
    assert r["S"] >= 4
    full = mixing_summary(r["refP"]["rows"], r["refE"]["rows"], K, N, r["S"], None)
    assert any(full[k] != r["info"][k] for k in INFO[2:6]) or full["min_ess_E"] != r["info"]["min_ess_E"], "keep changes nothing here"
    for k in ("min_ess_P_at", "max_rhat_P_at"):
        assert r["keep"][r["dev"][k] // K] == 1
    for k in ("min_ess_E_at", "max_rhat_E_at"):
        assert r["keep"][r["dev"][k] % N] == 1


def test_a_fixed_column_is_constant():
    r = _run("fixed")
    K, G, N = CASES["fixed"][:3]
    dev = r["dev"]
    # the renormalised fixed column of P is constant; its row of E moves (E is sampled)
    assert dev["n_const"] >= K and (dev["pairs_P"][:, 1] == 0).all() and (dev["exit_P"][:, 1] == 0).all()
    for k in ("ess", "mcse", "rhat"):
        assert np.isnan(dev[f"{k}_P"][:, 1]).all()
    # (mean and var are written as the formulas give them: canon(x) / S need not round back to x, which leaves var at rounding noise)
    assert (dev["var_P"][:, 1] <= (4 * np.finfo(float).eps * dev["mean_P"][:, 1]) ** 2).all() and np.isfinite(dev["mean_P"]).all()
    assert dev["min_ess_P_at"] // K != 1 and np.isfinite(dev["min_ess_P"]) and dev["max_rhat_P_at"] // K != 1


@pytest.mark.parametrize("case", ["s9", "s130", "k96", "normal"])
def test_equivalent_calls_give_the_same_bits(case):
    r = _run(case)
    e, n = r["e"], r["n"]
    _same(r["dev"], e.mixing(n, used=r["used"], end_iter=r["end"], keep=r["keep"]))                     # a second call
    _same(r["dev"], e.mixing(n, used=r["used"], end_iter=r["end"], keep=r["keep"], arrays=False), False)   # arrays NULL: the same info
    _same(e.mixing(10), e.mixing(10, end_iter=e.iter))                                                 # bnmf_mixing is bnmf_mixing_at(iter)
    _same(e.mixing(10), e.mixing(10, used=np.ones(10, dtype=np.int32)))                                # NULL is all ones
    _same(e.mixing(10), e.mixing(10, keep=np.ones(e.N, dtype=np.int32)))
    _same(e.mixing(n, end_iter=r["end"]), e.mixing(n, used=np.ones(n, dtype=np.int32), end_iter=r["end"]))


@pytest.mark.parametrize("case", ["k96", "normal"])
def test_the_mean_is_bnmf_maps_mean(case):
    """row 1 against code that exists today: with every sample used, bnmf_map's renormalised means (the sum in sample order instead of
    the canonical one: within 1e-12 relative)"""
    r = _run(case)
    e, n = r["e"], r["n"]
    mp = e.map(n, None, end_iter=r["end"])
    assert mp["used"].all()
    m = e.mixing(n, end_iter=r["end"])
    assert np.allclose(m["mean_P"], mp["P"], rtol=1e-12, atol=0) and np.allclose(m["mean_E"], mp["E"], rtol=1e-12, atol=0)


@pytest.mark.parametrize("case", ["k96", "normal"])
def test_a_reopened_chain_gives_the_same_diagnostics(case, tmp_path):
    r = _run(case)
    path = str(tmp_path / "state.bin")
    r["e"].save_state(path)
    c, _ = _create(case)
    assert c.load_state(path) == CASES[case][8]
    _same(r["dev"], c.mixing(r["n"], used=r["used"], end_iter=r["end"], keep=r["keep"]))
    c.close()


def test_refusals():
    from bayesnmf_amd import Engine
    from bayesnmf_amd.engine import lib, BnmfMixingInfo, BnmfError
    from bayesnmf_amd.setup import apply_hyperprior_params
    r = _run("s9")
    e, M, L, W = r["e"], r["M"], lib(), CASES["s9"][7]
    info = BnmfMixingInfo()
    ip = C.POINTER(C.c_int32)

    def err():
        msg = L.bnmf_last_error().decode()
        assert msg
        return msg
    assert L.bnmf_mixing(e._h, 10, None, None, None, None, None) == -1 and "null" in err()                       # BNMF_EINVAL
    assert L.bnmf_mixing_at(e._h, e.iter, 10, None, None, None, None, None) == -1 and "null" in err()
    u = np.ones(10, dtype=np.int32); u[6] = 2
    assert L.bnmf_mixing(e._h, 10, u.ctypes.data_as(ip), None, None, None, C.byref(info)) == -1 and "used[6] = 2" in err()
    k = np.ones(3, dtype=np.int32); k[1] = -1
    assert L.bnmf_mixing_at(e._h, e.iter, 10, None, k.ctypes.data_as(ip), None, None, C.byref(info)) == -1 and "keep[1] = -1" in err()
    u = np.zeros(10, dtype=np.int32); u[[1, 4, 8]] = 1
    assert L.bnmf_mixing(e._h, 10, u.ctypes.data_as(ip), None, None, None, C.byref(info)) == -2 and "3 used samples" in err()   # BNMF_ESIZE
    assert "at least 4" in err()
    assert L.bnmf_mixing(e._h, 3, None, None, None, None, C.byref(info)) == -2 and err()
    # the range rule of bnmf_map_at: iterations [max(1, iter - window + 1), iter]
    assert L.bnmf_mixing_at(e._h, e.iter + 1, 5, None, None, None, None, C.byref(info)) == -2 and "are kept" in err()
    assert L.bnmf_mixing_at(e._h, e.iter, W + 1, None, None, None, None, C.byref(info)) == -2 and "are kept" in err()
    assert L.bnmf_mixing_at(e._h, e.iter - W + 3, 5, None, None, None, None, C.byref(info)) == -2 and "are kept" in err()
    assert L.bnmf_mixing(e._h, W + 1, None, None, None, None, C.byref(info)) == -2 and err()
    with pytest.raises(BnmfError, match="used has 3 entries"):
        e.mixing(10, used=[1, 1, 1])
    with pytest.raises(BnmfError, match="keep has 2 entries"):
        e.mixing(10, keep=[1, 1])
    # window = 0: BNMF_ESTATE
    z = Engine(M, 3, prior="gamma", seed=4, window=0)
    apply_hyperprior_params(z, "gamma", M, 3)
    z.init(); z.run(5)
    assert L.bnmf_mixing(z._h, 4, None, None, None, None, C.byref(info)) == -7 and "window = 0" in err()
    assert L.bnmf_mixing_at(z._h, z.iter, 4, None, None, None, None, C.byref(info)) == -7 and "window = 0" in err()
    z.close()
    # the handle is usable afterwards: the same bits as before the refusals
    _same(r["dev"], e.mixing(r["n"], used=r["used"], end_iter=r["end"]))


@pytest.mark.parametrize("case", ["k96", "ptn_mh", "sbfi"])
def test_the_call_is_read_only_for_the_chain(case):
    """a chain that called mixing continues with the bits of one that never did: the arrays and the metric rows of the next 5 iterations"""
    r = _run(case)
    MH, T = CASES[case][5], CASES[case][8]
    b, _ = _create(case)
    row1 = b.init()
    rows_b = np.vstack([row1[None, :], b.run(T - 1, converged=MH)])
    assert np.array_equal(_bits(rows_b), _bits(r["rows"]))
    more_a, more_b = r["e"].run(5, converged=MH), b.run(5, converged=MH)
    assert np.array_equal(_bits(more_a), _bits(more_b))
    for nm in ("P", "E", "A"):
        assert np.array_equal(_bits(r["e"].get(nm)), _bits(b.get(nm))), nm
    b.close()
    _RUNS.pop(case)["e"].close()                                                 # (this case's chain has moved on)
