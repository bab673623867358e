"""Exposures of new tumours under the recorded signatures on the device (bnmf_project / bnmf_project_at, csrc/project.h) against the
numerical spec restated in numpy float64 (tests/project_ref.py, written from DESIGN.md 17): every output and every info field of
every case bit for bit, no tolerance — the operations are multiply, add, IEEE division, square root and compare only; then the
equivalences and the refusals.

Every case keeps window = 16 samples and runs to iteration 40, so the kept range wraps the ring; the range is the 12 samples that end
2 iterations before `iter`, with a `used` mask that has gaps (tests/test_gpu_attribution.py's); n_steps = 25.  The shapes are the
smallest that reach each path: one partial wave; a full wave and a partial one; K > 128; the rank-learning chain of
tests/test_gpu_attribution.py (several factors excluded per sample, and one used sample with A = 0, whose exposures are all 0 and
whose cosine is NaN); N = 40, where e and g live in the LDS; K = 700 with N = 30, where x exceeds the LDS whichever form is asked
for; rings recorded by the MH sweep.  X comes from synth_counts, with column 0 made fractional, column 1 all zero and the last
column a repeat of column 0.

NaN: IEEE 754 leaves the sign and payload of a generated NaN to the implementation (x86 makes 0 / 0 negative, gfx950 positive), so a
NaN is compared as "a NaN" (one canonical pattern); every other value by its 64 bits."""
import ctypes as C

import numpy as np
import pytest

import project_ref as R

pytestmark = pytest.mark.gpu

W, T_END, N_RANGE, STEPS = 16, 40, 12, 25
USED = np.array([1, 1, 0, 1, 1, 1, 0, 0, 1, 1, 1, 1], dtype=np.int32)
ARRAYS = ("load", "fit", "series", "exposures")
INFO = ("n_used", "n_steps", "n_present", "min_load", "total", "max_rel_change", "min_cosine", "min_cosine_at")

# name: K, G, N, prior, MH, learning_rank, seed, J
CASES = {
    "pg_k8": (8, 7, 3, "gamma", False, False, 4, 7),                 # one partial wave
    "pg_k96": (96, 6, 5, "gamma", False, False, 4, 70),              # a full wave and a partial one
    "pg_k130": (130, 5, 2, "gamma", False, False, 4, 5),
    "sbfi": (96, 8, 20, "gamma", False, True, 14, 9),                # samples with A[n] = 0, one with A = 0; NT = 24 with 4 idle places
    "lds_eg": (12, 5, 40, "gamma", False, False, 4, 66),             # e and g in the LDS; a second workgroup of 2 lanes
    "unstaged": (700, 3, 30, "gamma", False, False, 4, 3),           # x exceeds 160 KB: never staged
    "ptn_mh": (96, 6, 5, "truncnormal", True, False, 4, 6),          # rings recorded by the MH sweep
}


def _bits(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = a.view(np.uint64).copy()
    b[np.isnan(a)] = np.uint64(0x7FF8000000000000)
    return b


def _new_tumours(K, J, seed=33):
    from bayesnmf_amd.setup import synth_counts
    X = np.asfortranarray(synth_counts(K, J, 3, seed, mean_total=1200)[0], dtype=np.float64)
    X[:, 0] = X[:, 0] * 0.5 + 0.25                                   # fractional values
    if J > 1:
        X[:, 1] = 0.0                                                # an all-zero tumour
    if J > 2:
        X[:, J - 1] = X[:, 0]                                        # the same tumour at two places
    return X


def _temps():
    return np.concatenate([np.ones(20), np.zeros(3), 10.0 ** np.linspace(-6, 0, 60), np.ones(100)])


def _fresh(case):
    from bayesnmf_amd import Engine
    from bayesnmf_amd.setup import synth_counts, apply_hyperprior_params
    K, G, N, prior, MH, lr, seed, _ = CASES[case]
    M, _, _ = synth_counts(K, G, min(3, N), 21, mean_total=1500)
    e = Engine(M, N, likelihood="poisson", prior=prior, MH=MH, learning_rank=lr, seed=seed, window=W, temperature=_temps() if lr else None)
    apply_hyperprior_params(e, prior, M, N)
    row1 = e.init()
    return e, row1


_RUNS = {}


def _run(case):
    """the chain at iteration 40, its metric rows, the device's projection of the new tumours and the restatement: made once per case"""
    if case in _RUNS:
        return _RUNS[case]
    K, G, N, prior, MH, lr, _, J = CASES[case]
    e, row1 = _fresh(case)
    rows = np.vstack([row1[None, :], e.run(T_END - 1, converged=MH)])
    assert e.iter == T_END
    end = T_END - 2
    back = T_END - (end - N_RANGE + 1) + 1
    sel = np.where(USED == 1)[0]
    win = {nm: np.stack([e.window(nm, back)[i] for i in sel]) for nm in ("P", "A")}
    samples = (win["P"], win["A"].reshape(len(sel), N))
    X = _new_tumours(K, J)
    ref = R.project_reference(*samples, X, STEPS, min_load=1.0)
    dev = e.project(N_RANGE, X, used=USED, end_iter=end, n_steps=STEPS, exposures=True)
    _RUNS[case] = dict(e=e, rows=rows, end=end, samples=samples, X=X, ref=ref, dev=dev)
    return _RUNS[case]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for r in _RUNS.values():
        r["e"].close()
    _RUNS.clear()


def _differences(tag, a, b, arrays=ARRAYS):
    """the names of the outputs of a that are not b's, bit for bit (printed with the first place they differ)"""
    bad = []
    for k in arrays:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if x.shape != y.shape:
            print(f"project[{tag}] {k}: shapes {x.shape} and {y.shape}")
            bad.append(k)
            continue
        ne = _bits(x) != _bits(y)
        if ne.any():
            i = tuple(np.argwhere(ne)[0])
            print(f"project[{tag}] {k}: {int(ne.sum())} of {ne.size} differ, first at {i}: {x[i]!r} against {y[i]!r}")
            bad.append(k)
    for k in INFO:
        if _bits(float(a[k])) != _bits(float(b[k])):
            print(f"project[{tag}] {k}: {a[k]!r} against {b[k]!r}")
            bad.append(k)
    return bad


def _same(a, b, arrays=ARRAYS):
    assert not _differences("equivalence", a, b, arrays)


@pytest.mark.parametrize("case", list(CASES))
def test_every_output_is_the_restatement_bit_for_bit(case, oracle_lib):
    r = _run(case)
    K, G, N, *_, J = CASES[case]
    dev, ref = r["dev"], r["ref"]
    part = ref["part"]
    print(f"project[{case}] S {dev['n_used']} total {dev['total']!r} (sum of X {float(r['X'].sum())!r}) present {dev['n_present']} of {N * J}; "
          f"max_rel_change {dev['max_rel_change']!r} min_cosine {dev['min_cosine']!r} at {dev['min_cosine_at']}; "
          f"factors taking part per sample {part.sum(axis=1).tolist()}")
    if case == "sbfi":
        assert (part.sum(axis=1) == 0).any(), "no used sample with A = 0"
        assert ((part.sum(axis=1) > 0) & (part.sum(axis=1) < N)).any(), "no used sample excludes only some factors"
        s0 = int(np.where(part.sum(axis=1) == 0)[0][0])
        assert (dev["exposures"][s0] == 0).all() and np.isnan(ref["cosines"][s0]).all() and np.isnan(dev["cosine"]).all()
    assert dev["n_used"] == int(USED.sum()) and dev["load"].shape == (4, N, J) and dev["fit"].shape == (3, J)
    assert dev["series"].shape == (dev["n_used"], N) and dev["exposures"].shape == (dev["n_used"], N, J)
    bad = _differences(case, dev, ref)
    assert not bad, bad
    # the same tumour at two places has the same bits; the all-zero tumour has no exposure
    assert np.array_equal(_bits(dev["exposures"][:, :, J - 1]), _bits(dev["exposures"][:, :, 0]))
    assert np.array_equal(_bits(dev["load"][:, :, J - 1]), _bits(dev["load"][:, :, 0])) and np.array_equal(_bits(dev["fit"][:, J - 1]), _bits(dev["fit"][:, 0]))
    assert (dev["exposures"][:, :, 1] == 0).all() and np.isnan(dev["cosine"][1])


@pytest.mark.parametrize("case", ["pg_k96", "sbfi", "lds_eg"])
def test_equivalent_calls_give_the_same_bits(case, monkeypatch):
    r = _run(case)
    e, end, X = r["e"], r["end"], r["X"]
    kw = dict(used=USED, end_iter=end, n_steps=STEPS, exposures=True)
    _same(r["dev"], e.project(N_RANGE, X, **kw))                                                      # a second call
    _same(r["dev"], e.project(N_RANGE, X, used=USED, end_iter=end, n_steps=STEPS), ARRAYS[:3])       # exposures = NULL
    _same(e.project(10, X, n_steps=3, exposures=True), e.project(10, X, end_iter=e.iter, n_steps=3, exposures=True))   # bnmf_project is bnmf_project_at(iter)
    _same(e.project(10, X, n_steps=3), e.project(10, X, used=np.ones(10, dtype=np.int32), n_steps=3), ARRAYS[:3])       # NULL is all ones
    for batch in ("1", "5"):                                                                          # 9 samples in 9 and in 2 batches
        monkeypatch.setenv("BNMF_PROJ_BATCH", batch)
        _same(r["dev"], e.project(N_RANGE, X, **kw))
    monkeypatch.delenv("BNMF_PROJ_BATCH")
    for stage in ("0", "1"):                                                                          # x through the caches, x staged in the LDS
        monkeypatch.setenv("BNMF_PROJ_STAGE", stage)
        _same(r["dev"], e.project(N_RANGE, X, **kw))
    monkeypatch.delenv("BNMF_PROJ_STAGE")
    # the tumours in another order: every column keeps its bits
    perm = np.roll(np.arange(X.shape[1]), 3)
    p = e.project(N_RANGE, np.asfortranarray(X[:, perm]), **kw)
    assert np.array_equal(_bits(p["exposures"]), _bits(r["dev"]["exposures"][:, :, perm])) and np.array_equal(_bits(p["fit"]), _bits(r["dev"]["fit"][:, perm]))
    assert np.array_equal(_bits(p["load"]), _bits(r["dev"]["load"][:, :, perm]))
    # J = 1
    one = e.project(N_RANGE, np.asfortranarray(X[:, :1]), **kw)
    assert np.array_equal(_bits(one["exposures"][:, :, 0]), _bits(r["dev"]["exposures"][:, :, 0])) and np.array_equal(_bits(one["fit"][:, 0]), _bits(r["dev"]["fit"][:, 0]))
    assert one["min_cosine_at"] == (-1 if np.isnan(one["fit"][0, 0]) else 0) and _bits(one["min_cosine"]) == _bits(one["fit"][0, 0])
    # load, fit, series and exposures all NULL: the info fields alone
    from bayesnmf_amd.engine import lib, BnmfProjectInfo
    info = BnmfProjectInfo()
    dp = C.POINTER(C.c_double)
    assert lib().bnmf_project_at(e._h, end, N_RANGE, USED.ctypes.data_as(C.POINTER(C.c_int32)), X.ctypes.data_as(dp), X.shape[1], STEPS, 1.0,
                                 None, None, None, None, C.byref(info)) == 0
    for k in INFO:
        assert _bits(float(getattr(info, k))) == _bits(float(r["dev"][k])), k
    # another min_load moves row 3 and n_present alone
    hi = e.project(N_RANGE, X, used=USED, end_iter=end, n_steps=STEPS, min_load=50.0)
    assert np.array_equal(_bits(hi["load"][:3]), _bits(r["dev"]["load"][:3])) and np.array_equal(_bits(hi["series"]), _bits(r["dev"]["series"]))
    assert np.array_equal(hi["p_present"], (r["dev"]["exposures"] >= 50.0).mean(axis=0)) and hi["min_load"] == 50.0


def test_identical_samples_have_variance_zero():
    """every column of P fixed: all samples share one P, so every sample's exposures are the same bits and the variance row is 0.0"""
    from bayesnmf_amd import Engine
    from bayesnmf_amd.setup import synth_counts, apply_hyperprior_params
    K, G, N, J = 24, 6, 3, 5
    M, P_true, _ = synth_counts(K, G, N, 21, mean_total=1500)
    e = Engine(M, N, likelihood="poisson", prior="gamma", seed=4, window=W)
    apply_hyperprior_params(e, "gamma", M, N)
    e.set("P", np.asfortranarray(np.random.default_rng(3).gamma(1.0, 1.0, size=(K, N))))
    e.set_fixed("P", np.ones(N, dtype=np.int32))
    e.init(); e.run(9)
    r = e.project(8, _new_tumours(K, J), n_steps=STEPS, exposures=True)
    assert (r["exposures"][:, :, 0] > 0).any()
    for s in range(1, 8):
        assert np.array_equal(_bits(r["exposures"][s]), _bits(r["exposures"][0])), s
    assert np.array_equal(_bits(r["load_var"]), _bits(np.zeros((N, J)))) and np.array_equal(_bits(r["load_mean"]), _bits(r["exposures"][0]))
    e.close()


def test_refusals():
    from bayesnmf_amd import Engine
    from bayesnmf_amd.engine import lib, BnmfProjectInfo, BnmfError
    from bayesnmf_amd.setup import synth_counts, apply_hyperprior_params
    r = _run("pg_k8")
    e, L, X = r["e"], lib(), r["X"]
    K, J = X.shape
    info = BnmfProjectInfo()
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    xp = X.ctypes.data_as(dp)

    def err():
        msg = L.bnmf_last_error().decode()
        assert msg
        return msg

    def call(h=None, last_n=10, used=None, x=xp, j=J, steps=5, min_load=1.0, inf=info, at=None):
        h = e._h if h is None else h
        tail = (used, x, j, steps, min_load, None, None, None, None, None if inf is None else C.byref(inf))
        return L.bnmf_project(h, last_n, *tail) if at is None else L.bnmf_project_at(h, at, last_n, *tail)
    for at in (None, e.iter):
        assert call(inf=None, at=at) == -1 and "null" in err()                                       # BNMF_EINVAL
        assert call(x=None, at=at) == -1 and "null" in err()
        u = np.ones(10, dtype=np.int32); u[6] = 2
        assert call(used=u.ctypes.data_as(ip), at=at) == -1 and "used[6] = 2" in err()
        assert call(j=0, at=at) == -1 and "J = 0" in err()
        for bad in (0, -3, 100001):
            assert call(steps=bad, at=at) == -1 and f"n_steps = {bad}" in err()
        for bad in (float("nan"), float("inf"), -float("inf"), -0.5):
            assert call(min_load=bad, at=at) == -1 and "min_load" in err()
        for bad in (float("nan"), float("inf"), -1.0):
            Xb = X.copy(order="F"); Xb[3, 2] = bad; Xb[5, 4] = bad
            assert call(x=Xb.ctypes.data_as(dp), at=at) == -1 and "X[3, 2]" in err()
        u = np.zeros(10, dtype=np.int32); u[3] = 1
        assert call(used=u.ctypes.data_as(ip), at=at) == -2 and "1 used sample" in err()             # BNMF_ESIZE
        assert call(last_n=1, at=at) == -2 and err()
    # the range rule of bnmf_map_at: iterations [max(1, iter - window + 1), iter]
    assert call(last_n=5, at=e.iter + 1) == -2 and "are kept" in err()
    assert call(last_n=W + 1, at=e.iter) == -2 and "are kept" in err()
    assert call(last_n=3, at=e.iter - W + 1) == -2 and "are kept" in err()
    assert call(last_n=W + 1) == -2 and err()
    with pytest.raises(BnmfError, match="used has 3 entries"):
        e.project(10, X, used=[1, 1, 1])
    with pytest.raises(BnmfError, match="rows are needed"):
        e.project(10, X[:-1])
    M, _, _ = synth_counts(K, 7, 3, 21, mean_total=1500)
    # window = 0: BNMF_ESTATE
    z = Engine(M, 3, prior="gamma", seed=4, window=0)
    apply_hyperprior_params(z, "gamma", M, 3)
    z.init(); z.run(5)
    assert call(h=z._h, last_n=3) == -7 and "window = 0" in err()
    assert call(h=z._h, last_n=3, at=z.iter) == -7 and "window = 0" in err()
    z.close()
    # the Normal likelihood: BNMF_EMODEL
    n = Engine(np.asfortranarray(M, dtype=np.float64), 3, likelihood="normal", prior="exponential", seed=4, window=W)
    apply_hyperprior_params(n, "exponential", M, 3)
    n.init(); n.run(5)
    assert call(h=n._h, last_n=3) == -6 and "Normal" in err() and "out of scope" in err()
    assert call(h=n._h, last_n=3, at=n.iter) == -6 and "Normal" in err()
    n.close()
    # more factors than BNMF_PROJ_MAX_N: BNMF_ESIZE, the limit named
    big = Engine(M, 129, prior="gamma", seed=4, window=4)
    apply_hyperprior_params(big, "gamma", M, 129)
    big.init(); big.run(3)
    assert call(h=big._h, last_n=3) == -2 and "BNMF_PROJ_MAX_N = 128" in err()
    big.close()
    assert L.bnmf_version() == 100
    assert call(min_load=0.0) == 0 and info.n_present == CASES["pg_k8"][2] * J                        # min_load = 0 is allowed: every exposure counts
    # the handle is usable afterwards: the same bits as before the refusals
    _same(r["dev"], e.project(N_RANGE, X, used=USED, end_iter=r["end"], n_steps=STEPS, exposures=True))


@pytest.mark.parametrize("case", ["pg_k96", "ptn_mh", "sbfi"])
def test_the_call_is_read_only_for_the_chain(case):
    """a chain that calls project mid-run continues with the bits of a twin that never did"""
    r = _run(case)
    MH = CASES[case][4]
    b, row1 = _fresh(case)
    rows_b = np.vstack([row1[None, :], b.run(T_END - 1, converged=MH)])
    assert np.array_equal(_bits(rows_b), _bits(r["rows"]))
    more_a, more_b = r["e"].run(10, converged=MH), b.run(10, converged=MH)       # a called project at iteration 40, b never did
    assert np.array_equal(_bits(more_a), _bits(more_b))
    for nm in ("P", "E", "A"):
        assert np.array_equal(_bits(r["e"].get(nm)), _bits(b.get(nm))), nm
    b.close()
    _RUNS.pop(case)["e"].close()                                                 # (this case's chain has moved on)
