"""Residual structure of a recorded range on the device (bnmf_residuals / bnmf_residuals_at, csrc/residuals.h) against the numerical spec
restated in numpy float64 (tests/residuals_ref.py, written from DESIGN.md 26): every output and every info field of every case bit for
bit, NaN compared as NaN, no tolerance — the operations are + - * /, sqrt, |.|, comparisons and whole numbers only; then the
equivalences and the refusals.

Every case keeps window = 16 samples and runs to iteration 40, so the kept range wraps the ring; the range is the 12 samples that end 2
iterations before `iter` (the _at form in the middle of the window), with a `used` mask that has gaps (tests/test_gpu_contrast.py's
recipe).  The shapes are the smallest that reach each path of the kernels:
  K = 8, G = 200, N = 5: the base shape, one tile of 8 types (two tiles of 4 in the other form), one block of positions;
  G = 1,023 / 1,024 / 1,025 / 1,100 with an include that has holes: the member list ends just below, at and just above a block of 1,024
  positions of canonB, and crosses it with a ragged last block;
  K = 1, 7, 65, 96, 97: below one tile, one short of it, one past eight tiles, whole tiles only, one past them (the clamped rows);
  N = 1; N = 40 (more factors than stay in registers: the column of E read through the caches in either form); m = 2;
  a rank-learning chain with N = 20 (samples with A[n] = 0); real-valued Normal data with negative cells (sigmasq); data with an
  all-zero mutation type (the 1e-6 clip where the fit gets there).
Both forms (BNMF_RES_FORM) and batches of 1 and 5 samples (BNMF_RES_BATCH) must give the same bits.

No chain state here produces a flat sample (a trace that is not > 0 and finite), and the rings cannot be written from outside, so none is
forced: the rule is pinned on the restatement and on the library's host routine (tests/test_residuals_host.py)."""
import ctypes as C

import numpy as np
import pytest

import residuals_ref as R

pytestmark = pytest.mark.gpu

W, T_END, N_RANGE = 16, 40, 12
USED = np.array([1, 1, 0, 1, 1, 1, 0, 0, 1, 1, 1, 1], dtype=np.int32)
ARRAYS = ("gram", "type", "component", "tumour", "series")
INFO = ("n_used", "n_flat", "n_included", "n_left_out", "n_steps", "n_biased", "n_overdispersed", "worst_type_at", "min_agreement_at", "lambda", "share", "move",
        "mean_share", "min_agreement", "worst_type", "max_dispersion")

# name: K, G, N, likelihood, prior, learning_rank, seed
CASES = {
    "g200": (8, 200, 5, "poisson", "gamma", False, 4),
    "g1023": (6, 1023, 3, "poisson", "gamma", False, 4),
    "g1024": (6, 1024, 3, "poisson", "gamma", False, 4),
    "g1025": (6, 1025, 3, "poisson", "gamma", False, 4),
    "g1100": (6, 1100, 3, "poisson", "gamma", False, 4),
    "k1": (1, 70, 2, "poisson", "gamma", False, 4),
    "k7": (7, 70, 3, "poisson", "gamma", False, 4),
    "k65": (65, 70, 3, "poisson", "gamma", False, 4),
    "k96": (96, 70, 3, "poisson", "gamma", False, 4),
    "k97": (97, 70, 3, "poisson", "gamma", False, 4),
    "n1": (8, 40, 1, "poisson", "gamma", False, 4),
    "n40": (8, 40, 40, "poisson", "gamma", False, 4),
    "sbfi": (96, 8, 20, "poisson", "gamma", True, 14),
    "normal": (12, 10, 3, "normal", "exponential", False, 4),
    "zero": (8, 60, 3, "poisson", "gamma", False, 4),
}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _data(case):
    from bayesnmf_amd.setup import synth_counts
    K, G, N, lk, *_ = CASES[case]
    if lk == "normal":
        rng = np.random.default_rng(11)
        M = np.asfortranarray(rng.gamma(1.0, 1.0, size=(K, 3)) @ rng.gamma(0.5, 1.0, size=(3, G)) + rng.normal(0.0, 0.5, size=(K, G)))
        assert (M < 0).any()
        return M
    M, _, _ = synth_counts(K, G, min(3, N), 21, mean_total=1500 if K > 1 else 96 * 40)
    if case == "zero":
        M[5, :] = 0
    return M


def _temps():
    return np.concatenate([np.ones(20), np.zeros(3), 10.0 ** np.linspace(-6, 0, 60), np.ones(100)])


_RUNS = {}


def _run(case):
    """the chain at iteration 40 and the used samples of the range: once per case"""
    if case in _RUNS:
        return _RUNS[case]
    from bayesnmf_amd import Engine
    from bayesnmf_amd.setup import apply_hyperprior_params
    K, G, N, lk, prior, lr, seed = CASES[case]
    M = _data(case)
    e = Engine(M, N, likelihood=lk, prior=prior, learning_rank=lr, seed=seed, window=W, temperature=_temps() if lr else None)
    apply_hyperprior_params(e, prior, M, N)
    e.init()
    e.run(T_END - 1)
    assert e.iter == T_END
    end = T_END - 2
    back = T_END - (end - N_RANGE + 1) + 1
    sel = np.where(USED == 1)[0]
    win = {nm: np.stack([e.window(nm, back)[i] for i in sel]) for nm in (("P", "E", "A", "sigmasq") if lk == "normal" else ("P", "E", "A"))}
    sig = win["sigmasq"].reshape(len(sel), G) if lk == "normal" else None
    _RUNS[case] = dict(e=e, end=end, samples=(win["P"], win["E"], win["A"].reshape(len(sel), N)), sigmasq=sig, M=M, G=G, N=N, K=K, back=back)
    return _RUNS[case]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for r in _RUNS.values():
        r["e"].close()
    _RUNS.clear()


def _ref(r, **kw):
    return R.residuals_reference(*r["samples"], r["M"], sigmasq=r["sigmasq"], **kw)


def _differences(tag, a, b, arrays=ARRAYS, info=INFO):
    """the names of the outputs of a that are not b's, bit for bit with NaN equal to NaN (printed with the first place they differ)"""
    bad = []
    for k in arrays:
        x, y = np.asarray(a[k], dtype=np.float64), np.asarray(b[k], dtype=np.float64)
        if x.shape != y.shape:
            print(f"residuals[{tag}] {k}: shapes {x.shape} and {y.shape}")
            bad.append(k)
            continue
        nx, ny = np.isnan(x), np.isnan(y)
        ne = (nx != ny) | (~nx & ~ny & (_bits(x).reshape(x.shape) != _bits(y).reshape(y.shape)))
        if ne.any():
            i = tuple(np.argwhere(ne)[0])
            print(f"residuals[{tag}] {k}: {int(ne.sum())} of {ne.size} differ, first at {i}: {x[i]!r} against {y[i]!r}")
            bad.append(k)
    for k in info:
        fa, fb = float(a[k]), float(b[k])
        if not ((np.isnan(fa) and np.isnan(fb)) or _bits(fa) == _bits(fb)):
            print(f"residuals[{tag}] {k}: {a[k]!r} against {b[k]!r}")
            bad.append(k)
    return bad


def _holes(G):
    inc = np.ones(G, dtype=np.int32)
    inc[[0, 3, G // 2, G - 1]] = 0
    return inc


@pytest.mark.parametrize("case,steps,holes", [("g200", 100, False), ("g200", 1, False), ("g1023", 100, False), ("g1024", 100, False), ("g1025", 100, False),
                                              ("g1025", 100, True), ("g1100", 100, True), ("k1", 100, False), ("k7", 100, False), ("k65", 100, False),
                                              ("k96", 1, False), ("k96", 100, False), ("k97", 100, False), ("n1", 100, False), ("n40", 100, False),
                                              ("sbfi", 100, False), ("normal", 100, False), ("normal", 1, True), ("zero", 100, False)])
def test_every_output_is_the_restatement_bit_for_bit(case, steps, holes, monkeypatch):
    r = _run(case)
    e, G, K = r["e"], r["G"], r["K"]
    inc = _holes(G) if holes else None
    kw = dict(used=USED, end_iter=r["end"], include=inc, n_steps=steps, max_dispersion=1.5)
    ref = _ref(r, include=inc, n_steps=steps, max_dispersion=1.5)
    dev = e.residuals(N_RANGE, **kw)
    A = r["samples"][2]
    print(f"residuals[{case}, steps {steps}] S {dev['n_used']} flat {dev['n_flat']} m {dev['n_included']} share {dev['share']!r} mean share {dev['mean_share']!r} "
          f"move {dev['move']!r} min agreement {dev['min_agreement']!r} dispersion {dev['type'][3].min()!r}..{dev['type'][3].max()!r} overdispersed "
          f"{dev['n_overdispersed']} biased {dev['n_biased']}; samples that exclude a factor {int((A == 0).any(axis=1).sum())}")
    assert dev["gram"].shape == (K, K) and dev["type"].shape == (5, K) and dev["component"].shape == (4, K) and dev["tumour"].shape == (3, G)
    assert dev["series"].shape == (5, 9) and dev["n_used"] == 9
    assert np.array_equal(_bits(dev["gram"]), _bits(dev["gram"].T))
    bad = _differences(f"{case} steps {steps}", dev, ref)
    if holes:
        assert np.isnan(dev["tumour"][:, inc == 0]).all() and dev["n_left_out"] == 4 and dev["n_included"] == G - 4
    if case == "sbfi":
        assert (A == 0).any(), "no used sample that excludes a factor"
    if case == "zero":
        fit = np.einsum("skn,sng->skg", r["samples"][0] * A[:, None, :], r["samples"][1])
        print(f"residuals[zero] the smallest fit of the all-zero type {fit[:, 5].min()!r}: the clip is {'reached' if fit[:, 5].min() < 1e-6 else 'not reached'}")
    # the other form and small batches of samples through the scratch: the same bits
    for form, batch in (("1", None), (None, "1"), ("1", "5"), ("0", "5")):
        if form:
            monkeypatch.setenv("BNMF_RES_FORM", form)
        if batch:
            monkeypatch.setenv("BNMF_RES_BATCH", batch)
        bad += _differences(f"{case} steps {steps}, form {form}, batch {batch}", e.residuals(N_RANGE, **kw), ref)
        monkeypatch.delenv("BNMF_RES_FORM", raising=False)
        monkeypatch.delenv("BNMF_RES_BATCH", raising=False)
    assert not bad, bad


def test_two_included_tumours():
    r = _run("g200")
    e, G = r["e"], r["G"]
    inc = np.zeros(G, dtype=np.int32)
    inc[[17, 150]] = 1
    dev = e.residuals(N_RANGE, include=inc, used=USED, end_iter=r["end"], n_steps=10)
    assert dev["n_included"] == 2 and dev["n_left_out"] == G - 2 and not np.isnan(dev["tumour"][:, [17, 150]]).any()
    assert not _differences("m = 2", dev, _ref(r, include=inc, n_steps=10))


@pytest.mark.parametrize("case", ["g200", "normal"])
def test_equivalent_calls_give_the_same_bits(case):
    r = _run(case)
    e, end, G = r["e"], r["end"], r["G"]
    kw = dict(n_steps=20)
    first = e.residuals(N_RANGE, used=USED, end_iter=end, **kw)
    assert not _differences("again", first, e.residuals(N_RANGE, used=USED, end_iter=end, **kw))
    assert not _differences("at", e.residuals(10, **kw), e.residuals(10, end_iter=e.iter, **kw))              # bnmf_residuals is bnmf_residuals_at(iter)
    assert not _differences("ones", e.residuals(10, **kw), e.residuals_at(e.iter, 10, used=np.ones(10, dtype=np.int32), include=np.ones(G, dtype=np.int32), **kw))
    s2 = np.zeros(N_RANGE, dtype=np.int32)
    s2[[2, 9]] = 1                                                                                             # S = 2
    two = e.residuals(N_RANGE, used=s2, end_iter=end, **kw)
    assert two["n_used"] == 2
    names = ("P", "E", "A", "sigmasq") if case == "normal" else ("P", "E", "A")
    win = {nm: np.stack([e.window(nm, r["back"])[i] for i in (2, 9)]) for nm in names}
    sig = win["sigmasq"].reshape(2, G) if case == "normal" else None
    assert not _differences("S = 2", two, R.residuals_reference(win["P"], win["E"], win["A"].reshape(2, -1), r["M"], sigmasq=sig, n_steps=20))
    # every output NULL: the info fields are the same
    from bayesnmf_amd.engine import lib, BnmfResidualsInfo
    L, ip = lib(), C.POINTER(C.c_int32)
    info = BnmfResidualsInfo()
    assert L.bnmf_residuals_at(e._h, end, N_RANGE, USED.ctypes.data_as(ip), None, 20, 2.0, None, None, None, None, None, C.byref(info)) == 0
    assert not _differences("all NULL", {k: getattr(info, k) for k in INFO}, first, arrays=())


def test_refusals():
    from bayesnmf_amd import Engine
    from bayesnmf_amd.engine import lib, BnmfResidualsInfo, BnmfError
    from bayesnmf_amd.setup import apply_hyperprior_params, synth_counts
    r = _run("g200")
    e, G, N, L = r["e"], r["G"], r["N"], lib()
    info = BnmfResidualsInfo()
    ip = C.POINTER(C.c_int32)
    before = e.residuals(N_RANGE, used=USED, end_iter=r["end"], n_steps=5)

    def err():
        msg = L.bnmf_last_error().decode()
        assert msg
        return msg

    def call(n=10, used=None, include=None, steps=5, md=2.0, inf=info, at=None, h=None):
        pt = lambda v: None if v is None else v.ctypes.data_as(ip)  # noqa: E731
        f = None if inf is None else C.byref(inf)
        h = e._h if h is None else h
        rest = (pt(used), pt(include), steps, md, None, None, None, None, None, f)
        return L.bnmf_residuals(h, n, *rest) if at is None else L.bnmf_residuals_at(h, at, n, *rest)

    for at in (None, e.iter):
        assert call(inf=None, at=at) == -1 and "null" in err()                                       # BNMF_EINVAL
        u = np.ones(10, dtype=np.int32); u[6] = 2
        assert call(used=u, at=at) == -1 and "used[6] = 2" in err()
        inc = np.ones(G, dtype=np.int32); inc[64] = -1
        assert call(include=inc, at=at) == -1 and "include[64] = -1" in err()
        for bad in (0, 10001):
            assert call(steps=bad, at=at) == -1 and f"n_steps = {bad}" in err() and "1..10000" in err()
        for bad in (float("nan"), -0.5):
            assert call(md=bad, at=at) == -1 and "max_dispersion" in err()
        u = np.zeros(10, dtype=np.int32); u[3] = 1
        assert call(used=u, at=at) == -2 and "1 used sample" in err()                                # BNMF_ESIZE
        inc = np.zeros(G, dtype=np.int32); inc[5] = 1
        assert call(include=inc, at=at) == -2 and "1 included tumour" in err()
        assert call(include=np.zeros(G, dtype=np.int32), at=at) == -2 and "0 included tumours" in err()
    assert call(n=W + 1) == -2 and err()
    assert call(n=5, at=e.iter + 1) == -2 and "are kept" in err()
    assert call(n=3, at=e.iter - W + 1) == -2 and "are kept" in err()
    with pytest.raises(BnmfError, match="used has 3 entries"):
        e.residuals(10, used=[1, 1, 1])
    with pytest.raises(BnmfError, match="include has shape"):
        e.residuals(10, include=[1, 1, 1])
    # window = 0: BNMF_ESTATE
    M, _, _ = synth_counts(8, 6, N, 21, mean_total=1500)
    z = Engine(M, N, prior="gamma", seed=4, window=0)
    apply_hyperprior_params(z, "gamma", M, N)
    z.init(); z.run(5)
    assert call(n=3, h=z._h) == -7 and "window = 0" in err()
    assert call(n=3, at=z.iter, h=z._h) == -7 and "window = 0" in err()
    z.close()
    # more mutation types than BNMF_RES_MAX_K: BNMF_ESIZE, the limit named (the power kernel's LDS is sized by it)
    Mb = np.asfortranarray(np.random.default_rng(3).poisson(2.0, size=(2049, 4)).astype(np.int32))
    big = Engine(Mb, 1, prior="gamma", seed=4, window=4)
    apply_hyperprior_params(big, "gamma", Mb, 1)
    big.init(); big.run(3)
    assert call(n=3, h=big._h) == -2 and "K = 2049 mutation types, at most 2048" in err()
    assert call(n=3, at=big.iter, h=big._h) == -2 and "K = 2049 mutation types, at most 2048" in err()
    big.close()
    assert L.bnmf_version() == 100
    # the handle is usable afterwards: the same bits as before the refusals
    assert not _differences("afterwards", before, e.residuals(N_RANGE, used=USED, end_iter=r["end"], n_steps=5))


def test_the_call_is_read_only_for_the_chain():
    """a chain that calls residuals mid-run continues with the bits of a twin that never did"""
    from bayesnmf_amd import Engine
    from bayesnmf_amd.setup import apply_hyperprior_params
    K, G, N, lk, prior, lr, seed = CASES["normal"]
    M = _data("normal")
    a, b = (Engine(M, N, likelihood=lk, prior=prior, seed=seed, window=W) for _ in range(2))
    for c in (a, b):
        apply_hyperprior_params(c, prior, M, N)
        c.init(); c.run(20)
    a.residuals(12, n_steps=10)
    ra, rb = a.run(10), b.run(10)
    assert np.array_equal(_bits(ra), _bits(rb))
    for nm in ("P", "E", "A", "sigmasq"):
        assert np.array_equal(_bits(a.get(nm)), _bits(b.get(nm))), nm
    a.close(); b.close()
