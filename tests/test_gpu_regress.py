"""Regression of exposures on tumour covariates over a recorded range on the device (bnmf_regress / bnmf_regress_at, csrc/regress.h)
against the numerical spec restated in numpy float64 (tests/regress_ref.py, written from DESIGN.md 20): every output and every info field
of every case bit for bit, NaN compared as NaN, no tolerance — the operations are + - * /, sqrt, comparisons and integer counts only;
then the equivalences and the refusals.

Every case keeps window = 16 samples and runs to iteration 40, so the kept range wraps the ring; the range is the 12 samples that end
2 iterations before `iter`, with a `used` mask that has gaps (tests/test_gpu_contrast.py's recipe).  The shapes are the smallest that
reach each path: 2,120 tumours of which 2,049 are included in a fixed shuffle (two full blocks of 1,024 and a block of one member) and 71
left out; G = 70 with 65 included (one block, one element into the second round of its accumulators); m = Q + 1, the smallest fit; Q = 1,
2, 5 and 16 at G = 70 for a partial and four full column tiles of either form; N = 5, 12, 30 and 40 for partial and full factor tiles; the
rank-learning chain of test_gpu_attribution (samples with A[n] = 0 and one with A = 0: r2 is NaN); real-valued data with negative cells
(sqrt of a negative load is NaN through the spec); rings recorded by the MH sweep."""
import ctypes as C

import numpy as np
import pytest

import regress_ref as R

pytestmark = pytest.mark.gpu

W, T_END, N_RANGE = 16, 40, 12
USED = np.array([1, 1, 0, 1, 1, 1, 0, 0, 1, 1, 1, 1], dtype=np.int32)
ARRAYS = ("coef", "fit", "coef_series", "r2_series")
INTS = ("n_used", "Q", "n_included", "n_left_out", "n_blocks", "min_pivot_at")
REALS = ("credible_interval", "min_pivot_ratio")
CI = 0.9


def _design(G, Q, seed=3):
    """ones, an age-like covariate in whole years, a 0 / 1 covariate, then standard normal columns"""
    rng = np.random.default_rng(seed)
    cols = [np.ones(G), np.round(60.0 + 12.0 * rng.standard_normal(G)), (rng.uniform(size=G) < 0.4).astype(np.float64)]
    cols += [rng.standard_normal(G) for _ in range(max(Q - 3, 0))]
    return np.asfortranarray(np.stack(cols[:Q], axis=1))


def _include(G, m, seed=17):
    """m of the G tumours in a fixed shuffle"""
    inc = np.zeros(G, dtype=np.int32)
    inc[np.random.default_rng(seed).permutation(G)[:m]] = 1
    return inc


# chain: K, G, N, likelihood, prior, MH, learning_rank, seed
CHAINS = {
    "blocks": (8, 2120, 3, "poisson", "gamma", False, False, 4),
    "g70": (96, 70, 5, "poisson", "gamma", False, False, 4),
    "n12": (8, 70, 12, "poisson", "gamma", False, False, 4),
    "n30": (8, 70, 30, "poisson", "gamma", False, False, 4),
    "n40": (8, 70, 40, "poisson", "gamma", False, False, 4),
    "sbfi": (96, 8, 20, "poisson", "gamma", False, True, 14),                      # samples with A[n] = 0, one with A = 0
    "normal": (12, 10, 3, "normal", "exponential", False, False, 4),               # real-valued data, negative cells
    "ptn_mh": (96, 6, 5, "poisson", "truncnormal", True, False, 4),                # rings recorded by the MH sweep
}
# case: chain, Q, include (None = all)
CASES = {
    "three_blocks": ("blocks", 3, _include(2120, 2049)),
    "m65": ("g70", 3, _include(70, 65)),
    "m_q_plus_1": ("g70", 3, _include(70, 4)),
    "q1": ("g70", 1, None),
    "q2": ("g70", 2, _include(70, 64)),
    "q5": ("g70", 5, None),
    "q16": ("g70", 16, None),
    "n12": ("n12", 3, None),
    "n30": ("n30", 4, _include(70, 66)),
    "n40": ("n40", 3, None),
    "sbfi": ("sbfi", 3, None),
    "normal": ("normal", 3, None),
    "ptn_mh": ("ptn_mh", 2, None),
}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _data(chain):
    from bayesnmf_amd.setup import synth_counts
    K, G, N, lk, *_ = CHAINS[chain]
    if lk == "normal":
        rng = np.random.default_rng(11)
        return np.asfortranarray(rng.gamma(1.0, 1.0, size=(K, 3)) @ rng.gamma(0.5, 1.0, size=(3, G)) + rng.normal(0.0, 0.5, size=(K, G)))   # small means: some cells below 0
    M, _, _ = synth_counts(K, G, min(3, N), 21, mean_total=1500)
    return M


def _temps():
    return np.concatenate([np.ones(20), np.zeros(3), 10.0 ** np.linspace(-6, 0, 60), np.ones(100)])


def _create(chain):
    from bayesnmf_amd import Engine
    K, G, N, lk, prior, MH, lr, seed = CHAINS[chain]
    M = _data(chain)
    return Engine(M, N, likelihood=lk, prior=prior, MH=MH, learning_rank=lr, seed=seed, window=W, temperature=_temps() if lr else None), M


def _fresh(chain):
    from bayesnmf_amd.setup import apply_hyperprior_params
    e, M = _create(chain)
    apply_hyperprior_params(e, CHAINS[chain][4], M, CHAINS[chain][2])
    row1 = e.init()
    return e, M, row1


_CHAINS, _RUNS = {}, {}


def _chain(chain):
    """the chain at iteration 40, its metric rows and the used samples of the range: made once per chain"""
    if chain in _CHAINS:
        return _CHAINS[chain]
    K, G, N, lk, prior, MH, lr, _ = CHAINS[chain]
    e, M, row1 = _fresh(chain)
    rows = np.vstack([row1[None, :], e.run(T_END - 1, converged=MH)])
    assert e.iter == T_END
    end = T_END - 2
    first = end - N_RANGE + 1
    back = T_END - first + 1
    sel = np.where(USED == 1)[0]
    win = {nm: np.stack([e.window(nm, back)[i] for i in sel]) for nm in ("P", "E", "A")}
    samples = (win["P"], win["E"], win["A"].reshape(len(sel), N))
    _CHAINS[chain] = dict(e=e, M=M, rows=rows, end=end, samples=samples)
    return _CHAINS[chain]


def _run(case):
    """the chain, the device's regression over the range and the restatement: made once per case"""
    if case in _RUNS:
        return _RUNS[case]
    chain, Q, inc = CASES[case]
    ch = _chain(chain)
    D = _design(CHAINS[chain][1], Q)
    ref = R.regress_reference(*ch["samples"], D, include=inc, credible_interval=CI)
    dev = ch["e"].regress(N_RANGE, D, include=inc, used=USED, end_iter=ch["end"], credible_interval=CI, series=True)
    _RUNS[case] = dict(ch, chain=chain, D=D, inc=inc, ref=ref, dev=dev)
    return _RUNS[case]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for r in _CHAINS.values():
        r["e"].close()
    _CHAINS.clear()
    _RUNS.clear()


def _differences(tag, a, b, arrays=ARRAYS):
    """the names of the outputs of a that are not b's, bit for bit with NaN equal to NaN (printed with the first place they differ)"""
    bad = []
    for k in arrays:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if x.shape != y.shape:
            print(f"regress[{tag}] {k}: shapes {x.shape} and {y.shape}")
            bad.append(k)
            continue
        nx, ny = np.isnan(x), np.isnan(y)
        ne = (nx != ny) | (~nx & ~ny & (_bits(x).reshape(x.shape) != _bits(y).reshape(y.shape)))
        if ne.any():
            i = tuple(np.argwhere(ne)[0])
            print(f"regress[{tag}] {k}: {int(ne.sum())} of {ne.size} differ, first at {i}: {x[i]!r} against {y[i]!r}")
            bad.append(k)
    for k in INTS + REALS + ("n_credible",):
        if k == "n_credible":
            same = np.array_equal(np.asarray(a[k]), np.asarray(b[k]))
        elif k in INTS:
            same = int(a[k]) == int(b[k])
        else:
            same = _bits(float(a[k])) == _bits(float(b[k]))
        if not same:
            print(f"regress[{tag}] {k}: {a[k]!r} against {b[k]!r}")
            bad.append(k)
    return bad


def _same(a, b, arrays=ARRAYS):
    assert not _differences("equivalence", a, b, arrays)


@pytest.mark.parametrize("case", list(CASES))
def test_every_output_is_the_restatement_bit_for_bit(case, monkeypatch):
    r = _run(case)
    chain, Q, inc = CASES[case]
    K, G, N, lk, *_ = CHAINS[chain]
    dev, ref, e, D = r["dev"], r["ref"], r["e"], r["D"]
    A = r["samples"][2]
    S = int(USED.sum())
    print(f"regress[{case}] S {dev['n_used']} Q {dev['Q']} included {dev['n_included']} left out {dev['n_left_out']} blocks {dev['n_blocks']} min_pivot_ratio "
          f"{dev['min_pivot_ratio']:.3g} at {dev['min_pivot_at']} n_credible {dev['n_credible'].tolist()}; samples that exclude a factor "
          f"{int((A == 0).any(axis=1).sum())}, r2 that are NaN {int(np.isnan(dev['r2_series']).sum())}")
    if case == "three_blocks":
        assert dev["n_included"] == 2049 and dev["n_left_out"] == 71 and dev["n_blocks"] == 3
        assert (np.diff(np.where(inc == 1)[0]) > 1).any(), "the members are contiguous"
    if case == "m65":
        assert dev["n_included"] == 65 and dev["n_blocks"] == 1
    if case == "m_q_plus_1":
        assert dev["n_included"] == Q + 1
    if case == "sbfi":
        assert (A == 0).any() and (A == 0).all(axis=1).any(), "no used sample without a factor"
        assert np.isnan(dev["r2_series"]).any() and not np.isnan(dev["coef_series"]).any() and (dev["fit"][:, 3] < S).any()
    if case == "normal":
        assert (np.asarray(r["M"]) < 0).any(), "no negative cell"
    assert dev["n_used"] == S and dev["coef"].shape == (3, 6, N, Q) and dev["fit"].shape == (3, 5, N)
    assert dev["coef_series"].shape == (3, S, N, Q) and dev["r2_series"].shape == (3, S, N) and dev["n_credible"].shape == (3, Q)
    bad = _differences(case, dev, ref)
    # the other form of the kernels (tiles of 2 factors and 2 design columns): the same bits
    monkeypatch.setenv("BNMF_REG_FORM", "1")
    bad += _differences(case + ", narrow tiles", e.regress(N_RANGE, D, include=inc, used=USED, end_iter=r["end"], credible_interval=CI, series=True), ref)
    monkeypatch.delenv("BNMF_REG_FORM")
    # no interval: NaN bounds, nothing counted
    for ci in (0.0, -1.0):
        d = e.regress(N_RANGE, D, include=inc, used=USED, end_iter=r["end"], credible_interval=ci, series=True)
        bad += _differences(f"{case}, interval {ci:g}", d, R.regress_reference(*r["samples"], D, include=inc, credible_interval=ci))
        assert np.isnan(d["coef"][:, 2:4]).all() and np.isnan(d["fit"][:, 1:3]).all() and (d["n_credible"] == 0).all()
    assert not bad, bad


def _raw(e, end, D, inc, used, ci, skip=()):
    """bnmf_regress_at through ctypes with the outputs in `skip` NULL -> (the Engine.regress layout of the others, the untouched buffers)"""
    from bayesnmf_amd.engine import lib, BnmfRegressInfo
    L, dp, ip = lib(), C.POINTER(C.c_double), C.POINTER(C.c_int32)
    N, Q, S = e.N, D.shape[1], int(used.sum())
    bufs = dict(coef=np.full((3, 6, Q, N), -7.0), fit=np.full((3, 5, N), -7.0), coef_series=np.full((3, S, Q, N), -7.0), r2_series=np.full((3, S, N), -7.0))
    ptr = {k: (None if k in skip else v.ctypes.data_as(dp)) for k, v in bufs.items()}
    info = BnmfRegressInfo()
    Df = np.asfortranarray(D)
    assert L.bnmf_regress_at(e._h, end, len(used), used.ctypes.data_as(ip), Df.ctypes.data_as(dp), Q, None if inc is None else inc.ctypes.data_as(ip), ci,
                             ptr["coef"], ptr["fit"], ptr["coef_series"], ptr["r2_series"], C.byref(info)) == 0
    got = dict(coef=bufs["coef"].transpose(0, 1, 3, 2), fit=bufs["fit"], coef_series=bufs["coef_series"].transpose(0, 1, 3, 2), r2_series=bufs["r2_series"],
               n_credible=np.array([[int(v) for v in row][:Q] for row in info.n_credible]), **{k: getattr(info, k) for k in INTS + REALS})
    return got, bufs


@pytest.mark.parametrize("case", ["three_blocks", "sbfi", "normal"])
def test_equivalent_calls_give_the_same_bits(case):
    r = _run(case)
    e, end, D, inc = r["e"], r["end"], r["D"], r["inc"]
    G = D.shape[0]
    kw = dict(include=inc, credible_interval=CI, series=True)
    _same(r["dev"], e.regress(N_RANGE, D, used=USED, end_iter=end, **kw))                              # a second call
    _same(e.regress(10, D, **kw), e.regress(10, D, end_iter=e.iter, **kw))                             # bnmf_regress is bnmf_regress_at(iter)
    _same(e.regress(10, D, **kw), e.regress(10, D, used=np.ones(10, dtype=np.int32), **kw))            # NULL used is all ones
    all_in = e.regress(N_RANGE, D, used=USED, end_iter=end, credible_interval=CI, series=True)
    _same(all_in, e.regress(N_RANGE, D, used=USED, end_iter=end, include=np.ones(G, dtype=np.int32), credible_interval=CI, series=True))   # NULL include too
    # each output NULL in turn, then all of them: the others and the info fields are the same
    for skip in [(k,) for k in ARRAYS] + [ARRAYS]:
        got, bufs = _raw(e, end, D, inc, USED, CI, skip)
        for k in skip:
            assert (bufs[k] == -7).all(), k                                                            # (not written)
        _same(got, r["dev"], tuple(k for k in ARRAYS if k not in skip))


@pytest.mark.parametrize("case", ["three_blocks", "q5"])
def test_scaling_a_column_by_a_power_of_two_divides_its_coefficient_exactly(case):
    r = _run(case)
    D2 = r["D"].copy()
    scale = np.ones(D2.shape[1])
    scale[1], scale[2] = 2.0 ** 7, 2.0 ** -3
    D2 *= scale
    a, b = r["dev"], r["e"].regress(N_RANGE, D2, include=r["inc"], used=USED, end_iter=r["end"], credible_interval=CI, series=True)
    assert np.array_equal(_bits(b["coef_series"]), _bits(a["coef_series"] / scale))
    assert np.array_equal(_bits(b["coef"][:, [0, 2, 3]]), _bits(a["coef"][:, [0, 2, 3]] / scale)) and np.array_equal(_bits(b["coef"][:, 1]), _bits(a["coef"][:, 1] / scale ** 2))
    assert np.array_equal(_bits(b["coef"][:, 4:]), _bits(a["coef"][:, 4:]))
    assert not _differences("scaled", dict(b, coef=a["coef"], coef_series=a["coef_series"]), a)         # fit, r2 and every info field: the same bits


@pytest.mark.parametrize("case", ["m65", "normal"])
def test_a_reopened_chain_gives_the_same_bits(case, tmp_path):
    r = _run(case)
    path = str(tmp_path / "state.bin")
    r["e"].save_state(path)
    c, _ = _create(r["chain"])
    assert c.load_state(path) == T_END
    _same(r["dev"], c.regress(N_RANGE, r["D"], include=r["inc"], used=USED, end_iter=r["end"], credible_interval=CI, series=True))
    c.close()


def test_refusals():
    from bayesnmf_amd import Engine
    from bayesnmf_amd.engine import lib, BnmfRegressInfo, BnmfError
    from bayesnmf_amd.setup import apply_hyperprior_params
    r = _run("q5")
    e, M, L = r["e"], r["M"], lib()
    G = 70
    info = BnmfRegressInfo()
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    good = np.asfortranarray(_design(G, 3))

    def err():
        msg = L.bnmf_last_error().decode()
        assert msg
        return msg

    def call(n=10, used=None, design=good, Q=None, include=None, ci=0.9, inf=info, at=None, h=None):
        u = None if used is None else used.ctypes.data_as(ip)
        d = None if design is None else design.ctypes.data_as(dp)
        c = None if include is None else include.ctypes.data_as(ip)
        i = None if inf is None else C.byref(inf)
        h = e._h if h is None else h
        Q = (design.shape[1] if design is not None else 3) if Q is None else Q
        if at is None:
            return L.bnmf_regress(h, n, u, d, Q, c, ci, None, None, None, None, i)
        return L.bnmf_regress_at(h, at, n, u, d, Q, c, ci, None, None, None, None, i)

    sq = _include(G, 64)                                                             # 64 tumours: the factor of a repeated column of ones is exact
    for at in (None, e.iter):
        assert call(inf=None, at=at) == -1 and "null" in err()                                       # BNMF_EINVAL
        assert call(design=None, at=at) == -1 and "null" in err()
        u = np.ones(10, dtype=np.int32); u[6] = 2
        assert call(used=u, at=at) == -1 and "used[6] = 2" in err()
        c = np.ones(G, dtype=np.int32); c[11] = 2
        assert call(include=c, at=at) == -1 and "include[11] = 2" in err()
        c[11] = -1
        assert call(include=c, at=at) == -1 and "include[11] = -1" in err()
        for Q in (0, -1, 17):
            assert call(Q=Q, at=at) == -1 and f"Q = {Q}" in err()
        for v in (float("nan"), float("inf"), -float("inf")):
            d = good.copy(order="F"); d[7, 1] = v
            assert call(design=d, at=at) == -1 and "design[7, 1]" in err()
            c = np.ones(G, dtype=np.int32); c[7] = 0                                                 # the cells of a left-out tumour are not read
            assert call(design=d, include=c, at=at) == 0
        for bad in (float("nan"), 1.0, 1.5, float("inf")):
            assert call(ci=bad, at=at) == -1 and "credible_interval" in err()
        dup = np.asfortranarray(np.concatenate([good, good[:, 0:1]], axis=1))
        assert call(design=dup, include=sq, at=at) == -1 and "full column rank" in err() and "column 3" in err()
        assert call(design=np.asfortranarray(np.zeros((G, 2))), at=at) == -1 and "column 0" in err()
        u = np.zeros(10, dtype=np.int32); u[3] = 1
        assert call(used=u, at=at) == -2 and "1 used sample" in err()                                # BNMF_ESIZE
        assert call(include=_include(G, 3), at=at) == -2 and "3 included tumours for Q = 3" in err()
        assert call(include=np.zeros(G, dtype=np.int32), at=at) == -2 and "0 included tumours" in err()
        assert call(include=_include(G, 4), at=at) == 0
    assert call(n=1) == -2 and err()
    assert call(n=W + 1) == -2 and err()
    # the range rule of bnmf_waic_at: iterations [max(1, iter - window + 1), iter]
    assert call(n=5, at=e.iter + 1) == -2 and "are kept" in err()
    assert call(n=W + 1, at=e.iter) == -2 and "are kept" in err()
    assert call(n=3, at=e.iter - W + 1) == -2 and "are kept" in err()
    with pytest.raises(BnmfError, match="used has 3 entries"):
        e.regress(10, good, used=[1, 1, 1])
    with pytest.raises(BnmfError, match="G = 70 rows are needed"):
        e.regress(10, good[:5])
    with pytest.raises(BnmfError, match="G = 70 flags are needed"):
        e.regress(10, good, include=[1, 1])
    # window = 0: BNMF_ESTATE
    z = Engine(M, 3, prior="gamma", seed=4, window=0)
    apply_hyperprior_params(z, "gamma", M, 3)
    z.init(); z.run(5)
    assert call(n=3, h=z._h) == -7 and "window = 0" in err()
    assert call(n=3, at=z.iter, h=z._h) == -7 and "window = 0" in err()
    z.close()
    assert L.bnmf_version() == 100
    assert call(ci=0.0) == 0 and info.n_credible[0][1] == 0 and info.Q == 3 and info.n_included == G and info.n_blocks == 1   # no interval is allowed
    assert call(ci=-3.0) == 0
    # the handle is usable afterwards: the same bits as before the refusals
    _same(r["dev"], e.regress(N_RANGE, r["D"], include=r["inc"], used=USED, end_iter=r["end"], credible_interval=CI, series=True))


@pytest.mark.parametrize("case", ["q16", "ptn_mh", "sbfi"])
def test_the_call_is_read_only_for_the_chain(case):
    """a chain that calls regress mid-run continues with the bits of a twin that never did"""
    r = _run(case)
    chain = r["chain"]
    MH = CHAINS[chain][5]
    b, _, row1 = _fresh(chain)
    rows_b = np.vstack([row1[None, :], b.run(T_END - 1, converged=MH)])
    assert np.array_equal(_bits(rows_b), _bits(r["rows"]))
    more_a, more_b = r["e"].run(10, converged=MH), b.run(10, converged=MH)       # a called regress at iteration 40, b never did
    assert np.array_equal(_bits(more_a), _bits(more_b))
    for nm in ("P", "E", "A"):
        assert np.array_equal(_bits(r["e"].get(nm)), _bits(b.get(nm))), nm
    b.close()
    _CHAINS.pop(chain)["e"].close()                                              # (this chain has moved on)
    for c in [c for c in _RUNS if CASES[c][0] == chain]:
        _RUNS.pop(c)
