"""Silhouette stability of the recorded signatures on the device (bnmf_stability / bnmf_stability_at, csrc/stability.h) against the
numerical spec restated in numpy float64 (tests/stability_ref.py, written from DESIGN.md 22): point, factor, between, medoid,
medoid_at and every info field of every case bit for bit, NaN compared as NaN, no tolerance — the operations are + - * /, sqrt,
comparisons and whole numbers only; then the equivalences and the refusals.

Every chain is a dozen iterations (the rank-learning one 40: its schedule excludes factors from iteration 21 on) with window = 16;
the range is the 12 samples that end 2 iterations before `iter`, with a `used` mask that has gaps (9 used samples).  The shapes are
the smallest that reach each path: N = 2 (one other cluster), 3, 5, 9 and 20; K = 8, 12 and 96; cluster 0 padded by extra columns to
63, 64, 65, 1,023, 1,024 and 1,025 members (one wave round, a block boundary with one member in the last block); member counts that
are and are not a multiple of the 8 rows of a wave or the 32 of a workgroup."""
import ctypes as C

import numpy as np
import pytest

import stability_ref as R

pytestmark = pytest.mark.gpu

W, N_RANGE = 16, 12
USED = np.array([1, 1, 0, 1, 1, 1, 0, 0, 1, 1, 1, 1], dtype=np.int32)
S_USED = int(USED.sum())
ARRAYS = ("point", "factor", "between", "medoid", "medoid_at")

# chain: K, G, N, likelihood, prior, MH, learning_rank, seed, last iteration, fixed_P
CHAINS = {
    "n2": (8, 40, 2, "poisson", "gamma", False, False, 4, 14, False),
    "g70": (8, 70, 3, "poisson", "gamma", False, False, 4, 14, False),
    "n9": (8, 70, 9, "poisson", "gamma", False, False, 4, 14, False),
    "normal": (12, 10, 3, "normal", "exponential", False, False, 4, 14, False),           # real-valued data, negative cells
    "ptn_mh": (96, 6, 5, "poisson", "truncnormal", True, False, 4, 14, False),            # rings recorded by the MH sweep
    "sbfi": (96, 8, 20, "poisson", "gamma", False, True, 14, 40, False),                  # samples with A[n] = 0
    "fixed": (8, 70, 3, "poisson", "gamma", False, False, 4, 14, True),                   # every column of P held: identical members
}


def _shuffled(N, rows=N_RANGE, seed=3):
    """a fixed shuffle of the labels per sample of the range, two rows and two single places left out"""
    lab = np.stack([np.random.default_rng(seed + s).permutation(N) for s in range(rows)]).astype(np.int32)
    lab[4] = -1
    lab[9] = -1
    lab[0, 0] = -1
    lab[11, N - 1] = -1
    return lab


def _once(N):
    """label N - 1 used exactly once"""
    lab = np.tile(np.arange(N, dtype=np.int32), (N_RANGE, 1))
    lab[:, N - 1] = -1
    lab[5, N - 1] = N - 1
    return lab


def _pad(K, N, total, seed=8):
    """extra columns that bring cluster 0 from its 9 ring members to `total`, and one for the last cluster"""
    X = total - S_USED
    ex = np.asfortranarray(np.random.default_rng(seed).gamma(0.5, 1.0, size=(K, X + 1)))
    return ex, np.concatenate([np.zeros(X, dtype=np.int32), [N - 1]]).astype(np.int32)


# case: chain, labels over the range (None = the factor), extras
CASES = {
    "n2": ("n2", None, None),
    "g70": ("g70", None, None),
    "n9": ("n9", None, None),
    "normal": ("normal", None, None),
    "ptn_mh": ("ptn_mh", None, None),
    "sbfi": ("sbfi", None, None),
    "fixed": ("fixed", None, None),
    "shuffled9": ("n9", _shuffled(9), None),
    "shuffled20": ("sbfi", _shuffled(20), None),
    "once": ("g70", _once(3), None),
    "one_cluster": ("g70", np.zeros((N_RANGE, 3), dtype=np.int32), None),
    "shuffled_extras": ("ptn_mh", _shuffled(5), _pad(96, 5, 40)),
}
for _m in (63, 64, 65, 1023, 1024, 1025):
    CASES[f"m{_m}"] = ("g70", None, _pad(8, 3, _m))
CASES["m1025_k96"] = ("ptn_mh", None, _pad(96, 5, 1025))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _data(chain):
    from bayesnmf_amd.setup import synth_counts
    K, G, N, lk, *_ = CHAINS[chain]
    if lk == "normal":
        rng = np.random.default_rng(11)
        return np.asfortranarray(rng.gamma(1.0, 1.0, size=(K, 3)) @ rng.gamma(0.5, 1.0, size=(3, G)) + rng.normal(0.0, 0.5, size=(K, G)))
    M, _, _ = synth_counts(K, G, min(3, N), 21, mean_total=1500)
    return M


def _temps():
    return np.concatenate([np.ones(20), np.zeros(3), 10.0 ** np.linspace(-6, 0, 60), np.ones(100)])


def _fresh(chain, seed=None):
    from bayesnmf_amd import Engine
    from bayesnmf_amd.setup import apply_hyperprior_params
    K, G, N, lk, prior, MH, lr, seed0, _, fixed = CHAINS[chain]
    seed = seed0 if seed is None else seed
    M = _data(chain)
    e = Engine(M, N, likelihood=lk, prior=prior, MH=MH, learning_rank=lr, seed=seed, window=W, temperature=_temps() if lr else None)
    apply_hyperprior_params(e, prior, M, N)
    if fixed:
        e.set("P", np.asfortranarray(np.random.default_rng(6).dirichlet(np.full(K, 0.4), size=N).T))
        e.set_fixed("P", np.ones(N, dtype=np.int32))
    row1 = e.init()
    return e, M, row1


_CHAINS, _RUNS = {}, {}


def _chain(chain):
    """the chain at its last iteration, its metric rows and the used samples of the range: made once per chain"""
    if chain in _CHAINS:
        return _CHAINS[chain]
    K, G, N, lk, prior, MH, lr, _, t_end, _ = CHAINS[chain]
    e, M, row1 = _fresh(chain)
    rows = np.vstack([row1[None, :], e.run(t_end - 1, converged=MH)])
    assert e.iter == t_end
    end, n = t_end - 2, N_RANGE
    back = t_end - (end - n + 1) + 1
    sel = np.where(USED == 1)[0]
    P = np.stack([e.window("P", back)[i] for i in sel])
    A = np.stack([e.window("A", back)[i] for i in sel]).reshape(len(sel), N)
    _CHAINS[chain] = dict(e=e, M=M, rows=rows, end=end, n=n, P=P, A=A)
    return _CHAINS[chain]


def _ref(ch, labels, extras):
    ex, el = extras if extras is not None else (None, None)
    return R.stability_reference(ch["P"], ch["A"], None if labels is None else labels[USED == 1], ex, el)


def _call(ch, labels, extras, e=None, **kw):
    ex, el = extras if extras is not None else (None, None)
    kw = dict(dict(labels=labels, used=USED, end_iter=ch["end"], extra_P=ex, extra_label=el), **kw)
    return (e or ch["e"]).stability(ch["n"], **kw)


def _run(case):
    if case in _RUNS:
        return _RUNS[case]
    chain, labels, extras = CASES[case]
    ch = _chain(chain)
    _RUNS[case] = dict(ch, chain=chain, labels=labels, extras=extras, ref=_ref(ch, labels, extras), dev=_call(ch, labels, extras))
    return _RUNS[case]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for r in _CHAINS.values():
        r["e"].close()
    _CHAINS.clear()
    _RUNS.clear()


def _differences(tag, a, b, arrays=ARRAYS, info=R.INFO):
    """the names of the outputs of a that are not b's, bit for bit with NaN equal to NaN (printed with the first place they differ)"""
    bad = []
    for k in arrays:
        x, y = np.asarray(a[k], dtype=np.float64), np.asarray(b[k], dtype=np.float64)
        if x.shape != y.shape:
            print(f"stability[{tag}] {k}: shapes {x.shape} and {y.shape}")
            bad.append(k)
            continue
        nx, ny = np.isnan(x), np.isnan(y)
        ne = (nx != ny) | (~nx & ~ny & (_bits(x).reshape(x.shape) != _bits(y).reshape(y.shape)))
        if ne.any():
            i = tuple(np.argwhere(ne)[0])
            print(f"stability[{tag}] {k}: {int(ne.sum())} of {ne.size} differ, first at {i}: {x[i]!r} against {y[i]!r}")
            bad.append(k)
    for k in info:
        fa, fb = float(a[k]), float(b[k])
        if not ((np.isnan(fa) and np.isnan(fb)) or _bits(fa) == _bits(fb)):
            print(f"stability[{tag}] {k}: {a[k]!r} against {b[k]!r}")
            bad.append(k)
    return bad


def _same(a, b, **kw):
    assert not _differences("equivalence", a, b, **kw)


@pytest.mark.parametrize("case", list(CASES))
def test_every_output_is_the_restatement_bit_for_bit(case):
    r = _run(case)
    chain, labels, extras = CASES[case]
    K, G, N = CHAINS[chain][:3]
    dev, ref = r["dev"], r["ref"]
    print(f"stability[{case}] S {dev['n_used']} points {dev['n_points']} extra {dev['n_extra']} left out {dev['n_left_out']} clusters {dev['n_clusters']} "
          f"members {dev['factor'][0].astype(int).tolist()} negative {dev['n_negative']} mean silhouette {dev['mean_silhouette']:.4g} "
          f"min stability {dev['min_stability']:.4g} at {dev['min_stability_at']}")
    X = 0 if extras is None else extras[0].shape[1]
    assert dev["n_used"] == S_USED and dev["point"].shape == (4, S_USED * N + X) and dev["medoid"].shape == (K, N)
    if case.startswith("m") and case[1:].isdigit():
        assert ref["factor"][0, 0] == int(case[1:])
    if case in ("sbfi", "shuffled20"):
        assert (r["A"] == 0).any() and ref["n_left_out"] > 0, "the chain has no sample that excludes a factor"
    if case == "fixed":
        assert (ref["point"][1] == 0).all() and (_bits(r["P"]) == _bits(r["P"][0])[None]).all(), "the members are not identical"
    if case == "normal":
        assert (np.asarray(r["M"]) < 0).any(), "no negative cell"
    if case == "once":
        assert ref["factor"][0, 2] == 1
    if case == "one_cluster":
        assert np.isnan(ref["mean_silhouette"]) and ref["n_clusters"] == 1
    assert not _differences(case, dev, ref)


def _raw(r, skip=()):
    """bnmf_stability_at through ctypes with the outputs in `skip` NULL -> (the Engine.stability layout of the others, the untouched buffers)"""
    from bayesnmf_amd.engine import lib, BnmfStabilityInfo
    e = r["e"]
    L, dp, ip, lp = lib(), C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    N, K = e.N, e.K
    ex, el = r["extras"] if r["extras"] is not None else (None, None)
    X = 0 if ex is None else ex.shape[1]
    bufs = dict(point=np.full((4, S_USED * N + X), -7.0), factor=np.full((6, N), -7.0), between=np.full((N, N), -7.0), medoid=np.full(K * N, -7.0),
                medoid_at=np.full(N, -7, dtype=np.int64))
    ptr = {k: (None if k in skip else v.ctypes.data_as(lp if k == "medoid_at" else dp)) for k, v in bufs.items()}
    info = BnmfStabilityInfo()
    lab = r["labels"]
    exf = None if ex is None else np.ascontiguousarray(ex.ravel(order="F"))
    assert L.bnmf_stability_at(e._h, r["end"], r["n"], USED.ctypes.data_as(ip), None if lab is None else lab.ctypes.data_as(ip),
                               None if ex is None else exf.ctypes.data_as(dp), None if ex is None else el.ctypes.data_as(ip), X,
                               ptr["point"], ptr["factor"], ptr["between"], ptr["medoid"], ptr["medoid_at"], C.byref(info)) == 0
    got = dict(bufs, **{k: getattr(info, k) for k in R.INFO})
    got["medoid"] = bufs["medoid"].reshape((K, N), order="F")
    return got, bufs


@pytest.mark.parametrize("case", ["n9", "shuffled20", "m1025"])
def test_equivalent_calls_give_the_same_bits(case, tmp_path):
    r = _run(case)
    e, labels, extras = r["e"], r["labels"], r["extras"]
    N = e.N
    ex, el = extras if extras is not None else (None, None)
    _same(r["dev"], _call(r, labels, extras))                                                            # a second call
    kw = dict(extra_P=ex, extra_label=el)
    _same(e.stability(10, **kw), e.stability_at(e.iter, 10, **kw))                                       # bnmf_stability is bnmf_stability_at(iter)
    _same(e.stability(10, **kw), e.stability(10, used=np.ones(10, dtype=np.int32), **kw))                # NULL used is all ones
    ident = np.tile(np.arange(N, dtype=np.int32), (N_RANGE, 1))
    _same(_call(r, None, extras), _call(r, ident, extras))                                               # NULL labels are the factors
    junk = ident.copy()
    junk[USED == 0] = 99                                                                                 # rows of unused samples are not read
    _same(_call(r, None, extras), _call(r, junk, extras))
    # renumbering the labels permutes the outputs
    pi = np.random.default_rng(1).permutation(N)
    lab = ident if labels is None else labels
    ren = _call(r, np.where(lab >= 0, pi[np.clip(lab, 0, None)], -1).astype(np.int32), None if extras is None else (ex, pi[el].astype(np.int32)))
    base = r["dev"]
    near = base["point"][3]
    back = dict(ren, factor=ren["factor"][:, pi], medoid=ren["medoid"][:, pi], between=ren["between"][np.ix_(pi, pi)], medoid_at=ren["medoid_at"][pi],
                point=np.vstack([ren["point"][:3], np.where(near >= 0, near, -1)[None]]))
    assert np.array_equal(ren["point"][3], np.where(near >= 0, pi[np.clip(near.astype(int), 0, None)], -1).astype(np.float64))
    _same(back, base, info=tuple(k for k in R.INFO if k != "min_stability_at"))
    assert ren["min_stability_at"] == (pi[base["min_stability_at"]] if base["min_stability_at"] >= 0 else -1)
    # each output NULL in turn, then all: the others and the info fields are the same
    for skip in [(k,) for k in ARRAYS] + [ARRAYS]:
        got, bufs = _raw(r, skip)
        for k in skip:
            assert (bufs[k] == -7).all(), k                                                              # (not written)
        _same(got, r["dev"], arrays=tuple(k for k in ARRAYS if k not in skip))


def test_extras_are_the_same_columns_recorded_in_the_ring():
    """the last used samples of the range handed in as extra columns instead: the member lists hold the same columns in the same
    order, so every output has the same bits (the chain's A is all ones, as an extra column is always a member)"""
    r = _run("g70")
    e, N = r["e"], 3
    assert (r["A"] != 0).all()
    used = USED.copy()
    used[8:] = 0                                                                                         # the first 5 used samples stay in the ring
    ex = np.asfortranarray(np.concatenate([r["P"][s] for s in range(5, S_USED)], axis=1))                # K x (4 N), sample by sample
    el = np.tile(np.arange(N, dtype=np.int32), S_USED - 5)
    got = e.stability(r["n"], used=used, end_iter=r["end"], extra_P=ex, extra_label=el)
    assert got["n_used"] == 5 and got["n_extra"] == 4 * N
    _same(got, r["dev"], info=tuple(k for k in R.INFO if k not in ("n_used", "n_extra")))


def test_refusals():
    from bayesnmf_amd import Engine
    from bayesnmf_amd.engine import lib, BnmfStabilityInfo, BnmfError
    from bayesnmf_amd.setup import apply_hyperprior_params
    r = _run("g70")
    e, M, L = r["e"], r["M"], lib()
    K, N = 8, 3
    info = BnmfStabilityInfo()
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)

    def err():
        msg = L.bnmf_last_error().decode()
        assert msg
        return msg

    def call(n=10, used=None, labels=None, ex=None, el=None, X=None, inf=info, at=None, h=None):
        u = None if used is None else used.ctypes.data_as(ip)
        lb = None if labels is None else labels.ctypes.data_as(ip)
        exf = None if ex is None else np.ascontiguousarray(ex.ravel(order="F"))
        X = (0 if ex is None else ex.shape[1]) if X is None else X
        args = (u, lb, None if exf is None else exf.ctypes.data_as(dp), None if el is None else el.ctypes.data_as(ip), X, None, None, None, None, None,
                None if inf is None else C.byref(inf))
        h = e._h if h is None else h
        return L.bnmf_stability(h, n, *args) if at is None else L.bnmf_stability_at(h, at, n, *args)

    good = np.asfortranarray(np.random.default_rng(2).gamma(0.5, 1.0, size=(K, 4)))
    gl = np.array([0, 1, 2, 0], dtype=np.int32)
    for at in (None, e.iter):
        assert call(inf=None, at=at) == -1 and "null" in err()                                       # BNMF_EINVAL
        u = np.ones(10, dtype=np.int32); u[6] = 2
        assert call(used=u, at=at) == -1 and "used[6] = 2" in err()
        lab = np.tile(np.arange(N, dtype=np.int32), (10, 1)); lab[7, 1] = N
        assert call(labels=lab, at=at) == -1 and "labels[7][1] = 3" in err()
        lab[7, 1] = -2
        assert call(labels=lab, at=at) == -1 and "labels[7][1] = -2" in err()
        assert call(X=-1, at=at) == -1 and "X = -1" in err()
        assert call(X=2, at=at) == -1 and "null" in err()
        assert call(ex=good, el=None, at=at) == -1 and "null" in err()
        for v in (-1, N):
            bl = gl.copy(); bl[2] = v
            assert call(ex=good, el=bl, at=at) == -1 and f"extra_label[2] = {v}" in err()
        for v in (float("nan"), float("inf")):
            b = good.copy(); b[5, 1] = v
            assert call(ex=b, el=gl, at=at) == -1 and "extra_P[5, 1]" in err()
        b = good.copy(); b[:, 3] = 0.0
        assert call(ex=b, el=gl, at=at) == -1 and "extra column 3 is all zero" in err()
        u = np.zeros(10, dtype=np.int32); u[3] = 1
        assert call(used=u, at=at) == -2 and "1 used sample" in err()                                # BNMF_ESIZE
        none = np.full((10, N), -1, dtype=np.int32)
        assert call(labels=none, at=at) == -2 and "0 members" in err()
        none[2, 1] = 1
        assert call(labels=none, at=at) == -2 and "1 member " in err()
        assert call(labels=none, ex=good[:, :1], el=gl[:1], at=at) == 0 and info.n_points == 2
        assert call(ex=good, el=gl, at=at) == 0 and info.n_extra == 4 and info.n_points == 10 * N + 4
    big = np.asfortranarray(np.ones((K, 65536 - 10 * N + 1)) + np.arange(K)[:, None])
    assert call(ex=big, el=np.zeros(big.shape[1], dtype=np.int32)) == -2 and "65537 members" in err()
    assert call(n=1) == -2 and err()
    assert call(n=W + 1) == -2 and err()
    # the range rule of bnmf_waic_at: iterations [max(1, iter - window + 1), iter]
    assert call(n=5, at=e.iter + 1) == -2 and "are kept" in err()
    assert call(n=W + 1, at=e.iter) == -2 and "are kept" in err()
    with pytest.raises(BnmfError, match="used has 3 entries"):
        e.stability(10, used=[1, 1, 1])
    with pytest.raises(BnmfError, match="labels is"):
        e.stability(10, labels=[[0, 1, 2]])
    with pytest.raises(BnmfError, match="extra_label has shape"):
        e.stability(10, extra_P=good, extra_label=[0, 1])
    # N < 2: BNMF_ESIZE;  window = 0: BNMF_ESTATE
    for N1, win, code, word in ((1, W, -2, "N = 1"), (3, 0, -7, "window = 0")):
        z = Engine(M, N1, prior="gamma", seed=4, window=win)
        apply_hyperprior_params(z, "gamma", M, N1)
        z.init(); z.run(5)
        assert call(n=3, h=z._h) == code and word in err()
        assert call(n=3, at=z.iter, h=z._h) == code and word in err()
        z.close()
    # the handle is usable afterwards: the same bits as before the refusals
    _same(r["dev"], _call(r, r["labels"], r["extras"]))


@pytest.mark.parametrize("chain", ["g70", "sbfi"])
def test_pooled_stability_of_two_replicas_is_the_restatement(chain):
    """two tiny replicas (plain, and rank-learning ones whose samples exclude factors): every replica aligned to the first one's
    aligned mean, the second one's aligned columns handed to the first handle as extra columns.  The expected points are put together
    here from the second replica's own windows of P and A and its perm: factor n of sample s enters with label perm[s][n] where
    A_s[n] != 0, and the aligned column under that label is that factor's own column up to its scale."""
    from bayesnmf_amd.multichain import pooled_stability

    class _Rep:
        """what pooled_stability needs of a sampler: its engine and the recorded range"""
        def __init__(self, e, n):
            self._chain, self.n = e, n

        def _recorded_range(self, end_iter, n_samples, idx):
            return self.n, None, None, {}

    N, MH, t_end = CHAINS[chain][2], CHAINS[chain][5], CHAINS[chain][8]
    a, _, _ = _fresh(chain)
    b, _, _ = _fresh(chain, seed=9)
    a.run(t_end - 1, converged=MH); b.run(t_end - 1, converged=MH)
    n = 6
    got = pooled_stability([_Rep(a, n), _Rep(b, n)])
    pivot = a.relabel(n)["P_mean"]
    ra = a.relabel(n, pivot_P=pivot)
    rb = b.relabel(n, pivot_P=pivot, aligned=True)
    Pb, Ab = np.stack(b.window("P", n)), np.stack(b.window("A", n)).reshape(n, N)
    cols, labs = [], []
    for s in range(n):
        if rb["perm"][s, 0] < 0:
            continue
        assert sorted(rb["perm"][s].tolist()) == list(range(N))
        for f in range(N):
            raw, col = Pb[s][:, f], rb["aligned_P"][s][:, rb["perm"][s, f]]
            if Ab[s, f] != 0 and np.isfinite(raw).all() and raw.any():
                assert abs(float(col @ raw) / float(np.sqrt((col @ col) * (raw @ raw))) - 1.0) < 1e-12, (s, f)
                cols.append(col)
                labs.append(int(rb["perm"][s, f]))
    if chain == "sbfi":
        assert (Ab == 0).any() and len(cols) < n * N, "the second replica excludes no factor"
    P = np.stack(a.window("P", n))
    A = np.stack(a.window("A", n)).reshape(n, N)
    ref = R.stability_reference(P, A, ra["perm"], np.stack(cols, axis=1), labs)
    assert got["n_extra"] == len(cols) and got["n_replicas"] == 2
    assert not _differences("pooled", got, ref)
    a.close(); b.close()


@pytest.mark.parametrize("case", ["n9", "ptn_mh", "sbfi"])
def test_the_call_is_read_only_for_the_chain(case):
    """a chain that calls stability mid-run continues with the bits of a twin that never did"""
    r = _run(case)
    chain = r["chain"]
    MH, t_end = CHAINS[chain][5], CHAINS[chain][8]
    b, _, row1 = _fresh(chain)
    rows_b = np.vstack([row1[None, :], b.run(t_end - 1, converged=MH)])
    assert np.array_equal(_bits(rows_b), _bits(r["rows"]))
    more_a, more_b = r["e"].run(5, converged=MH), b.run(5, converged=MH)         # a called stability, b never did
    assert np.array_equal(_bits(more_a), _bits(more_b))
    for nm in ("P", "E", "A"):
        assert np.array_equal(_bits(r["e"].get(nm)), _bits(b.get(nm))), nm
    b.close()
    _CHAINS.pop(chain)["e"].close()                                              # (this chain has moved on)
    for c in [c for c in _RUNS if CASES[c][0] == chain]:
        _RUNS.pop(c)
