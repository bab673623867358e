"""Trade-offs between signatures within a tumour on the device (bnmf_tradeoff / bnmf_tradeoff_at, csrc/tradeoff.h) against the numerical
spec restated in numpy float64 (tests/tradeoff_ref.py, written from DESIGN.md 27): every output and every info field of every case bit
for bit, NaN compared as NaN, no tolerance — the operations are + - * /, sqrt, comparisons and whole numbers only; then the equivalences
and the refusals.

Every case keeps window = 16 samples and runs 13 iterations (the rank-learning chain 40, as tests/test_gpu_subtypes.py's, so that A
excludes factors); the range is the 10 samples that end one iteration before `iter`, with a `used` mask that has gaps.  The shapes are
the smallest that reach each path of the kernels:
  K = 6, G = 70, N = 5: 5 lanes per tumour, 51 tumours per workgroup: two workgroups, the second ragged; with bands of 7 and 64 members
  the canonB accumulators are carried between bands;
  N = 1: one lane per tumour, no pair, the pair kernel is not launched;
  N = 17, G = 3: one past a tile of 16 values of l: factor 16 has two tiles (three tiles of 8 in the other form);
  G = 1: one member; G = 1,100: the member list crosses a block of 1,024 positions of canonB, with a band that ends inside the second
  block (1,000) and one that ends on the boundary (1,024);
  a rank-learning chain with N = 20 (24 lanes per tumour, samples with A[n] = 0); real-valued Normal data.
Both forms (BNMF_TRD_FORM) and small bands (BNMF_TRD_BAND) must give the same bits."""
import ctypes as C

import numpy as np
import pytest

import tradeoff_ref as R

pytestmark = pytest.mark.gpu

W, N_RANGE = 16, 10
USED = np.array([1, 1, 0, 1, 1, 0, 0, 1, 1, 1], dtype=np.int32)
ARRAYS = ("tumour", "pair_at", "pair", "setstat", "dense")
INFO = ("n_used", "n_matched", "n_unmatched", "n_included", "n_left_out", "n_sets", "n_query", "n_traded", "strongest_pair_at", "strongest_pair", "mean_ratio",
        "min_corr")

# name: K, G, N, likelihood, prior, learning_rank, seed, iterations
CASES = {
    "g70": (6, 70, 5, "poisson", "gamma", False, 4, 13),
    "n1": (6, 10, 1, "poisson", "gamma", False, 4, 13),
    "n17": (6, 3, 17, "poisson", "gamma", False, 4, 13),
    "g1": (6, 1, 3, "poisson", "gamma", False, 4, 13),
    "g1100": (6, 1100, 3, "poisson", "gamma", False, 4, 13),
    "sbfi": (96, 8, 20, "poisson", "gamma", True, 14, 40),
    "normal": (12, 10, 3, "normal", "exponential", False, 4, 13),
}
SETS = {5: [0, 1, 1, -1, 2], 1: [0], 17: [0] * 8 + [1] * 8 + [-1], 3: [0, 0, 1], 20: [0] * 10 + [-1] * 5 + [1] * 5}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _data(case):
    from bayesnmf_amd.setup import synth_counts
    K, G, N, lk, *_ = CASES[case]
    if lk == "normal":
        rng = np.random.default_rng(11)
        return np.asfortranarray(rng.gamma(1.0, 1.0, size=(K, 3)) @ rng.gamma(0.5, 1.0, size=(3, G)) + rng.normal(0.0, 0.5, size=(K, G)))
    M, _, _ = synth_counts(K, G, min(3, N), 21, mean_total=1500)
    return M


def _temps():
    return np.concatenate([np.ones(20), np.zeros(3), 10.0 ** np.linspace(-6, 0, 60), np.ones(100)])


def _engine(case, iters=None):
    from bayesnmf_amd import Engine
    from bayesnmf_amd.setup import apply_hyperprior_params
    K, G, N, lk, prior, lr, seed, T = CASES[case]
    M = _data(case)
    e = Engine(M, N, likelihood=lk, prior=prior, learning_rank=lr, seed=seed, window=W, temperature=_temps() if lr else None)
    apply_hyperprior_params(e, prior, M, N)
    e.init()
    e.run((T if iters is None else iters) - 1)
    return e


def _window(e, end, n, sel):
    back = e.iter - (end - n + 1) + 1
    win = {nm: np.stack([e.window(nm, back)[i] for i in sel]) for nm in ("P", "E", "A")}
    return win["P"], win["E"], win["A"].reshape(len(sel), -1)


_RUNS = {}


def _run(case):
    """the chain at its last iteration and the used samples of the range: once per case"""
    if case not in _RUNS:
        e = _engine(case)
        assert e.iter == CASES[case][7]
        end = e.iter - 1
        _RUNS[case] = dict(e=e, end=end, samples=_window(e, end, N_RANGE, np.where(USED == 1)[0]), G=CASES[case][1], N=CASES[case][2])
    return _RUNS[case]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for r in _RUNS.values():
        r["e"].close()
    _RUNS.clear()


def _differences(tag, a, b, arrays=ARRAYS, info=INFO):
    """the names of the outputs of a that are not b's, bit for bit with NaN equal to NaN (printed with the first place they differ)"""
    bad = []
    for k in arrays:
        if (k in a) != (k in b):
            if np.asarray(a[k] if k in a else b[k]).size == 0:                                                # (no query: the binding leaves it out)
                continue
            print(f"tradeoff[{tag}] {k}: only one side has it")
            bad.append(k)
            continue
        if k not in a:
            continue
        x, y = np.asarray(a[k], dtype=np.float64), np.asarray(b[k], dtype=np.float64)
        if x.shape != y.shape:
            print(f"tradeoff[{tag}] {k}: shapes {x.shape} and {y.shape}")
            bad.append(k)
            continue
        nx, ny = np.isnan(x), np.isnan(y)
        ne = (nx != ny) | (~nx & ~ny & (_bits(x).reshape(x.shape) != _bits(y).reshape(y.shape)))
        if ne.any():
            i = tuple(np.argwhere(ne)[0])
            print(f"tradeoff[{tag}] {k}: {int(ne.sum())} of {ne.size} differ, first at {i}: {x[i]!r} against {y[i]!r}")
            bad.append(k)
    for k in info:
        fa, fb = float(a[k]), float(b[k])
        if not ((np.isnan(fa) and np.isnan(fb)) or _bits(fa) == _bits(fb)):
            print(f"tradeoff[{tag}] {k}: {a[k]!r} against {b[k]!r}")
            bad.append(k)
    return bad


def _queries(G):
    return np.array([G - 1, G // 2, G - 1], dtype=np.int32)                                                    # Q = 3, one named twice


@pytest.mark.parametrize("case", list(CASES))
def test_every_output_is_the_restatement_bit_for_bit(case, monkeypatch):
    r = _run(case)
    e, G, N = r["e"], r["G"], r["N"]
    q, sets = _queries(G), np.array(SETS[N], dtype=np.int32)
    kw = dict(used=USED, end_iter=r["end"], query=q, sets=sets, min_corr=0.5)
    ref = R.tradeoff_reference(*r["samples"], sets=sets, query=q, min_corr=0.5)
    dev = e.tradeoff(N_RANGE, **kw)
    A = r["samples"][2]
    print(f"tradeoff[{case}] S {dev['n_used']} m {dev['n_included']} traded {dev['n_traded']} strongest {dev['strongest_pair']!r} at {dev['strongest_pair_at']} "
          f"mean ratio {dev['mean_ratio']!r}; defined pairs {np.unique(dev['tumour'][1]).tolist()}; factors excluded in every used sample "
          f"{int((A == 0).all(axis=0).sum())}, in some {int((A == 0).any(axis=0).sum())}")
    C_ = int(sets.max()) + 1
    assert dev["tumour"].shape == (3, G) and dev["pair"].shape == (5, N, N) and dev["setstat"].shape == (4, C_, G) and dev["dense"].shape == (3, 2, N, N)
    assert dev["n_used"] == 7 and dev["n_matched"] == 7 and dev["n_sets"] == C_
    bad = _differences(case, dev, ref)
    if N == 1:
        assert np.isnan(dev["tumour"][0]).all() and (dev["tumour"][1] == 0).all() and (dev["pair_at"] == -1).all() and np.isnan(dev["pair"]).all()
        assert np.isnan(dev["dense"][:, 1]).all() and dev["strongest_pair_at"] == -1
    if case == "sbfi":
        assert (A == 0).any(), "no used sample excludes a factor"
    # the other form and small bands of members through the scratch: the same bits
    bands = ("1000", "1024") if case == "g1100" else ("7", "64")
    for form, band in (("1", None), (None, bands[0]), ("1", bands[1]), (None, "1")):
        if band == "1" and G > 100:
            continue
        if form:
            monkeypatch.setenv("BNMF_TRD_FORM", form)
        if band:
            monkeypatch.setenv("BNMF_TRD_BAND", band)
        bad += _differences(f"{case}, form {form}, band {band}", e.tradeoff(N_RANGE, **kw), ref)
        monkeypatch.delenv("BNMF_TRD_FORM", raising=False)
        monkeypatch.delenv("BNMF_TRD_BAND", raising=False)
    assert not bad, bad


def test_a_factor_excluded_in_every_used_sample_gives_undefined_pairs():
    """the rank-learning chain: the used samples are those of the range in which A excludes one factor (the one excluded most often),
    so its exposure is +0.0 throughout, its variance 0 and every pair with it undefined"""
    r = _run("sbfi")
    e, end, G, N = r["e"], r["end"], r["G"], r["N"]
    _, _, A = _window(e, end, N_RANGE, np.arange(N_RANGE))
    n = int(np.argmax((A == 0).sum(axis=0)))
    used = (A[:, n] == 0).astype(np.int32)
    print(f"tradeoff[sbfi] factor {n} is excluded in {int(used.sum())} of {N_RANGE} samples")
    assert used.sum() >= 2, "no factor is excluded in two samples of the range"
    dev = e.tradeoff(N_RANGE, used=used, end_iter=end, query=[0, G - 1], sets=np.array(SETS[N], dtype=np.int32))
    ref = R.tradeoff_reference(*_window(e, end, N_RANGE, np.where(used == 1)[0]), query=[0, G - 1], sets=np.array(SETS[N], dtype=np.int32))
    assert not _differences("excluded", dev, ref)
    assert (dev["tumour"][1] <= (N - 1) * (N - 2) // 2).all() and (dev["pair"][1, n, np.arange(N) != n] == 0).all() and np.isnan(dev["pair"][0, n]).all()
    assert np.isnan(dev["dense"][:, 1, n]).all() and (dev["dense"][:, 0, n] == 0).all() and (dev["pair_at"] // N != n).all() and (dev["pair_at"] % N != n).all()


def test_sets_of_everything_of_one_and_none():
    r = _run("g70")
    e, N = r["e"], r["N"]
    kw = dict(used=USED, end_iter=r["end"])
    every = e.tradeoff(N_RANGE, sets=np.zeros(N, dtype=np.int32), **kw)
    assert not _differences("C = 1", every, R.tradeoff_reference(*r["samples"], sets=np.zeros(N, dtype=np.int32)))
    assert np.array_equal(_bits(every["setstat"][3, 0]), _bits(every["tumour"][2]))                            # the set of everything is the total
    one = e.tradeoff(N_RANGE, sets=np.array([-1, -1, 0, -1, -1], dtype=np.int32), **kw)
    assert (one["setstat"][3, 0] == 1.0).all() and np.array_equal(_bits(one["setstat"][1, 0]), _bits(one["setstat"][2, 0]))
    none = e.tradeoff(N_RANGE, **kw)
    assert none["setstat"].shape == (4, 0, r["G"]) and none["n_sets"] == 0 and "dense" not in none
    assert not _differences("no sets", none, R.tradeoff_reference(*r["samples"]))
    assert not _differences("the sets change nothing else", none, every, arrays=("tumour", "pair_at", "pair"), info=tuple(k for k in INFO if k != "n_sets"))


def test_two_samples_perm_and_an_unmatched_sample():
    r = _run("g70")
    e, end, G, N = r["e"], r["end"], r["G"], r["N"]
    s2 = np.zeros(N_RANGE, dtype=np.int32)
    s2[[2, 8]] = 1                                                                                             # S' = 2: the minimum
    two = e.tradeoff(N_RANGE, used=s2, end_iter=end, query=[3])
    assert two["n_used"] == 2 and not _differences("S = 2", two, R.tradeoff_reference(*_window(e, end, N_RANGE, [2, 8]), query=[3]))
    sel = np.where(USED == 1)[0]
    rows = np.tile(np.arange(N, dtype=np.int32), (len(sel), 1))
    rows[1] = rows[1][[1, 0, 2, 3, 4]]                                                                         # two rows with swapped factors
    rows[5] = rows[5][[0, 1, 4, 3, 2]]
    rows[3] = -1                                                                                               # an unmatched sample
    perm = np.full((N_RANGE, N), -1, dtype=np.int32)
    perm[sel] = rows
    perm[2] = 7                                                                                                # (a row of an unused sample is not read)
    sets = np.array(SETS[N], dtype=np.int32)
    dev = e.tradeoff(N_RANGE, perm=perm, used=USED, end_iter=end, sets=sets, query=[0, 69])
    assert dev["n_unmatched"] == 1 and dev["n_matched"] == 6
    assert not _differences("perm", dev, R.tradeoff_reference(*r["samples"], perm=rows, sets=sets, query=[0, 69]))
    rel = np.asarray(e.relabel(N_RANGE, used=USED, end_iter=end)["perm"], dtype=np.int32)                     # bnmf_relabel's, a row per used sample
    perm[sel] = rel
    assert not _differences("relabel", e.tradeoff(N_RANGE, perm=perm, used=USED, end_iter=end), R.tradeoff_reference(*r["samples"], perm=rel))
    ident = np.tile(np.arange(N, dtype=np.int32), (N_RANGE, 1))
    assert not _differences("identity", e.tradeoff(N_RANGE, perm=ident, used=USED, end_iter=end), e.tradeoff(N_RANGE, used=USED, end_iter=end))


def test_include_gives_the_bits_of_the_cohort_cut_down(monkeypatch):
    r = _run("g70")
    e, G, N = r["e"], r["G"], r["N"]
    inc = np.ones(G, dtype=np.int32)
    inc[[0, 63, 64, G - 1]] = 0
    keep = np.where(inc == 1)[0]
    sets = np.array(SETS[N], dtype=np.int32)
    P, E, A = r["samples"]
    cut = R.tradeoff_reference(P, E[:, :, keep], A, sets=sets, query=[0, len(keep) - 1])                       # an engine on the remaining columns' samples
    for band in (None, "7"):
        if band:
            monkeypatch.setenv("BNMF_TRD_BAND", band)
        dev = e.tradeoff(N_RANGE, include=inc, sets=sets, query=[1, G - 2], used=USED, end_iter=r["end"])
        assert dev["n_left_out"] == 4 and dev["n_included"] == G - 4 and np.isnan(dev["tumour"][:, inc == 0]).all() and (dev["pair_at"][inc == 0] == -1).all()
        assert np.isnan(dev["setstat"][:, :, inc == 0]).all()
        sub = dict(dev, tumour=dev["tumour"][:, keep], pair_at=dev["pair_at"][keep], setstat=dev["setstat"][:, :, keep])
        assert not _differences(f"include, band {band}", sub, cut, info=tuple(k for k in INFO if k not in ("n_left_out",)))
        assert not _differences("include", dev, R.tradeoff_reference(P, E, A, include=inc, sets=sets, query=[1, G - 2]))


def test_at_is_the_plain_call_made_then_and_the_call_is_read_only():
    """twins: one calls tradeoff at iteration 12, both go on to 13; the other's _at call over the same range gives the same bits, and the
    chain that made the call continues with the bits of the one that had not"""
    a, b = _engine("g70", 12), _engine("g70", 12)
    q = _queries(70)
    sets = np.array(SETS[5], dtype=np.int32)
    then = a.tradeoff(N_RANGE, used=USED, sets=sets, query=q)
    assert not _differences("at(iter)", then, a.tradeoff_at(a.iter, N_RANGE, used=USED, sets=sets, query=q))
    ones = a.tradeoff_at(a.iter, N_RANGE, used=np.ones(N_RANGE, dtype=np.int32), include=np.ones(70, dtype=np.int32), sets=sets, query=q)
    assert not _differences("all ones", a.tradeoff(N_RANGE, sets=sets, query=q), ones)
    ra, rb = a.run(1), b.run(1)
    assert a.iter == 13 and np.array_equal(_bits(ra), _bits(rb))
    for nm in ("P", "E", "A"):
        assert np.array_equal(_bits(a.get(nm)), _bits(b.get(nm))), nm
    assert not _differences("inner range", b.tradeoff_at(12, N_RANGE, used=USED, sets=sets, query=q), then)
    assert not _differences("the case's", _run("g70")["e"].tradeoff(N_RANGE, used=USED, end_iter=12, sets=sets, query=q), then)
    # every output NULL: the info fields are the same
    from bayesnmf_amd.engine import lib, BnmfTradeoffInfo
    L, ip = lib(), C.POINTER(C.c_int32)
    info = BnmfTradeoffInfo()
    assert L.bnmf_tradeoff_at(b._h, 12, N_RANGE, USED.ctypes.data_as(ip), None, None, sets.ctypes.data_as(ip), 3, q.ctypes.data_as(ip), 3, 0.5, None, None, None, None,
                              None, C.byref(info)) == 0
    assert not _differences("all NULL", {k: getattr(info, k) for k in INFO}, then, arrays=())
    a.close(); b.close()


def test_refusals():
    from bayesnmf_amd import Engine
    from bayesnmf_amd.engine import lib, BnmfTradeoffInfo, BnmfError
    from bayesnmf_amd.setup import apply_hyperprior_params, synth_counts
    r = _run("g70")
    e, G, N, L = r["e"], r["G"], r["N"], lib()
    info = BnmfTradeoffInfo()
    ip = C.POINTER(C.c_int32)
    before = e.tradeoff(N_RANGE, used=USED, end_iter=r["end"], query=[3])

    def err():
        msg = L.bnmf_last_error().decode()
        assert msg
        return msg

    def call(n=10, used=None, include=None, perm=None, sets=None, Cn=None, query=None, Q=None, mc=0.5, inf=info, at=None, h=None):
        pt = lambda v: None if v is None else v.ctypes.data_as(ip)  # noqa: E731
        Q = (0 if query is None else len(query)) if Q is None else Q
        Cn = (0 if sets is None else int(sets.max()) + 1) if Cn is None else Cn
        f = None if inf is None else C.byref(inf)
        h = e._h if h is None else h
        rest = (pt(used), pt(include), pt(perm), pt(sets), Cn, pt(query), Q, mc, None, None, None, None, None, f)
        return L.bnmf_tradeoff(h, n, *rest) if at is None else L.bnmf_tradeoff_at(h, at, n, *rest)

    i32 = lambda v: np.array(v, dtype=np.int32)  # noqa: E731
    for at in (None, e.iter):
        assert call(inf=None, at=at) == -1 and "null" in err()                                       # BNMF_EINVAL
        u = np.ones(10, dtype=np.int32); u[6] = 2
        assert call(used=u, at=at) == -1 and "used[6] = 2" in err()
        inc = np.ones(G, dtype=np.int32); inc[64] = -1
        assert call(include=inc, at=at) == -1 and "include[64] = -1" in err()
        pm = np.tile(np.arange(N, dtype=np.int32), (10, 1)); pm[3, 1] = 0                             # a factor named twice
        assert call(perm=pm, at=at) == -1 and "perm[3]" in err() and "sample 3" in err()
        pm[3] = -1; pm[3, 0] = 2                                                                      # -1 in part
        assert call(perm=pm, at=at) == -1 and "perm[3]" in err()
        assert call(sets=i32([0, 1, 3, 0, 0]), Cn=3, at=at) == -1 and "sets[2] = 3" in err()
        assert call(sets=i32([0, -2, 1, 0, 0]), at=at) == -1 and "sets[1] = -2" in err()
        assert call(sets=i32([0, 2, 2, 0, 0]), at=at) == -1 and "set 1 is empty" in err()
        for bad in (-1, 33):
            assert call(sets=i32([0] * N), Cn=bad, at=at) == -1 and f"C = {bad}" in err()
        assert call(Cn=2, at=at) == -1 and "sets is null" in err()
        assert call(Q=-1, at=at) == -1 and "Q = -1" in err()
        assert call(Q=2, at=at) == -1 and "query is null" in err()
        assert call(query=i32([1, G]), at=at) == -1 and f"query[1] = {G}" in err()
        assert call(query=i32([-1]), at=at) == -1 and "query[0] = -1" in err()
        inc = np.ones(G, dtype=np.int32); inc[7] = 0
        assert call(include=inc, query=i32([3, 7]), at=at) == -1 and "query[1] = 7" in err() and "leaves out" in err()
        for bad in (float("nan"), -0.1, 1.5):
            assert call(mc=bad, at=at) == -1 and "min_corr" in err()
        u = np.zeros(10, dtype=np.int32); u[3] = 1
        assert call(used=u, at=at) == -2 and "1 used sample" in err()                                # BNMF_ESIZE
        pm = np.full((10, N), -1, dtype=np.int32); pm[5] = np.arange(N)
        assert call(perm=pm, at=at) == -2 and "1 matched sample" in err()
        assert call(include=np.zeros(G, dtype=np.int32), at=at) == -2 and "no included tumour" in err()
    assert call(n=W + 1) == -2 and err()
    assert call(n=5, at=e.iter + 1) == -2 and "are kept" in err()
    with pytest.raises(BnmfError, match="used has 3 entries"):
        e.tradeoff(10, used=[1, 1, 1])
    with pytest.raises(BnmfError, match="include has shape"):
        e.tradeoff(10, include=[1, 1, 1])
    with pytest.raises(BnmfError, match="sets has shape"):
        e.tradeoff(10, sets=[0, 0])
    with pytest.raises(BnmfError, match="perm is"):
        e.tradeoff(10, perm=np.zeros((3, N), dtype=np.int32))
    # window = 0: BNMF_ESTATE
    M, _, _ = synth_counts(8, 6, N, 21, mean_total=1500)
    z = Engine(M, N, prior="gamma", seed=4, window=0)
    apply_hyperprior_params(z, "gamma", M, N)
    z.init(); z.run(5)
    assert call(n=3, h=z._h) == -7 and "window = 0" in err()
    assert call(n=3, at=z.iter, h=z._h) == -7 and "window = 0" in err()
    z.close()
    # more factors than BNMF_TRD_MAX_N: BNMF_ESIZE, the limit named
    big = Engine(M, 129, prior="gamma", seed=4, window=4)
    apply_hyperprior_params(big, "gamma", M, 129)
    big.init(); big.run(3)
    assert call(n=3, h=big._h) == -2 and "N = 129 factors, at most 128" in err()
    assert call(n=3, at=big.iter, h=big._h) == -2 and "N = 129 factors, at most 128" in err()
    big.close()
    assert L.bnmf_version() == 100
    # the handle is usable afterwards: the same bits as before the refusals
    assert not _differences("afterwards", before, e.tradeoff(N_RANGE, used=USED, end_iter=r["end"], query=[3]))
