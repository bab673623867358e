"""Sparse per-tumour assignment with refit over a recorded range on the device (bnmf_prune / bnmf_prune_at, csrc/prune.h) against the
numerical spec restated in numpy float64 (tests/prune_ref.py, written from DESIGN.md 28): every output and every info field of every
case bit for bit, NaN compared as NaN, no tolerance — the operations are + - * /, sqrt, |.|, comparisons and whole numbers only; then
the equivalences and the refusals.

Every case is a Poisson-Gamma chain with window = 16 that runs to iteration 40, so the kept range wraps the ring; the range is the 6
samples that end 2 iterations before `iter`, with a `used` mask that has gaps (4 used).  The shapes are the smallest that reach each
path, because the restatement walks every problem in Python: N = 1 (no elimination), N = 5, N = 8 and 9 (the register forms of 8 and
16: the boundary of the padding), N = 17 and 25 (the forms of 24 and 32), N = 33 (the first past the registers: W and g in the LDS,
the accepted state in the device buffer), G = 1, G = 257 (one lane past a workgroup of 256), K = 1, an all-zero tumour and one with a
single non-zero cell, a rank-learning chain started with excluded factors (samples with A[n] = 0).  A column of P whose sum is 0
cannot be recorded by a chain (bnmf_init refuses a fixed column that sums to 0 and a Gamma draw is positive): that rule is k_proj_x's,
which tests/test_gpu_project.py holds, and tests/test_prune_host.py holds it on the restatement.

A permutation of the tumours: the rings cannot be written from outside and a chain on permuted data draws other samples, so on the
device this is held through include[] (a cohort without some tumours moves every later tumour to another lane, the same bits) and
through the restatement (a tumour's bits are the restatement's wherever it sits); the restatement's own invariance is in
tests/test_prune_host.py."""
import ctypes as C

import numpy as np
import pytest

import prune_ref as R

pytestmark = pytest.mark.gpu

W, T_END, N_RANGE = 16, 40, 6
USED = np.array([1, 1, 0, 1, 0, 1], dtype=np.int32)
ARRAYS = ("load", "tumour", "series", "signature", "exposures")
INFO = ("n_used", "n_included", "n_undefined", "n_single", "n_steps", "trials", "max_change", "max_loss")
STEPS, LOSS = 4, 0.01

# name: K, G, N, learning_rank, seed
CASES = {
    "n1": (6, 20, 1, False, 4),
    "n5": (8, 70, 5, False, 4),
    "n8": (6, 20, 8, False, 4),                # the register form of 8, no padding
    "n9": (6, 20, 9, False, 4),                # the register form of 16
    "n17": (6, 10, 17, False, 4),              # ... of 24
    "n25": (6, 10, 25, False, 4),              # ... of 32
    "n33": (5, 6, 33, False, 4),               # past the registers
    "g1": (6, 1, 3, False, 4),
    "g257": (4, 257, 3, False, 4),             # one lane past a workgroup
    "k1": (1, 20, 3, False, 4),
    "zeros": (8, 70, 5, False, 5),             # all-zero tumours, a tumour with a single non-zero cell
    "lr": (12, 8, 6, True, 14),                # samples with A[n] = 0
}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _data(case):
    from bayesnmf_amd.setup import synth_counts
    K, G, N, *_ = CASES[case]
    M, _, _ = synth_counts(K, G, min(3, N), 21, mean_total=1500)
    if case == "zeros":
        M = M.copy()
        M[:, 37] = 0
        M[:, 69] = 0                                                              # the last lane of the second wave
        M[:, 11] = 0
        M[3, 11] = 7                                                              # a single non-zero cell
    return M


def _fresh(case):
    from bayesnmf_amd import Engine
    from bayesnmf_amd.setup import apply_hyperprior_params
    K, G, N, lr, seed = CASES[case]
    M = _data(case)
    e = Engine(M, N, likelihood="poisson", prior="gamma", learning_rank=lr, seed=seed, window=W, temperature=np.ones(100) if lr else None)
    apply_hyperprior_params(e, "gamma", M, N)
    if lr:
        A0 = np.ones((1, N)); A0[0, 1::3] = 0.0                                   # start with a third of the factors excluded
        e.set("A", A0)
    row1 = e.init()
    return e, M, row1


_RUNS = {}


def _run(case):
    """the chain at iteration 40, its metric rows, the used samples of the range, the device's result and the restatement: once per case"""
    if case in _RUNS:
        return _RUNS[case]
    K, G, N, lr, _ = CASES[case]
    e, M, row1 = _fresh(case)
    rows = np.vstack([row1[None, :], e.run(T_END - 1)])
    assert e.iter == T_END
    end = T_END - 2
    back = T_END - (end - N_RANGE + 1) + 1
    sel = np.where(USED == 1)[0]
    win = {nm: np.stack([e.window(nm, back)[i] for i in sel]) for nm in ("P", "E", "A")}
    samples = (win["P"], win["E"], win["A"].reshape(len(sel), N))
    ref = R.prune_reference(*samples, M, n_steps=STEPS, max_loss=LOSS)
    dev = e.prune(N_RANGE, used=USED, end_iter=end, n_steps=STEPS, max_loss=LOSS, exposures=True)
    _RUNS[case] = dict(e=e, M=M, rows=rows, end=end, samples=samples, ref=ref, dev=dev)
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
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if x.shape != y.shape:
            print(f"prune[{tag}] {k}: shapes {x.shape} and {y.shape}")
            bad.append(k)
            continue
        nx, ny = np.isnan(x), np.isnan(y)
        ne = (nx != ny) | (~nx & ~ny & (_bits(x).reshape(x.shape) != _bits(y).reshape(y.shape)))
        if ne.any():
            i = tuple(np.argwhere(ne)[0])
            print(f"prune[{tag}] {k}: {int(ne.sum())} of {ne.size} differ, first at {i}: {x[i]!r} against {y[i]!r}")
            bad.append(k)
    for k in info:
        fa, fb = float(a[k]), float(b[k])
        if not ((np.isnan(fa) and np.isnan(fb)) or _bits(fa) == _bits(fb)):
            print(f"prune[{tag}] {k}: {a[k]!r} against {b[k]!r}")
            bad.append(k)
    return bad


def _same(a, b, arrays=ARRAYS, info=INFO):
    assert not _differences("equivalence", a, b, arrays, info)


@pytest.mark.parametrize("case", list(CASES))
def test_every_output_is_the_restatement_bit_for_bit(case, monkeypatch):
    r = _run(case)
    K, G, N, lr, _ = CASES[case]
    dev, ref, e = r["dev"], r["ref"], r["e"]
    S = int(USED.sum())
    print(f"prune[{case}] S {dev['n_used']} included {dev['n_included']} undefined {dev['n_undefined']} single {dev['n_single']} trials {dev['trials']} "
          f"max_change {dev['max_change']!r}; N_in {ref['n_in'].tolist()}; mean n_kept {dev['series'][0].round(3).tolist()}")
    assert dev["load"].shape == (4, N, G) and dev["tumour"].shape == (7, G) and dev["series"].shape == (2, S) and dev["signature"].shape == (3, N)
    assert dev["exposures"].shape == (S, N, G)
    bad = _differences(case, dev, ref)
    live = ~np.isnan(dev["tumour"][0])
    assert (dev["tumour"][1][live] >= dev["tumour"][0][live] - LOSS - 1e-12).all() and (dev["tumour"][3][live] >= 1).all()   # (means of per-sample values that hold it exactly)
    gone = dev["exposures"][:, :, live] == 0
    assert not np.signbit(dev["exposures"][:, :, live][gone]).any()                # a removed factor is +0.0
    if case == "zeros":
        assert dev["n_undefined"] == 2 and np.isnan(dev["tumour"][:, [37, 69]]).all() and np.isnan(dev["load"][:, :, [37, 69]]).all()
        assert np.isnan(dev["exposures"][:, :, [37, 69]]).all() and int(np.isnan(dev["tumour"][0]).sum()) == 2
        assert not np.isnan(dev["tumour"][:, 11]).any() and dev["tumour"][4, 11] >= 1
    if case == "lr":
        A = r["samples"][2]
        assert (A == 0).any(), "no used sample excludes a factor"
        assert (dev["exposures"][A == 0] == 0).all() and not np.signbit(dev["exposures"][A == 0]).any()
    if case == "n1":
        assert dev["trials"] == 0 and (dev["tumour"][2] == 1).all()
    # the other form of the kernel and other batches of samples: the same bits
    kw = dict(used=USED, end_iter=r["end"], n_steps=STEPS, max_loss=LOSS, exposures=True)
    for env in ({"BNMF_PRN_FORM": "1"}, {"BNMF_PRN_BATCH": "1"}, {"BNMF_PRN_BATCH": "3"}, {"BNMF_PRN_FORM": "1", "BNMF_PRN_BATCH": "3"}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        bad += _differences(f"{case}, {env}", e.prune(N_RANGE, **kw), ref)
        for k in env:
            monkeypatch.delenv(k)
    assert not bad, bad


@pytest.mark.parametrize("max_loss", [-2.0, 0.0, 2.0])
def test_other_thresholds(max_loss):
    r = _run("n5")
    e, N = r["e"], CASES["n5"][2]
    d = e.prune(N_RANGE, used=USED, end_iter=r["end"], n_steps=STEPS, max_loss=max_loss, exposures=True)
    ref = R.prune_reference(*r["samples"], r["M"], n_steps=STEPS, max_loss=max_loss)
    _same(d, ref)
    if max_loss == -2.0:                                                          # nothing is removed: every candidate of the one round is tried
        assert (d["tumour"][2] == N).all() and (d["tumour"][6] == N).all() and d["n_single"] == 0
    if max_loss == 2.0:                                                           # every tumour ends with one signature, one trial per round
        assert (d["tumour"][4] == 1).all() and (d["tumour"][6] == N - 1).all() and d["n_single"] == CASES["n5"][1]
        assert ((d["exposures"] > 0).sum(axis=1) <= 1).all()


def test_include_gives_the_bits_of_the_cohort_without_the_tumours_left_out():
    r = _run("zeros")
    e, M = r["e"], r["M"]
    K, G, N, *_ = CASES["zeros"]
    inc = np.ones(G, dtype=np.int32)
    inc[[0, 5, 37, 40, 64]] = 0
    d = e.prune(N_RANGE, include=inc, used=USED, end_iter=r["end"], n_steps=STEPS, max_loss=LOSS, exposures=True)
    _same(d, R.prune_reference(*r["samples"], M, n_steps=STEPS, max_loss=LOSS, include=inc))
    keep = inc == 1
    P, E, A = r["samples"]
    sub = R.prune_reference(P, E[:, :, keep], A, M[:, keep], n_steps=STEPS, max_loss=LOSS)      # the cohort without them
    assert d["n_included"] == int(keep.sum()) and d["n_undefined"] == 1
    got = dict(load=d["load"][:, :, keep], tumour=d["tumour"][:, keep], series=d["series"], signature=d["signature"], exposures=d["exposures"][:, :, keep],
               **{k: d[k] for k in INFO})
    _same(got, sub)
    assert np.isnan(d["load"][:, :, ~keep]).all() and np.isnan(d["tumour"][:, ~keep]).all() and np.isnan(d["exposures"][:, :, ~keep]).all()
    # a tumour's own rows are the full cohort's: its place among the lanes does not matter
    full = r["dev"]
    live = keep & ~np.isnan(full["tumour"][0])
    assert np.array_equal(_bits(d["load"][:, :, live]), _bits(full["load"][:, :, live])) and np.array_equal(_bits(d["tumour"][:, live]), _bits(full["tumour"][:, live]))


def test_one_sample_and_an_inner_range():
    r = _run("n5")
    e, M = r["e"], r["M"]
    K, G, N, *_ = CASES["n5"]
    end = r["end"] - 3
    P, E, A = (np.stack(e.window(nm, T_END - end + 1)[:1]) for nm in ("P", "E", "A"))           # iteration `end` alone
    d = e.prune_at(end, 1, n_steps=STEPS, max_loss=LOSS, exposures=True)
    ref = R.prune_reference(P, E, A.reshape(1, N), M, n_steps=STEPS, max_loss=LOSS)
    _same(d, ref)
    assert d["n_used"] == 1 and np.isnan(d["load"][1]).all() and not np.isnan(d["load"][0]).any()  # one sample has no variance
    u = np.zeros(5, dtype=np.int32); u[4] = 1
    _same(e.prune_at(end, 5, used=u, n_steps=STEPS, max_loss=LOSS, exposures=True), ref)


@pytest.mark.parametrize("case", ["n5", "lr"])
def test_equivalent_calls_give_the_same_bits(case):
    r = _run(case)
    e, end = r["e"], r["end"]
    K, G, N, *_ = CASES[case]
    kw = dict(n_steps=STEPS, max_loss=LOSS, exposures=True)
    _same(r["dev"], e.prune(N_RANGE, used=USED, end_iter=end, **kw))                             # a second call
    _same(e.prune(5, **kw), e.prune(5, end_iter=e.iter, **kw))                                   # bnmf_prune is bnmf_prune_at(iter)
    _same(e.prune(5, **kw), e.prune_at(e.iter, 5, used=np.ones(5, dtype=np.int32), include=np.ones(G, dtype=np.int32), **kw))   # NULL is all ones
    # each output NULL in turn, then all of them: the others and the info fields are the same
    from bayesnmf_amd.engine import lib, BnmfPruneInfo
    L, dp, ip = lib(), C.POINTER(C.c_double), C.POINTER(C.c_int32)
    S = int(USED.sum())
    for skip in ARRAYS + ("all",):
        bufs = dict(load=np.full((4, G, N), -7.0), tumour=np.full((7, G), -7.0), series=np.full((2, S), -7.0), signature=np.full((3, N), -7.0),
                    exposures=np.full((S, G, N), -7.0))
        ptr = {k: (None if skip in (k, "all") else v.ctypes.data_as(dp)) for k, v in bufs.items()}
        info = BnmfPruneInfo()
        assert L.bnmf_prune_at(e._h, end, N_RANGE, USED.ctypes.data_as(ip), None, STEPS, LOSS, ptr["load"], ptr["tumour"], ptr["series"], ptr["signature"],
                               ptr["exposures"], C.byref(info)) == 0
        got = dict(load=bufs["load"].transpose(0, 2, 1), tumour=bufs["tumour"], series=bufs["series"], signature=bufs["signature"],
                   exposures=bufs["exposures"].transpose(0, 2, 1), **{k: getattr(info, k) for k in INFO})
        for k in ARRAYS:
            if skip in (k, "all"):
                assert (bufs[k] == -7).all(), k                                                   # (not written)
        _same(got, r["dev"], tuple(k for k in ARRAYS if skip not in (k, "all")))


def test_refusals():
    from bayesnmf_amd import Engine
    from bayesnmf_amd.engine import lib, BnmfPruneInfo, BnmfError
    from bayesnmf_amd.setup import apply_hyperprior_params
    r = _run("n5")
    e, M, L = r["e"], r["M"], lib()
    K, G, N, *_ = CASES["n5"]
    info = BnmfPruneInfo()
    ip = C.POINTER(C.c_int32)

    def err():
        msg = L.bnmf_last_error().decode()
        assert msg
        return msg

    def call(n=5, used=None, inc=None, steps=STEPS, loss=LOSS, inf=info, at=None, h=None):
        u = None if used is None else used.ctypes.data_as(ip)
        i = None if inc is None else inc.ctypes.data_as(ip)
        tail = (u, i, steps, loss, None, None, None, None, None, None if inf is None else C.byref(inf))
        h = e._h if h is None else h
        return L.bnmf_prune(h, n, *tail) if at is None else L.bnmf_prune_at(h, at, n, *tail)

    for at in (None, e.iter):
        assert call(inf=None, at=at) == -1 and "null" in err()                                       # BNMF_EINVAL
        u = np.ones(5, dtype=np.int32); u[3] = 2
        assert call(used=u, at=at) == -1 and "used[3] = 2" in err()
        inc = np.ones(G, dtype=np.int32); inc[6] = -1
        assert call(inc=inc, at=at) == -1 and "include[6] = -1" in err()
        for bad in (0, -3, 100001):
            assert call(steps=bad, at=at) == -1 and "n_steps" in err()
        for bad in (float("nan"), float("inf"), -float("inf")):
            assert call(loss=bad, at=at) == -1 and "max_loss" in err()
        assert call(used=np.zeros(5, dtype=np.int32), at=at) == -2 and "no used sample" in err()     # BNMF_ESIZE
        assert call(inc=np.zeros(G, dtype=np.int32), at=at) == -2 and "no included tumour" in err()
    assert call(n=0) == -2 and err()
    assert call(n=W + 1) == -2 and err()
    # the range rule of bnmf_project_at: iterations [max(1, iter - window + 1), iter]
    assert call(n=5, at=e.iter + 1) == -2 and "are kept" in err()
    assert call(n=W + 1, at=e.iter) == -2 and "are kept" in err()
    assert call(n=3, at=e.iter - W + 1) == -2 and "are kept" in err()
    with pytest.raises(BnmfError, match="used has 3 entries"):
        e.prune(5, used=[1, 1, 1])
    with pytest.raises(BnmfError, match="include has shape"):
        e.prune(5, include=[1, 1, 1])
    # the Normal likelihood: BNMF_EMODEL, as bnmf_project
    rng = np.random.default_rng(11)
    Mn = np.asfortranarray(rng.gamma(1.0, 1.0, size=(6, 3)) @ rng.gamma(0.5, 1.0, size=(3, 10)) + rng.normal(0.0, 0.5, size=(6, 10)))
    z = Engine(Mn, 3, likelihood="normal", prior="exponential", seed=4, window=W)
    apply_hyperprior_params(z, "exponential", Mn, 3)
    z.init(); z.run(5)
    for at in (None, z.iter):
        assert call(n=3, h=z._h, at=at) == -6 and "Normal likelihood" in err()
    z.close()
    # window = 0: BNMF_ESTATE
    z = Engine(M, 3, prior="gamma", seed=4, window=0)
    apply_hyperprior_params(z, "gamma", M, 3)
    z.init(); z.run(5)
    assert call(n=3, h=z._h) == -7 and "window = 0" in err()
    z.close()
    assert L.bnmf_version() == 100
    # the handle is usable afterwards: the same bits as before the refusals
    _same(r["dev"], e.prune(N_RANGE, used=USED, end_iter=r["end"], n_steps=STEPS, max_loss=LOSS, exposures=True))


@pytest.mark.parametrize("case", ["g257", "lr"])
def test_the_call_is_read_only_for_the_chain(case):
    """a chain that calls prune mid-run continues with the bits of a twin that never did"""
    r = _run(case)
    b, _, row1 = _fresh(case)
    rows_b = np.vstack([row1[None, :], b.run(T_END - 1)])
    assert np.array_equal(_bits(rows_b), _bits(r["rows"]))
    more_a, more_b = r["e"].run(10), b.run(10)                                    # a called prune at iteration 40, b never did
    assert np.array_equal(_bits(more_a), _bits(more_b))
    for nm in ("P", "E", "A"):
        assert np.array_equal(_bits(r["e"].get(nm)), _bits(b.get(nm))), nm
    b.close()
    _RUNS.pop(case)["e"].close()                                                  # (this chain has moved on)
