"""The geometry-fixed instantiations of k_zalloc_sort (csrc/zalloc_sort.h ZSFixed; round 6) against the dynamic form of the same kernel
(BNMF_ZSFIXED=0) and against the oracle, bit for bit: K = 96, N = 20, G = 2,000 — the smallest shape the planner routes to an
instantiation (8 columns per block, 4-byte items of 16 quads); the other one, the metric configuration's, runs one ragged case here beside
the regular data of tests/test_gpu_parity.py::test_full_size_chain_bitexact.  The switches are read at every bnmf_create: the two
forms are two handles of one process.  The planner's side of the choice is pinned on the host (tests/test_zsort_fixed_host.py).
WHICH FORM A HANDLE LAUNCHED IS INFERRED, NOT OBSERVED: no stat index reports it (the export list is pinned), so the tests check the
planner's tuple with a Python copy of zsort_fixed_form (takes_fixed_form) and trust build_zsort / launch_zsort_t to act on it; the
kernel names in profiles/r06_bench_kernel_stats_after.csv are the observation."""
import numpy as np
import pytest

from test_gpu_parity import _pair
from test_gpu_sparse_schedule import _bits, _n_cu, _sparse
from test_zsort_fixed_host import DATA_SEED, FIXED, plan_desc, takes_fixed_form

pytestmark = pytest.mark.gpu
K, G, N = 96, 2000, 20
CALLS = (2, 2, 2)


def _pin_2k_geometry(monkeypatch):
    """data whose cells are smaller than configuration 2's would get another item size by itself: the instantiation's, by the test switches"""
    monkeypatch.setenv("BNMF_ZSQMAX", "16")
    monkeypatch.setenv("BNMF_ZSIT16", "0")


def _plan_is_fixed(M, n=N, save_Z=False):
    return takes_fixed_form(plan_desc(M, n_cu=_n_cu(), save_Z=save_Z, n=n), M.shape[0], n)


def _chain(M, n, fixed, monkeypatch, save_Z=False, seed=3, nempty=None):
    """one engine chain in CALLS calls: after every call the arrays of the sweep and the metrics rows"""
    from bayesnmf_amd import Engine
    from bayesnmf_amd.setup import apply_hyperprior_params
    if fixed:
        monkeypatch.delenv("BNMF_ZSFIXED", raising=False)
    else:
        monkeypatch.setenv("BNMF_ZSFIXED", "0")
    e = Engine(M, n, prior="gamma", seed=seed, save_Z=save_Z)
    monkeypatch.delenv("BNMF_ZSFIXED", raising=False)
    apply_hyperprior_params(e, "gamma", M, n)
    assert e.stat(5) > 0, "the handle is not on the sorted schedule"
    if nempty is not None:
        assert e.stat(7) == nempty, "blocks without an own column"
    out = [e.init()[:9].copy()]
    for c in CALLS:
        met = e.run(c)
        out.append({"metrics": met[:, :9].copy(), **{nm: e.get(nm).copy() for nm in ("P", "E", "ZsumK", "ZsumG") + (("Z",) if save_Z else ())}})
    e.close()
    return out


def _same(a, b):
    assert np.array_equal(_bits(a[0]), _bits(b[0])), "init row"
    for i, (x, y) in enumerate(zip(a[1:], b[1:])):
        for nm in x:
            if x[nm].dtype.kind == "f":
                assert np.array_equal(_bits(x[nm]), _bits(y[nm])), (nm, i)
            else:
                assert np.array_equal(x[nm], y[nm]), (nm, i)


def _oracle_chain(M, n, seed=3):
    o, e = _pair(M, n, "gamma", seed=seed, save_Z=False)
    e.close()
    out = [o.init()[:9].copy()]
    for c in CALLS:
        met = o.run(c)
        out.append({"metrics": met[:, :9].copy(), "P": o.get("P").copy(), "E": o.get("E").copy(),
                    "ZsumK": o.get("ZsumK").astype(np.int32), "ZsumG": o.get("ZsumG").astype(np.int32)})
    o.close()
    return out


def _three_ways(M, monkeypatch, nempty=None):
    assert _plan_is_fixed(M), "the planner does not route this data to an instantiated geometry"
    fx, dyn = _chain(M, N, True, monkeypatch, nempty=nempty), _chain(M, N, False, monkeypatch, nempty=nempty)
    _same(fx, dyn)
    _same(fx, _oracle_chain(M, N))
    assert fx[-1]["ZsumK"].sum() == M.sum() == fx[-1]["ZsumG"].sum()


def test_fixed_form_selected(monkeypatch):
    """BASELINE's configuration 2 as bench.py draws it: the planner yields ZSFix2k's geometry by itself.  3 calls of 2 iterations."""
    from bayesnmf_amd.setup import synth_counts
    M, _, _ = synth_counts(K, G, 8, DATA_SEED + 2)
    d = plan_desc(M, n_cu=_n_cu())
    assert (d[1], d[2], d[6], d[5]) == FIXED[G]
    _three_ways(M, monkeypatch)


def test_ragged_tasks(monkeypatch):
    """Counts drawn so that the tasks of every block mix items of 1, 2 and 16 (= qmax) quads with cells of no counts, and last quads with 0,
    1, 2 and 3 pads: tasks whose common run of full quads is empty (1 and 2 quads side by side), tail tasks with lanes that have no
    quad at all (they skip the uniform loop), and the ragged remainder behind the uniform loop (16 quads beside the last fragment of a cell)."""
    _pin_2k_geometry(monkeypatch)
    rng = np.random.default_rng(41)
    kind = rng.choice(4, size=(K, G), p=[0.15, 0.3, 0.25, 0.3])
    M = np.where(kind == 0, 0, np.where(kind == 1, rng.integers(1, 5, size=(K, G)), np.where(kind == 2, rng.integers(5, 9, size=(K, G)),
                                                                                              rng.integers(61, 135, size=(K, G))))).astype(np.int32)
    M = np.asfortranarray(M)
    assert {int(m) & 3 for m in np.unique(M)} == {0, 1, 2, 3} and (M == 0).any() and M.max() > 4 * 16 * 2
    _three_ways(M, monkeypatch)


def test_columns_of_zeros_and_blocks_without_counts(monkeypatch):
    """The sparse generator of tests/test_gpu_sparse_schedule.py at this shape: 200 columns with counts, 1,800 of zeros.  56 blocks own only
    columns of zeros — all their tasks are cells without counts — and the others one column with counts and seven of zeros."""
    _pin_2k_geometry(monkeypatch)
    M = _sparse(G, 200)
    assert (M.sum(0) == 0).sum() == G - 200
    _three_ways(M, monkeypatch, nempty=0)


def test_columns_of_zeros_and_one_empty_block(monkeypatch):
    """Five columns with counts, 1,995 of zeros: the planner hands the columns of zeros to a block without load until it holds 8, so the 251
    blocks without a column with counts take 1,995 = 249 x 8 + 3 of them and ONE block is left with no column at all (ncols = 0, no task):
    its set-up reads the trailing entry of the column list, its epilogue adds nothing.  Still ZSFix2k's geometry."""
    _pin_2k_geometry(monkeypatch)
    M = _sparse(G, 5)
    assert (M.sum(0) > 0).sum() == 5
    d = plan_desc(M, n_cu=_n_cu())
    assert d[9] == 1 and (d[1], d[2], d[6], d[5]) == FIXED[G]
    _three_ways(M, monkeypatch, nempty=1)


def test_headline_instantiation_on_ragged_tasks(monkeypatch):
    """ZSFix10k (G = 10,000: 40 columns per block, 2-byte items of 64 quads) on ragged data: items of 1, 2 and 64 quads, cells without counts,
    every number of pads — the 2-byte item decode, the uniform loop and its remainder, and the tail tasks of that instantiation."""
    monkeypatch.setenv("BNMF_ZSQMAX", "64")
    rng = np.random.default_rng(43)
    G10 = 10000
    kind = rng.choice(4, size=(K, G10), p=[0.15, 0.4, 0.3, 0.15])
    M = np.where(kind == 0, 0, np.where(kind == 1, rng.integers(1, 5, size=(K, G10)), np.where(kind == 2, rng.integers(5, 9, size=(K, G10)),
                                                                                                rng.integers(250, 300, size=(K, G10))))).astype(np.int32)
    M = np.asfortranarray(M)
    d = plan_desc(M, n_cu=_n_cu())
    assert (d[1], d[2], d[6], d[5]) == FIXED[G10]
    _three_ways(M, monkeypatch, nempty=0)


@pytest.mark.parametrize("case", ["K = 95", "N = 21", "save_Z", "spread cell"])
def test_fallbacks_take_the_dynamic_form(case, monkeypatch):
    """Shapes beside the instantiated ones: the planner's geometry matches no instantiation, the handle runs the dynamic form with and
    without BNMF_ZSFIXED=0, and the two chains are the same bits — the selection does not take the fixed form for a geometry it was not built for."""
    from bayesnmf_amd.setup import synth_counts
    k, n, save_Z = (95 if case == "K = 95" else K), (21 if case == "N = 21" else N), case == "save_Z"
    M, _, _ = synth_counts(k, G, 8, DATA_SEED + 2)
    if case == "spread cell":
        M = M.copy()
        M[5, 7] = 9000                                                                # above 8,192: its fragments are spread, ZsumK has several writers
    assert not _plan_is_fixed(M, n, save_Z) or save_Z                                 # (save_Z: the same plan, refused by the record)
    a, b = _chain(M, n, True, monkeypatch, save_Z=save_Z), _chain(M, n, False, monkeypatch, save_Z=save_Z)
    _same(a, b)
    assert a[-1]["ZsumK"].sum() == M.sum()
    if save_Z:
        assert (a[-1]["Z"].sum(1) == M).all()
