"""bnmf_assign / bnmf_assign_at on the device (assign_impl in csrc/api.hip; k_ref_cosine, k_hungarian / hungarian_wave in
csrc/kernels.h) against their numerical spec restated in numpy float64 (map_ref.assign_reference: relabel_ref's cosines and its
shortest-augmenting-path solver with the lowest column among equal reduced costs, rectangular and transposed): votes, MAP_cosine and the
cosine bounds bit for bit, `assigned` exactly.  tests/test_gpu_assign.py keeps the independent comparison with scipy;
tests/test_map_host.py pins the restatement on the CPU (there the optimum was unique in every sample of every case but the tied
catalogue, where the tie rule alone decides).

The chains are tests/map_cases.py's (window = 16 at iteration 40: the range of 12 samples that ends at iteration 38 wraps the ring), with
the gapped `used` mask of tests/test_gpu_attribution.py and a keep mask with a gap: K = 8, N = 3 against R = 1, 2, 3, 7 (R below the
number of kept factors: the transposed solver); N = 70 against R = 3 (transposed, more columns than lanes) and R = 150 (several columns
per lane); the rank-learning chains with keep = A_mode and used = the samples at the mode (sbfi: the mode keeps nothing); a catalogue
with a duplicated column and a doubled one."""
import numpy as np
import pytest

import map_cases as MC
import map_ref as R
from test_map_host import ASSIGN_CASES, assign_inputs

pytestmark = pytest.mark.gpu

W, T_END, N_RANGE = MC.W, MC.T_END, MC.N_RANGE
END = T_END - 2
OUT = ("votes", "MAP_cosine", "lower_cosine", "upper_cosine")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


_RUNS = {}


def _run(case):
    """the chain at iteration 40 and the 12 samples that end at iteration 38: made once per case"""
    if case in _RUNS:
        return _RUNS[case]
    from bayesnmf_amd import Engine
    e, M = MC.create(Engine, case, window=W)
    e.init()
    e.run(T_END - 1, converged=MC.CASES[case][5])
    assert e.iter == T_END
    back = T_END - (END - N_RANGE)
    Pw, Ew, Aw = (np.stack(e.window(nm, back)[:N_RANGE]) for nm in ("P", "E", "A"))
    _RUNS[case] = dict(e=e, M=M, Pw=Pw, Ew=Ew, Aw=Aw.reshape(N_RANGE, e.N))
    return _RUNS[case]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for r in _RUNS.values():
        r["e"].close()
    _RUNS.clear()


def _differences(tag, a, b):
    """the names of the outputs of a that are not b's (printed with the first place they differ)"""
    bad = []
    for k in OUT:
        ne = _bits(a[k]) != _bits(b[k])
        if ne.any():
            i = tuple(np.argwhere(ne)[0])
            print(f"assign[{tag}] {k}: {int(ne.sum())} of {ne.size} differ, first at {i}: {np.asarray(a[k])[i]!r} against {np.asarray(b[k])[i]!r}")
            bad.append(k)
    if not np.array_equal(a["assigned"], b["assigned"]):
        print(f"assign[{tag}] assigned: {a['assigned']} against {b['assigned']}")
        bad.append("assigned")
    return bad


@pytest.mark.parametrize("case,Rn,keep", ASSIGN_CASES)
def test_every_output_is_the_restatement(case, Rn, keep):
    r = _run(case)
    e = r["e"]
    ref, kp, used = assign_inputs(case, Rn, keep, r["Pw"], r["Aw"], r["M"])
    Pu = r["Pw"][used == 1]
    MAP_P = R.series_mean(R.renormalised(Pu, r["Ew"][used == 1])[1])
    want = R.assign_reference(Pu, ref, kp, MAP_P, 0.9)
    got = e.assign(N_RANGE, ref, used=used, keep=kp, MAP_P=MAP_P, credible_interval=0.9, end_iter=END)
    nk, Rr = int(kp.sum()), ref.shape[1]
    print(f"assign[{case}, R = {Rn}, keep = {keep}] {int(used.sum())} samples, {nk} x {Rr}{', transposed' if nk > Rr else ''}: assigned {got['assigned'][:8]}")
    bad = _differences(f"{case}, R = {Rn}, keep = {keep}", got, want)
    again = e.assign(N_RANGE, ref, used=used, keep=kp, MAP_P=MAP_P, credible_interval=0.9, end_iter=END)      # a second call
    bad += _differences("second call", again, got)
    if case == "sbfi":
        assert nk == 0 and not got["votes"].any() and (got["assigned"] == -1).all()
    if case == "rank_n3":
        assert 2 <= used.sum() < N_RANGE and (np.diff(np.where(used)[0]) > 1).any() and 0 < nk < e.N
    if Rn == "tied":                                           # the duplicate with the lower index receives the votes
        assert got["votes"][:, [0, 1]].any() and not got["votes"][:, [2, 3]].any()
        assert sorted(got["assigned"]) == [0, 1, 4]
    assert not bad, bad


@pytest.mark.parametrize("case", ["pg_k8", "n70"])
def test_bnmf_assign_is_bnmf_assign_at_iter(case):
    r = _run(case)
    e = r["e"]
    ref = MC.catalogue(e.K, 7)
    a, b = e.assign(10, ref, credible_interval=0.9), e.assign(10, ref, credible_interval=0.9, end_iter=e.iter)
    assert not _differences("at iter", a, b)
    assert not _differences("used = NULL is all ones", a, e.assign(10, ref, used=np.ones(10, dtype=np.int32), keep=np.ones(e.N, dtype=np.int32), credible_interval=0.9))


@pytest.mark.parametrize("case,Rn", [("pg_k8", 3), ("pg_k8", 7), ("k7", 5), ("n70", 150), ("rank_n3", 4)])
def test_the_votes_are_the_cosines_of_bnmf_label_switching(case, Rn):
    """N <= R, every factor kept: the cosines bnmf_label_switching reports for the used iterations, added in sample order, are the votes"""
    r = _run(case)
    e = r["e"]
    ref = MC.catalogue(e.K, Rn)
    a = e.assign(N_RANGE, ref, used=MC.USED, end_iter=END)
    iters = (END - N_RANGE + 1) + np.where(MC.USED == 1)[0]
    ls = e.label_switching(iters, ref)
    votes = np.zeros((e.N, Rn))
    for s in range(len(iters)):
        for n in range(e.N):
            votes[n, ls["assigned"][s, n]] += ls["cosine"][s, n]
    assert np.array_equal(_bits(votes), _bits(a["votes"]))
    want = R.assign_reference(r["Pw"][MC.USED == 1], ref)
    assert np.array_equal(ls["assigned"], want["cols"]) and np.array_equal(_bits(ls["cosine"]), _bits(np.take_along_axis(want["cosines"], want["cols"][:, :, None].astype(np.int64), axis=2)[:, :, 0]))
