"""Fixed columns of P through the C ABI (bnmf_set_fixed), on the GPU, bit for bit against the CPU oracle composed one
conditional at a time (tests/test_fixed_host.py shows that the composed chain is the oracle's own).

Which case reaches which draw site (each case asserts the path it names from the handle's statistics, bnmf_get_stat):
  k_pdraw                      every Poisson Gibbs case at the small shapes (no launch of the merged draw kernel: statistic 10 == 0), rank
                               learning included, and "pdraw" of test_draw_sites (BNMF_GATE=0)
  k_draw::p_column             "merged" of test_draw_sites (BNMF_GATE=1, N = 20; statistic 10 > 0)
  k_draw::p_column_wave        "wave" of test_draw_sites (BNMF_GATE=1 + BNMF_DEBUG_DRAW_NO_P=1: the E workgroups draw the columns)
  allocation schedule `sort`   "pdraw" / "merged" / "wave" of test_draw_sites (N = 20: blocks of a static schedule that is not `step`);
                      `step`   "step" of test_draw_sites (N = 30; statistic 11)
  k_mh_prow hosted / two-kernel   test_all_fixed, test_partial_mh_and_normal, test_maintained_mhat (BNMF_MHPIPE default / 0; statistic 4)
  k_mh_prow REG / non-REG      G = 60 (statistic 9 == 1) / "mh_wide" of test_draw_sites (G = 5,200: 17 segments) and test_maintained_mhat (statistic 9 == 2)
  k_mh_prow MHSTEP / Normal    converged = True of the MH models / the two Normal models"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRIOR_NAMES = dict(gamma=["Alpha_p", "Beta_p", "Alpha_e", "Beta_e"], exponential=["Lambda_p", "Lambda_e"],
                   truncnormal=["Mu_p", "Sigmasq_p", "Mu_e", "Sigmasq_e"])
MODELS = {
    "poisson_gamma": ("poisson", "gamma", False), "poisson_exponential": ("poisson", "exponential", False),
    "poisson_exponential_mh": ("poisson", "exponential", True), "poisson_truncnormal_mh": ("poisson", "truncnormal", True),
    "normal_truncnormal": ("normal", "truncnormal", False), "normal_exponential": ("normal", "exponential", False),
}
T = 30
W = 40


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _cosmic(F, K=96):
    if K != 96:
        return np.random.default_rng(8).dirichlet(np.ones(K), size=F).T
    return np.ascontiguousarray(np.load(os.path.join(ROOT, "tests", "golden", "cosmic_v3.3.1_sbs.npz"))["P"][:, :F], dtype=np.float64)


def _temps():
    return np.concatenate([np.zeros(3), 10.0 ** np.linspace(-6, 0, 12), np.ones(1000)])


def _data(lk, K, G, seed=21):
    from bayesnmf_amd.setup import synth_counts
    if lk == "normal":
        rng = np.random.default_rng(seed)
        return np.asfortranarray(rng.gamma(1.0, 1.0, size=(K, 3)) @ rng.gamma(2.0, 4.0, size=(3, G)) + rng.normal(0.0, 0.5, size=(K, G)))
    return synth_counts(K, G, 3, seed, mean_total=1500 if G <= 100 else 4000)[0]


def _P0(K, N, mask, scale):
    """the initial P of both chains: the catalogue's columns where fixed, random positive ones elsewhere"""
    P = np.random.default_rng(17).gamma(1.0, 1.0, size=(K, N)) * scale
    F = int(np.sum(mask))
    P[:, np.flatnonzero(mask)] = _cosmic(max(F, 1), K)[:, :F] * (scale * K)
    return np.asfortranarray(P)


def _names(lk, prior, MH, save_Z=False):
    return (["P", "E", "A", "R"] + PRIOR_NAMES[prior] + (["sigmasq"] if lk == "normal" else [] if MH else ["ZsumK", "ZsumG"])
            + (["Z"] if save_Z else []))


def _chain(cls, model, M, N, rank, seed, save_Z, **kw):
    from bayesnmf_amd.setup import apply_hyperprior_params
    lk, prior, MH = MODELS[model]
    c = cls(M, N, likelihood=lk, prior=prior, MH=MH, learning_rank=rank is not None, rank_method=rank or "SBFI", seed=seed,
            temperature=_temps() if rank else None, save_Z=save_Z, **kw)
    apply_hyperprior_params(c, prior, M, N)
    return c


def _engine(model, M, N, rank, mask, P0, seed=4, save_Z=False, window=W):
    from bayesnmf_amd import Engine
    e = _chain(Engine, model, M, N, rank, seed, save_Z, window=window)
    if P0 is not None:
        e.set("P", P0)
    if mask is not None:
        e.set_fixed("P", mask)
    return e


def _steps(lk, MH, rank, skip_P):
    return ["hyper"] + ([] if skip_P else ["P"]) + ["E"] + (["R", "A"] if rank else []) + (["sigmasq"] if lk == "normal" else [] if MH else ["Z"])


def _against_oracle(model, rank, mask, K=96, G=60, N=6, converged=False, save_Z=False, nthreads=4, iters=T, expect=None):
    """engine with `mask` against the oracle composed without STEP_P (all fixed) or with STEP_P followed by restoring the fixed columns
    (some fixed; Poisson Gibbs only), after every iteration; the recorded samples of P at the end.  Returns the A history."""
    import oracle as O
    lk, prior, MH = MODELS[model]
    mask = np.asarray(mask, dtype=np.int32)
    allfix = bool(mask.all())
    assert allfix or (lk == "poisson" and not MH), "no composed reference for some fixed columns of a sequential sweep"
    M = _data(lk, K, G)
    P0 = _P0(K, N, mask, float(np.sqrt(np.mean(np.abs(M)) / N)) / K if K == 96 else 0.5)
    o = _chain(O.Oracle, model, M, N, rank, 4, save_Z, nthreads=nthreads)
    o.set("P", P0)
    e = _engine(model, M, N, rank, mask, P0, save_Z=save_Z)
    assert np.array_equal(e.get_fixed("P"), mask) and e.stat(8) == mask.sum()
    o.init(); e.init()
    fx = np.flatnonzero(mask)
    names = _names(lk, prior, MH, save_Z)
    A_hist = []
    for t in range(2, iters + 2):
        for what in _steps(lk, MH, rank, allfix):
            o.step(what, t, converged=converged)
            if what == "P":
                P = o.get("P"); P[:, fx] = P0[:, fx]; o.set("P", P)
        e.run(1, converged=converged)
        for nm in names:
            assert np.array_equal(_bits(o.get(nm)), _bits(e.get(nm))), (nm, t)
        A_hist.append(o.get("A").ravel().copy())
    for Pw in e.window("P", min(W, e.iter)):
        assert np.array_equal(_bits(Pw[:, fx]), _bits(P0[:, fx])), "a recorded sample of a fixed column differs from the input"
    if expect is not None:
        expect(e)                                            # the path the case names was the path taken
    e.close(); o.close()
    return np.array(A_hist)


# ---- 1. all of P fixed: every model family, fixed rank and SBFI / BFI, MH before and after convergence, both MH sweep forms
# (BNMF_MHPIPE only changes the Poisson MH sweep at fixed rank: the two-kernel form is asked for there)
ALL_FIXED = [(m, r, "default") for m in MODELS for r in (None, "SBFI", "BFI")] + [(m, None, "0") for m in MODELS if MODELS[m][2]]


@pytest.mark.parametrize("model,rank,pipe", ALL_FIXED)
def test_all_fixed(model, rank, pipe, monkeypatch):
    MH = MODELS[model][2]
    if pipe == "0":
        monkeypatch.setenv("BNMF_MHPIPE", "0")
    lk = MODELS[model][0]

    def expect(e):
        if lk == "poisson" and not MH:
            assert e.stat(10) == 0                           # k_pdraw, never the merged draw kernel
        else:
            assert e.stat(9) == 1                            # the register form of the row sweep
            hosted = MH and rank is None and pipe == "default"
            assert e.stat(4) == (1 if hosted else 0)
    for converged in ([False, True] if MH else [False]):
        _against_oracle(model, rank, np.ones(6), converged=converged, save_Z=(model == "poisson_gamma" and rank is None), expect=expect)


# ---- 2. some columns fixed, Poisson Gibbs: the oracle with STEP_P, then the fixed columns restored
@pytest.mark.parametrize("rank", [None, "SBFI", "BFI"])
@pytest.mark.parametrize("model", ["poisson_gamma", "poisson_exponential"])
def test_some_fixed_poisson_gibbs(model, rank):
    mask = np.array([1, 0, 1, 1, 0, 0])
    A = _against_oracle(model, rank, mask, save_Z=(rank is None), expect=lambda e: e.stat(10) == 0 or pytest.fail("merged draw kernel"))
    if rank is not None:
        assert (A[:, np.flatnonzero(mask)] == 0).any(), "no iteration with A[n] == 0 on a fixed column: the case does not test what it says"


# ---- 3. the other draw sites and schedules
@pytest.mark.parametrize("site", ["pdraw", "merged", "wave", "step", "mh_wide"])
def test_draw_sites(site, monkeypatch):
    if site in ("pdraw", "merged", "wave"):
        monkeypatch.setenv("BNMF_GATE", "0" if site == "pdraw" else "1")
        if site == "wave":
            monkeypatch.setenv("BNMF_DEBUG_DRAW_NO_P", "1")
        N = 20
        mask = (np.arange(N) % 3 != 1).astype(np.int32)

        def expect(e):
            assert e.stat(6) > 0 and e.stat(11) == 0, "not the sorted allocation schedule"
            if site == "pdraw":
                assert e.stat(10) == 0, "the merged draw kernel ran"
            else:
                assert e.stat(10) > 0, "the merged draw kernel never ran"
        _against_oracle("poisson_gamma", None, mask, G=900, N=N, nthreads=8, iters=12, expect=expect)
        _against_oracle("poisson_exponential", None, np.ones(N), G=900, N=N, nthreads=8, iters=12, expect=expect)
    elif site == "step":
        N = 30

        def expect(e):
            assert e.stat(11) == 1 and e.stat(10) == 0, "not k_zalloc_step behind k_pdraw"
        _against_oracle("poisson_gamma", None, (np.arange(N) % 2).astype(np.int32), N=N, expect=expect)
    else:
        def expect(e):
            assert e.stat(9) == 2, "not the form of the row sweep that keeps Mhat in memory"
        for converged in (False, True):
            _against_oracle("poisson_exponential_mh", None, np.ones(4), K=12, G=5200, N=4, converged=converged, iters=10, expect=expect)


# ---- 4. some columns fixed, MH and Normal models (sequential columns: no composed reference)
def _run_engine(model, mask, converged, called=True, P0=None, G=60, N=6):
    lk, prior, MH = MODELS[model]
    M = _data(lk, 96, G)
    if P0 is None:
        P0 = _P0(96, N, np.ones(N) if mask is None else mask, float(np.sqrt(np.mean(np.abs(M)) / N)) / 96)
    e = _engine(model, M, N, None, mask if called else None, P0)
    rows = [e.init()]
    rows += list(e.run(T, converged=converged))
    state = {nm: e.get(nm).copy() for nm in _names(lk, prior, MH)}
    win = e.window("P", T)
    e.close()
    return np.array(rows), state, win, P0


@pytest.mark.parametrize("model,converged", [("poisson_exponential_mh", False), ("poisson_exponential_mh", True), ("poisson_truncnormal_mh", False),
                                             ("poisson_truncnormal_mh", True), ("normal_truncnormal", False), ("normal_exponential", False)])
def test_partial_mh_and_normal(model, converged, monkeypatch):
    mask = np.array([1, 0, 1, 1, 0, 0], dtype=np.int32)
    fx, fr = np.flatnonzero(mask), np.flatnonzero(1 - mask)
    rows, st, win, P0 = _run_engine(model, mask, converged)
    for Pw in win:
        assert np.array_equal(_bits(Pw[:, fx]), _bits(P0[:, fx]))
    assert any(not np.array_equal(win[0][:, n], win[-1][:, n]) for n in fr), "the free columns are sampled"
    # a mask of zeros is the chain of a handle on which bnmf_set_fixed was never called, metric rows included
    r0, s0, _, _ = _run_engine(model, np.zeros(6, dtype=np.int32), converged, P0=P0)
    r1, s1, _, _ = _run_engine(model, None, converged, called=False, P0=P0)
    assert np.array_equal(_bits(r0), _bits(r1))
    for nm in s0:
        assert np.array_equal(_bits(s0[nm]), _bits(s1[nm])), nm
    # the two-kernel form of the sweep gives the bits of the default form
    monkeypatch.setenv("BNMF_MHPIPE", "0")
    r2, s2, _, _ = _run_engine(model, mask, converged, P0=P0)
    assert np.array_equal(_bits(rows), _bits(r2))
    for nm in st:
        assert np.array_equal(_bits(st[nm]), _bits(s2[nm])), nm


MHAT_CASES = [(m, c, form) for m, c in (("poisson_exponential_mh", False), ("poisson_exponential_mh", True), ("poisson_truncnormal_mh", False),
                                        ("poisson_truncnormal_mh", True), ("normal_truncnormal", False), ("normal_exponential", False))
              for form in (("small", "small_two_kernel", "wide") if MODELS[m][2] else ("small", "wide"))]


@pytest.mark.parametrize("model,converged,form", MHAT_CASES)
def test_maintained_mhat(model, converged, form, monkeypatch):
    """The independent check of the row sweep with SOME columns fixed (the columns are sequential: no composed oracle).
    (a) The row Mhat that k_mh_prow maintains factor by factor (fresh at the start of the sweep, then - old term + new term for every factor
    that is stepped; a fixed column's term is never touched) equals P_t diag(A) E_(t-1) formed afresh in numpy, to relative 1e-10 in every
    cell (the summation-order bound is K G 2^-53: 6e-13 at 96 x 60, 7e-12 at 12 x 5,200).  Read from the form of the kernel that keeps Mhat
    in memory: G = 5,200 ("wide"), or BNMF_MHREG=0 at G = 60.  A stale product behind a skipped column would leave the free columns'
    updates on the wrong Mhat.
    (b) At G = 60 the register form (the default there; its Mhat cannot be read) gives the bits of the memory form just checked, state
    and metric rows: the two are different code (the register form hands the exposures over one factor ahead) for one stream spec.
    Hosted and two-kernel launch, the MH step and the Normal model."""
    from bayesnmf_amd.engine import BnmfError
    lk, prior, MH = MODELS[model]
    K, G, N = (12, 5200, 6) if form == "wide" else (96, 60, 6)
    if form == "small_two_kernel":
        monkeypatch.setenv("BNMF_MHPIPE", "0")
    M = _data(lk, K, G)
    mask = np.array([1, 0, 1, 1, 0, 0], dtype=np.int32)
    fx = np.flatnonzero(mask)
    P0 = _P0(K, N, mask, float(np.sqrt(np.mean(np.abs(M)) / N)) / K if K == 96 else 0.5)
    names = _names(lk, prior, MH)

    def chain(read_mhat):
        e = _engine(model, M, N, None, mask, P0)
        assert e.stat(9) == (2 if read_mhat else 1)
        if form != "wide":
            assert e.stat(4) == (1 if MH and form == "small" else 0)   # hosted / two-kernel launch
        rows = [e.init()] + list(e.run(3, converged=converged))
        if not read_mhat:
            with pytest.raises(BnmfError, match="BNMF_MHREG") as ei:
                e.get("Mhat")
            assert ei.value.code == -3
        for t in range(10):
            E_prev, A = e.get("E"), e.get("A").ravel()
            rows += list(e.run(1, converged=converged))
            P = e.get("P")
            assert np.array_equal(_bits(P[:, fx]), _bits(P0[:, fx]))
            if read_mhat:
                Mh, ref = e.get("Mhat"), (P * A[None, :]) @ E_prev
                assert np.allclose(Mh, ref, rtol=1e-10, atol=0), float(np.max(np.abs(Mh - ref) - 1e-10 * np.abs(ref)))
        out = np.array(rows), {nm: e.get(nm).copy() for nm in names}
        e.close()
        return out
    if form == "wide":
        chain(True)
        return
    rows_reg, st_reg = chain(False)
    monkeypatch.setenv("BNMF_MHREG", "0")
    rows_mem, st_mem = chain(True)
    assert np.array_equal(_bits(rows_reg), _bits(rows_mem))
    for nm in names:
        assert np.array_equal(_bits(st_reg[nm]), _bits(st_mem[nm])), nm


def test_mask_of_zeros_is_no_mask_poisson_gibbs():
    for model in ("poisson_gamma", "poisson_exponential"):
        r0, s0, _, P0 = _run_engine(model, np.zeros(6, dtype=np.int32), False)
        r1, s1, _, _ = _run_engine(model, None, False, called=False, P0=P0)
        assert np.array_equal(_bits(r0), _bits(r1))
        for nm in s0:
            assert np.array_equal(_bits(s0[nm]), _bits(s1[nm])), nm


# ---- 5. metric rows of a fixed chain
@pytest.mark.parametrize("model", ["poisson_gamma", "poisson_exponential_mh", "normal_truncnormal"])
def test_metric_rows(model):
    lk, prior, MH = MODELS[model]
    K, G, N = 96, 60, 6
    M = _data(lk, K, G)
    mask = np.array([1, 1, 0, 1, 0, 0], dtype=np.int32)
    e = _engine(model, M, N, None, mask, _P0(K, N, mask, float(np.sqrt(np.mean(np.abs(M)) / N)) / K))
    e.init()
    Md = np.asarray(M, dtype=np.float64)
    for t in range(2, 12):
        row = e.run(1)[0]
        P, A, E = e.get("P"), e.get("A").ravel(), e.get("E")
        Mhat = (P * A[None, :]) @ E
        assert row[0] == t and row[7] == A.sum() and row[5] == A.sum() * (G + K)
        assert np.isclose(row[1], np.sqrt(np.mean((Mhat - Md) ** 2)), rtol=1e-10, atol=0)
        if lk == "poisson":
            from scipy.special import gammaln
            Mh, Mt = np.maximum(Mhat, 1e-6), np.maximum(Md, 1e-6)
            assert np.isclose(row[2], np.sum(Mt * np.log(Mt / Mh)), rtol=1e-10, atol=0)
            assert np.isclose(row[3], np.sum(Md * np.log(Mh) - Mh - gammaln(Md + 1.0)), rtol=1e-10, atol=0)
        else:
            sig = e.get("sigmasq").ravel()[None, :]
            assert np.isclose(row[3], np.sum(-0.5 * np.log(2 * np.pi * sig) - (Md - Mhat) ** 2 / (2 * sig)), rtol=1e-10, atol=0)
        assert np.isfinite(row[4])
    e.close()


# ---- 6. state file
@pytest.mark.parametrize("model", ["poisson_gamma", "poisson_exponential_mh", "normal_truncnormal"])
def test_state_file(model, tmp_path):
    from bayesnmf_amd.engine import BnmfError
    lk, prior, MH = MODELS[model]
    K, G, N = 96, 60, 6
    M = _data(lk, K, G)
    mask = np.array([0, 1, 1, 0, 1, 0], dtype=np.int32)
    P0 = _P0(K, N, mask, float(np.sqrt(np.mean(np.abs(M)) / N)) / K)
    a = _engine(model, M, N, None, mask, P0)
    a.init(); a.run(19)
    path = str(tmp_path / "s.bin")
    a.save_state(path)
    rows_a = a.run(15)
    # reopened without a mask: the file's is applied; with the same mask: accepted; with another: refused, the column named
    for given in (None, mask):
        b = _engine(model, M, N, None, given, None)
        assert b.load_state(path) == 20 and np.array_equal(b.get_fixed("P"), mask) and b.stat(8) == 3
        assert np.array_equal(_bits(rows_a), _bits(b.run(15)))
        for nm in _names(lk, prior, MH):
            assert np.array_equal(_bits(a.get(nm)), _bits(b.get(nm))), nm
        b.close()
    other = mask.copy(); other[3] = 1
    c = _engine(model, M, N, None, other, None)
    with pytest.raises(BnmfError, match="column 3") as ei:
        c.load_state(path)
    assert ei.value.code == -7 and c.iter == 0
    # refused before anything was written: the handle keeps its own mask and has no state
    assert np.array_equal(c.get_fixed("P"), other) and c.stat(8) == 4
    with pytest.raises(BnmfError) as ei:
        c.get("P")
    assert ei.value.code == -3
    c.close()
    # a loaded handle takes no mask any more
    b = _engine(model, M, N, None, None, None)
    b.load_state(path)
    with pytest.raises(BnmfError, match="initialised, loaded or run") as ei:
        b.set_fixed("P", mask)
    assert ei.value.code == -7 and np.array_equal(b.get_fixed("P"), mask)
    b.close(); a.close()


def test_reloaded_sampler_rebuilds_the_fixed_engine(tmp_path):
    """bayesNMF(save_engine_state = True, fixed_P = ...) stopped after a save, reopened with load_sampler: the engine carries the mask
    again (from specs["fixed_P"], checked against the file's), and the resumed run is the uninterrupted run bit for bit."""
    from bayesnmf_amd.sampler import bayesNMF, bayesNMF_sampler, load_sampler
    from bayesnmf_amd.convergence import new_convergence_control
    rng = np.random.default_rng(5)
    fp = _cosmic(3)
    M = np.asfortranarray(rng.poisson(fp @ rng.gamma(2.0, 150.0, size=(3, 50))), dtype=np.int32)

    def kw(name):
        return dict(rank=5, prior="gamma", fixed_P=fp, convergence_control=new_convergence_control(MAP_over=40, MAP_every=20, maxiters=200, miniters=40),
                    save_all_samples=True, output_dir=str(tmp_path / name), overwrite=True, seed=3, save_engine_state=True, periodic_save=True)
    full = bayesNMF(M, **kw("full"))

    class Stop(Exception):
        pass
    orig, n = bayesNMF_sampler.save_object, [0]

    def stopping(self):
        orig(self)
        n[0] += 1
        if n[0] == 2:
            raise Stop()
    bayesNMF_sampler.save_object = stopping
    try:
        with pytest.raises(Stop):
            bayesNMF(M, **kw("cut"))
    finally:
        bayesNMF_sampler.save_object = orig
    r = load_sampler(str(tmp_path / "cut"))
    assert np.array_equal(r.specs["fixed_P"], fp) and np.array_equal(r._chain.get_fixed("P"), [1, 1, 1, 0, 0]) and r._chain.stat(8) == 3
    assert r.state["iter"] < full.state["iter"]
    r.run_gibbs_sampler()
    a, b = full.state["sample_metrics"].to_numpy(dtype=float), r.state["sample_metrics"].to_numpy(dtype=float)
    assert a.shape == b.shape and np.array_equal(_bits(np.nan_to_num(a, nan=0.5)), _bits(np.nan_to_num(b, nan=0.5)))
    for nm in ("P", "E"):
        assert np.array_equal(_bits(full.params[nm]), _bits(r.params[nm])), nm
    for Pw in r.samples["P"]:
        assert np.array_equal(_bits(Pw[:, :3]), _bits(fp))
    full.close(); r.close()


# ---- 7. refusals
def test_refusals():
    import ctypes as C
    from bayesnmf_amd.engine import BnmfError, lib
    M = _data("poisson", 96, 60)
    N = 6
    mask = np.array([1, 0, 1, 0, 0, 0], dtype=np.int32)
    good = _P0(96, N, mask, 0.01)

    def fresh(P=None):
        e = _engine("poisson_gamma", M, N, None, None, P)
        return e

    e = fresh()
    ip = C.POINTER(C.c_int32)
    call = lambda idn, m: lib().bnmf_set_fixed(e._h, idn, np.ascontiguousarray(m, dtype=np.int32).ctypes.data_as(ip), len(m))   # noqa: E731
    err = lambda: lib().bnmf_last_error().decode()   # noqa: E731
    assert call(1, mask) == -6 and "out of scope" in err()                       # BNMF_EMODEL: E
    assert call(0, mask[:5]) == -2 and "5" in err()                              # BNMF_ESIZE
    assert call(0, [1, 0, 2, 0, 0, 0]) == -1 and "column 2" in err()             # BNMF_EINVAL, the column and the value named
    assert call(0, [1, 0, 0, 0, -1, 0]) == -1 and "column 4" in err()
    assert np.array_equal(e.get_fixed("P"), np.zeros(N)) and e.stat(8) == 0
    # bnmf_init: a fixed column without a value
    e.set_fixed("P", mask)
    with pytest.raises(BnmfError, match="column 0") as ei:
        e.init()
    assert ei.value.code == -3                                                   # BNMF_EUNSET: P never set
    e.close()
    for bad, code, col in ((np.nan, -3, 2), (-1.0, -1, 2), (np.inf, -1, 0)):
        P = good.copy(); P[5, col] = bad
        e = fresh(P); e.set_fixed("P", mask)
        with pytest.raises(BnmfError, match=f"column {col}") as ei:
            e.init()
        assert ei.value.code == code
        e.close()
    P = good.copy(); P[:, 2] = 0.0
    e = fresh(P); e.set_fixed("P", mask)
    with pytest.raises(BnmfError, match="column 2 of P sums to 0") as ei:
        e.init()
    assert ei.value.code == -1
    # a NaN in a column that is NOT fixed is no refusal: the column is drawn from the prior
    P = good.copy(); P[:, 1] = np.nan
    e2 = fresh(P); e2.set_fixed("P", mask); e2.init()
    P1 = e2.get("P")
    assert np.isfinite(P1).all() and np.array_equal(_bits(P1[:, [0, 2]]), _bits(good[:, [0, 2]])) and np.array_equal(_bits(P1[:, 3:]), _bits(good[:, 3:]))
    # a handle that has been initialised / run
    with pytest.raises(BnmfError) as ei:
        e2.set_fixed("P", mask)
    assert ei.value.code == -7
    e2.run(2)
    with pytest.raises(BnmfError) as ei:
        e2.set_fixed("P", mask)
    assert ei.value.code == -7
    e.close(); e2.close()


# ---- 8. end to end through bayesNMF()
def test_end_to_end_refit_and_rank_range(tmp_path):
    from bayesnmf_amd.sampler import bayesNMF
    from bayesnmf_amd.convergence import new_convergence_control
    rng = np.random.default_rng(101)
    F, G = 5, 80
    fp = _cosmic(F)
    E = rng.gamma(2.0, 150.0, size=(F, G))
    M = np.asfortranarray(rng.poisson(fp @ E), dtype=np.int32)
    cc = new_convergence_control(maxiters=600, miniters=100, MAP_over=100, MAP_every=50)
    s = bayesNMF(M, 5, likelihood="poisson", prior="gamma", fixed_P=fp, convergence_control=cc, output_dir=str(tmp_path / "refit"),
                 periodic_save=False, save_all_samples=False)
    assert np.allclose(s.MAP["P"], fp / fp.sum(axis=0)[None, :], rtol=0, atol=1e-14)
    s.assign_signatures_ensemble(fp)
    asg = s.reference_comparison["assignments"]
    assert list(asg["sig_ref"]) == [1, 2, 3, 4, 5]
    for col in ("MAP_cosine", "lower_cosine", "upper_cosine"):
        assert np.allclose(asg[col], 1.0, rtol=0, atol=1e-12), col
    ls = s.label_switching(fp)
    assert (ls["assigned"] == [f"Ref{int(k)}" for k in ls["k"]]).all() and np.allclose(ls["cosine_sim"], 1.0, rtol=0, atol=1e-12)
    s.close()
    s = bayesNMF(M, range(0, 8), likelihood="poisson", prior="gamma", fixed_P=fp, convergence_control=cc, output_dir=str(tmp_path / "range"),
                 periodic_save=False, save_all_samples=False)
    for Pw in s.samples["P"]:
        assert np.array_equal(_bits(Pw[:, :F]), _bits(fp))
    assert s.state["iter"] > 100 and np.isfinite(s.samples["P"][-1]).all()
    s.close()
