"""A chain's state in a file and back (bnmf_save_state / bnmf_load_state, Engine.save_state / load_state, load_sampler): a chain saved,
destroyed and reopened in a fresh handle continues bit for bit as the uninterrupted chain, in every sweep form; saving leaves the chain's
bits alone; deltas replay; refusals leave the handle usable; a reopened sampler post-processes and resumes as the live one."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")

PRIOR_NAMES = dict(gamma=["Alpha_p", "Beta_p", "Alpha_e", "Beta_e"], exponential=["Lambda_p", "Lambda_e"],
                   truncnormal=["Mu_p", "Sigmasq_p", "Mu_e", "Sigmasq_e"])
# name: likelihood, prior, MH, learning_rank, rank_method, save_Z, N, G
CASES = {
    "pg_sorted": ("poisson", "gamma", False, False, "SBFI", False, 6, 60),         # N <= 24: the sorted / register allocation
    "pg_step": ("poisson", "gamma", False, False, "SBFI", False, 30, 60),          # N = 30: k_zalloc_step
    "pe_mh": ("poisson", "exponential", True, False, "SBFI", False, 6, 60),        # the hosted MH sweep (mh_pipe)
    "ptn_mh": ("poisson", "truncnormal", True, False, "SBFI", False, 6, 60),
    "normal_tn": ("normal", "truncnormal", False, False, "SBFI", False, 5, 40),
    "normal_exp": ("normal", "exponential", False, False, "SBFI", False, 5, 40),
    "sbfi": ("poisson", "gamma", False, True, "SBFI", False, 6, 60),
    "bfi": ("poisson", "gamma", False, True, "BFI", False, 6, 60),
    "save_Z": ("poisson", "gamma", False, False, "SBFI", True, 6, 40),
}
W = 40


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _cosmic():
    return np.load(os.path.join(GOLD, "cosmic_v3.3.1_sbs.npz"))["P"]


def _data(case):
    from bayesnmf_amd.setup import synth_counts
    lk, *_, G = CASES[case]
    if lk == "normal":                                       # real-valued, negative cells included
        rng = np.random.default_rng(11)
        P, E = rng.gamma(1.0, 1.0, size=(96, 3)), rng.gamma(2.0, 4.0, size=(3, G))
        return np.asfortranarray(P @ E + rng.normal(0.0, 0.5, size=(96, G)))
    M, _, _ = synth_counts(96, G, 3, 21, mean_total=1500)
    return M


def _temps():
    return np.concatenate([np.zeros(3), 10.0 ** np.linspace(-6, 0, 30), np.ones(1000)])


def _engine(case, seed=4, chain_id=0, window=W, data=None):
    from bayesnmf_amd import Engine
    from bayesnmf_amd.setup import apply_hyperprior_params
    lk, prior, MH, lr, rm, sz, N, _ = CASES[case]
    M = _data(case) if data is None else data
    e = Engine(M, N, likelihood=lk, prior=prior, MH=MH, learning_rank=lr, rank_method=rm, seed=seed, chain_id=chain_id,
               window=window, save_Z=sz, temperature=_temps() if lr else None)
    return e, M


def _fresh(case, **kw):
    from bayesnmf_amd.setup import apply_hyperprior_params
    e, M = _engine(case, **kw)
    apply_hyperprior_params(e, CASES[case][1], M, CASES[case][6])
    e.init()
    return e


def _names(case):
    lk, prior, MH, *_ = CASES[case]
    return ["P", "E", "A", "R"] + PRIOR_NAMES[prior] + (["P_acceptance_rate", "E_acceptance_rate"] if MH else []) + \
        (["sigmasq"] if lk == "normal" else [])


def _same_state(a, b, case):
    assert a.iter == b.iter
    for nm in _names(case):
        assert np.array_equal(_bits(a.get(nm)), _bits(b.get(nm))), nm
    if CASES[case][0] == "poisson":
        for nm in ("ZsumK", "ZsumG"):
            assert np.array_equal(a.get(nm), b.get(nm)), nm
    if CASES[case][5]:
        assert np.array_equal(a.get("Z"), b.get("Z")), "Z"


def _same_reads(a, b, case):
    """every kept read: the window of every recorded name, map_at / assign_at on two ranges, label_switching"""
    n = min(W, a.iter)
    for nm in _names(case):
        wa, wb = a.window(nm, n), b.window(nm, n)
        assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(wa, wb)), f"window {nm}"
    if CASES[case][5]:
        assert all(np.array_equal(x, y) for x, y in zip(a.window("Z", n), b.window("Z", n))), "window Z"
    ref = _cosmic()
    for end, k in ((a.iter, n), (a.iter - 5, n - 10)):
        ma, mb = a.map(k, 0.9, end_iter=end), b.map(k, 0.9, end_iter=end)
        for key in ("P", "E", "A", "P_lower", "E_upper"):
            assert np.array_equal(_bits(ma[key]), _bits(mb[key])), f"map {key}"
        assert ma["top_counts"] == mb["top_counts"] and _bits(ma["rmse"]) == _bits(mb["rmse"])
        kw = dict(used=ma["used"].astype(np.int32), MAP_P=ma["P"], credible_interval=0.9, end_iter=end)
        sa, sb = a.assign(k, ref, **kw), b.assign(k, ref, **kw)
        for key in ("votes", "MAP_cosine", "lower_cosine", "upper_cosine"):
            assert np.array_equal(_bits(sa[key]), _bits(sb[key])), f"assign {key}"
        assert np.array_equal(sa["assigned"], sb["assigned"])
    iters = np.arange(a.iter - n + 1, a.iter + 1)
    la, lb = a.label_switching(iters, ref), b.label_switching(iters, ref)
    assert np.array_equal(la["assigned"], lb["assigned"]) and np.array_equal(_bits(la["cosine"]), _bits(lb["cosine"]))
    assert np.array_equal(la["included"], lb["included"])


def _conv(case, seg):
    return bool(CASES[case][2]) and seg > 0                  # MH: the later segments with true accept / reject


@pytest.mark.parametrize("case", list(CASES))
def test_continuity_save_destroy_load_run(case, tmp_path):
    """T1 iterations, save, destroy; a fresh handle loads and runs T2 more: bit-identical to T1 + T2 uninterrupted (arrays, metric
    rows, the whole window, map_at / assign_at / label_switching).  The chain that saved continues with the same bits too."""
    T1, T2 = 50, 30
    p = str(tmp_path / "s.bin")
    c = _fresh(case)                                         # never saves
    rc1 = c.run(T1, converged=_conv(case, 0))
    a = _fresh(case)
    ra1 = a.run(T1, converged=_conv(case, 0))
    assert np.array_equal(_bits(ra1), _bits(rc1))
    nbytes = a.save_state(p)
    assert nbytes == os.path.getsize(p)
    ra2 = a.run(T2, converged=_conv(case, 1))
    a.close()
    b, _ = _engine(case)
    assert b.load_state(p) == T1 + 1                         # (bnmf_init is iteration 1)
    _same_state(b, c, case)
    _same_reads(b, c, case)
    rc2 = c.run(T2, converged=_conv(case, 1))
    rb2 = b.run(T2, converged=_conv(case, 1))
    assert np.array_equal(_bits(rb2), _bits(rc2)), "metric rows after the load"
    assert np.array_equal(_bits(ra2), _bits(rc2)), "metric rows of the chain that saved"
    _same_state(b, c, case)
    _same_reads(b, c, case)
    b.close(); c.close()


@pytest.mark.parametrize("case", ["pg_sorted", "pe_mh", "sbfi"])
def test_deltas_replay_and_saving_every_block_changes_nothing(case, tmp_path):
    p = str(tmp_path / "d.bin")
    from bayesnmf_amd.engine import state_info
    c, a = _fresh(case), _fresh(case)
    since = 0
    for seg, T in enumerate((30, 25, 45)):                   # the last block wraps the ring past everything the first record held
        rc, ra = c.run(T, converged=_conv(case, seg)), a.run(T, converged=_conv(case, seg))
        assert np.array_equal(_bits(ra), _bits(rc))
        a.save_state(p, since_iter=since)
        since = a.iter
    info = state_info(p)
    assert (info["n_records"], info["first_iter"], info["last_iter"]) == (3, 31, 101) and info["bytes"] == os.path.getsize(p)
    with pytest.raises(Exception, match="since_iter"):
        a.save_state(p, since_iter=31)                       # the file ends at 101
    b, _ = _engine(case)
    assert b.load_state(p) == 101
    _same_state(b, c, case)
    _same_reads(b, c, case)
    assert np.array_equal(_bits(b.run(20, converged=_conv(case, 3))), _bits(c.run(20, converged=_conv(case, 3))))
    _same_state(b, c, case)
    a.close(); b.close(); c.close()


_CHILD = textwrap.dedent("""
    import sys, numpy as np
    sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
    import test_gpu_state as T
    b, _ = T._engine({case!r})
    b.load_state({path!r})
    rows = b.run(25, converged=False)
    np.savez({out!r}, rows=rows, **{{nm: b.get(nm) for nm in T._names({case!r})}})
""")


def test_restore_into_a_recycled_handle_and_in_a_fresh_process(tmp_path):
    """The restoring handle is created right after a different chain of the same shape was destroyed (its blocks come from the pool,
    still holding that chain's data); the same restore in a fresh child process; both equal the uninterrupted chain."""
    case = "pg_sorted"
    p, out = str(tmp_path / "r.bin"), str(tmp_path / "child.npz")
    a = _fresh(case)
    a.run(45)
    a.save_state(p)
    c = _fresh(case)
    c.run(45)
    other = _fresh(case, seed=99)                            # a different chain: its buffers go to the pool
    other.run(60)
    other.close()
    b, _ = _engine(case)
    b.load_state(p)
    rb = b.run(25)
    rc = c.run(25)
    assert np.array_equal(_bits(rb), _bits(rc))
    _same_state(b, c, case)
    script = _CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), case=case, path=p, out=out)
    r = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    z = np.load(out)
    assert np.array_equal(_bits(z["rows"]), _bits(rc))
    for nm in _names(case):
        assert np.array_equal(_bits(z[nm]), _bits(c.get(nm))), nm
    a.close(); b.close(); c.close()


def test_refusals_name_the_mismatch_and_leave_the_handle_usable(tmp_path):
    from bayesnmf_amd.engine import BnmfError
    case = "pg_sorted"
    p = str(tmp_path / "ok.bin")
    a = _fresh(case)
    a.run(30)
    a.save_state(p)
    a.run(5)
    a.save_state(p, since_iter=31)
    raw = open(p, "rb").read()
    M = _data(case)
    mism = [(dict(seed=5), "seed"), (dict(chain_id=1), "chain_id"), (dict(window=W + 1), "window"),
            (dict(data=M + (np.arange(M.size).reshape(M.shape, order="F") == 7)), "other data")]
    for kw, what in mism:
        e, _ = _engine(case, **kw)
        with pytest.raises(BnmfError, match=what):
            e.load_state(p)
        e.close()
    from bayesnmf_amd import Engine
    for kw, what in [(dict(N=7), "N = "), (dict(prior="exponential", MH=True), "prior"), (dict(save_Z=True), "save_Z")]:
        args = dict(prior="gamma", seed=4, window=W)
        N = kw.pop("N", 6)
        args.update(kw)
        e = Engine(M, N, **args)
        with pytest.raises(BnmfError, match=what):
            e.load_state(p)
        e.close()
    e = Engine(M[:, :50], 6, prior="gamma", seed=4, window=W)
    with pytest.raises(BnmfError, match="G = "):
        e.load_state(p)
    e.close()
    e = Engine(M, 6, prior="gamma", seed=4, window=W, learning_rank=True, temperature=_temps())
    with pytest.raises(BnmfError, match="learning_rank"):
        e.load_state(p)
    e.close()
    # bad files: magic, version, a flipped byte inside each record, a truncated file, a delta without its predecessor
    bad = {"magic": b"X" + raw[1:], "version": raw[:8] + b"\x07" + raw[9:], "flip0": bytearray(raw), "flip1": bytearray(raw),
           "trunc": raw[:len(raw) - 100], "head": raw[:60]}
    bad["flip0"][len(raw) // 3] ^= 0x10
    bad["flip1"][len(raw) - 200] ^= 0x01
    want = {"magic": "bad magic", "version": "format version", "flip0": "record 0 .*checksum", "flip1": "record 1 .*checksum",
            "trunc": "record 1 .*truncated", "head": "shorter than its header"}
    b, _ = _engine(case)
    for k, blob in bad.items():
        q = str(tmp_path / f"{k}.bin")
        open(q, "wb").write(bytes(blob))
        with pytest.raises(BnmfError, match=want[k]):
            b.load_state(q)
    assert b.load_state(p) == 36                             # the same handle, after every refusal
    _same_state(b, a, case)
    with pytest.raises(BnmfError, match="already run"):
        b.load_state(p)
    c = _fresh(case)
    with pytest.raises(BnmfError, match="already run"):
        c.load_state(p)
    a.close(); b.close(); c.close()


def test_two_saves_of_one_chain_are_the_same_bytes(tmp_path):
    for case in ("pe_mh", "save_Z", "normal_exp"):
        a = _fresh(case)
        a.run(45, converged=_conv(case, 1))
        p1, p2 = str(tmp_path / "1.bin"), str(tmp_path / "2.bin")
        a.save_state(p1)
        a.save_state(p2)
        assert open(p1, "rb").read() == open(p2, "rb").read(), case
        a.close()


# ------------------------------------------------------------------------------------------------ the Python sampler
def _sampler_kw(tmp_path, name, prior, MH=None):
    from bayesnmf_amd.convergence import new_convergence_control
    from bayesnmf_amd.setup import synth_counts
    M, _, _ = synth_counts(96, 40, 3, 5, mean_total=1500)
    cc = new_convergence_control(MAP_over=40, MAP_every=20, maxiters=200, miniters=40)
    return M, dict(rank=5, prior=prior, MH=MH, convergence_control=cc, save_all_samples=True, output_dir=str(tmp_path / name), overwrite=True, seed=3,
                   chain_id=2, post_warmup=60 if MH else None)


def test_reloaded_sampler_post_processes_as_the_live_one(tmp_path):
    from bayesnmf_amd.sampler import bayesNMF, load_sampler
    M, kw = _sampler_kw(tmp_path, "pp", "gamma")
    s = bayesNMF(M, save_engine_state=True, periodic_save=True, **kw)
    ref = _cosmic()
    r = load_sampler(kw["output_dir"])
    assert r.specs["seed"] == 3 and r.specs["chain_id"] == 2 and r.specs["window"] == len(s.temperature_schedule)
    assert r.state["iter"] == s.state["iter"]
    sa, sb = s.samples, r.samples
    for nm in sa:
        assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(sa[nm], sb[nm])), nm
    for args in (dict(), dict(end_iter=s.state["iter"] - 4, n_samples=30)):
        ma, mb = s.get_MAP(**args), r.get_MAP(**args)
        for k in ("P", "E", "A"):
            assert np.array_equal(_bits(ma[k]), _bits(mb[k])), k
        aa, ab = s.assign_signatures_ensemble(ref), r.assign_signatures_ensemble(ref)
        assert aa["assignments"].equals(ab["assignments"]) and aa["votes"].equals(ab["votes"])
    assert s.label_switching(ref).equals(r.label_switching(ref))
    s.close(); r.close()


@pytest.mark.parametrize("prior,MH", [("gamma", False), ("exponential", True)])
def test_resumed_run_is_the_uninterrupted_run(tmp_path, prior, MH):
    """bayesNMF(periodic_save = TRUE, save_engine_state = TRUE) stopped by an exception after a save, resumed with
    load_sampler(dir).run_gibbs_sampler(): the same sample_metrics, MAP_metrics, final MAP and assignment as an uninterrupted run
    (the MH case stops inside the post-warm-up tail)."""
    from bayesnmf_amd.sampler import bayesNMF, bayesNMF_sampler, load_sampler
    M, kw = _sampler_kw(tmp_path, "full", prior, MH)
    full = bayesNMF(M, save_engine_state=True, periodic_save=True, **kw)
    M, kw2 = _sampler_kw(tmp_path, "cut", prior, MH)

    class Stop(Exception):
        pass
    orig, n = bayesNMF_sampler.save_object, [0]

    def stopping(self):
        orig(self)
        n[0] += 1
        # Gibbs: after the second save; MH: at the first save inside the post-warm-up tail
        if (not MH and n[0] == 2) or (MH and 0 < self.state.get("post_warmup_done", 0) < self.specs["post_warmup"]):
            raise Stop()
    bayesNMF_sampler.save_object = stopping
    try:
        with pytest.raises(Stop):
            bayesNMF(M, save_engine_state=True, periodic_save=True, **kw2)
    finally:
        bayesNMF_sampler.save_object = orig
    r = load_sampler(kw2["output_dir"])
    if MH:
        assert r.state.get("post_warmup_done", 0) > 0, "the stop was meant to fall inside the tail"
    r.run_gibbs_sampler()
    for k in ("sample_metrics", "MAP_metrics"):
        a, b = full.state[k].to_numpy(dtype=float), r.state[k].to_numpy(dtype=float)
        assert a.shape == b.shape and np.array_equal(_bits(np.nan_to_num(a, nan=0.5)), _bits(np.nan_to_num(b, nan=0.5))), k
    for k in ("P", "E", "A"):
        assert np.array_equal(_bits(full.MAP[k]), _bits(r.MAP[k])), k
    ref = _cosmic()
    full.assign_signatures_ensemble(ref); r.assign_signatures_ensemble(ref)
    assert full.reference_comparison["assignments"].equals(r.reference_comparison["assignments"])
    full.close(); r.close()
