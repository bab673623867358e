"""Both words of the Philox key through every kernel family.  The key of a chain is (seed_lo, seed_hi ^ chain_id); it is
copied into the argument struct of every kernel family by hand.  With seeds below 2^32 and chain 0 the second word is 0 and the
first is small, so a kernel that dropped or swapped a word, or sign-extended one, would agree with the oracle all the same.  Here one
small case per family runs with the key (1, 0) and with a seed and a chain id that give two different words with their top bits set."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KEYS = {"key_1_0": (1, 0), "key_wide": (0x9E3779B97F4A7C15, 0x80000001)}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _temps(n=60):
    return np.concatenate([np.zeros(3), 10.0 ** np.linspace(-6, 0, 12), np.ones(n)])


GIBBS = dict(prior="gamma")
MH_TN = dict(prior="truncnormal", MH=True)
# family: shape (K, G, N), model, environment, which save_Z, the statistic (bnmf_get_stat) that names the path, calls [(iterations, converged)]
CASES = {
    "alloc_general": dict(shape=(33, 17, 26), model=GIBBS, env=dict(BNMF_ZSTEP="0", BNMF_ZTILE="0", BNMF_ZCHUNK="1"), save_Z=(False, True)),
    "alloc_register": dict(shape=(96, 40, 9), model=GIBBS, env=dict(BNMF_ZSORT="0"), save_Z=(False, True), stat=(5, 0.0)),
    "alloc_tile": dict(shape=(33, 17, 26), model=GIBBS, env=dict(BNMF_ZSTEP="0"), save_Z=(False, True), stat=(11, 0.0)),
    "alloc_step": dict(shape=(200, 9, 30), model=GIBBS, save_Z=(False,), stat=(11, 1.0)),
    "alloc_sorted": dict(shape=(96, 40, 9), model=GIBBS, save_Z=(False, True), stat=(6, None)),
    "draw_merged": dict(shape=(96, 700, 12), model=GIBBS, env=dict(BNMF_GATE="1"), calls=[(1, False), (2, False), (5, False)], stat=(10, None),
                        excluded=[7]),
    "draw_split": dict(shape=(96, 700, 12), model=GIBBS, env=dict(BNMF_GATE="0"), calls=[(1, False), (2, False), (5, False)], stat=(10, 0.0),
                       excluded=[7]),
    "mh_row_ecol16_hosted_tail": dict(shape=(96, 70, 6), model=MH_TN, calls=[(4, False), (4, True)], stat=(4, 1.0)),
    "mh_tail_kernel": dict(shape=(96, 70, 6), model=MH_TN, env=dict(BNMF_MHPIPE="0"), calls=[(4, False), (4, True)], stat=(4, 0.0)),
    "mh_ecol": dict(shape=(130, 9, 3), model=dict(prior="exponential", MH=True), calls=[(4, False), (4, True)]),
    "rank_register": dict(shape=(96, 120, 8), model=dict(prior="gamma", learning_rank=True), calls=[(15, False), (15, False)]),
    "rank_general": dict(shape=(96, 40, 50), model=dict(prior="gamma", learning_rank=True), calls=[(12, False), (8, False)]),
    "normal": dict(shape=(60, 40, 4), model=dict(prior="truncnormal", likelihood="normal"), calls=[(5, False), (5, False)]),
}


def _counts(K, G):
    rng = np.random.default_rng(K * 1000 + G)
    M = rng.poisson(rng.gamma(0.6, 25.0, size=(K, G))).astype(np.int32)
    M[:, G // 2] = 0
    M[K // 3, :] = 0
    M[1, 1] = 1500
    return np.asfortranarray(M)


@pytest.mark.parametrize("key", list(KEYS))
@pytest.mark.parametrize("family", list(CASES))
def test_kernel_family_with_key(family, key, monkeypatch):
    import oracle as O
    from bayesnmf_amd import Engine
    from bayesnmf_amd.setup import apply_hyperprior_params
    case = CASES[family]
    seed, chain = KEYS[key]
    K, G, N = case["shape"]
    model = dict(case["model"])
    for k, v in case.get("env", {}).items():
        monkeypatch.setenv(k, v)
    if model.get("learning_rank"):
        model["temperature"] = _temps()
    M = _counts(K, G)
    gibbs = not model.get("MH") and model.get("likelihood", "poisson") == "poisson"
    calls = case.get("calls", [(4, False)])
    for save_Z in case.get("save_Z", (False,)):
        o = O.Oracle(M, N, seed=seed, chain_id=chain, save_Z=gibbs, nthreads=8, **model)
        e = Engine(M, N, seed=seed, chain_id=chain, save_Z=save_Z, **model)
        for c in (o, e):
            apply_hyperprior_params(c, model["prior"], M, N)
            if case.get("excluded"):
                A0 = np.ones((1, N)); A0[0, case["excluded"]] = 0.0
                c.set("A", A0)
        r0, r1 = o.init(), e.init()
        assert np.array_equal(_bits(r0[:9]), _bits(r1[:9])), "metrics row of init"
        for n_it, conv in calls:
            mo, me = o.run(n_it, converged=conv), e.run(n_it, converged=conv)
            names = ["P", "E", "A"] + (["ZsumK", "ZsumG"] if gibbs else []) + (["Z"] if save_Z else []) + \
                (["sigmasq"] if model.get("likelihood") == "normal" else []) + (["P_acceptance_rate", "E_acceptance_rate"] if model.get("MH") else [])
            for nm in names:
                assert np.array_equal(_bits(o.get(nm)), _bits(e.get(nm))), (nm, save_Z, conv)
            assert np.array_equal(_bits(mo[:, :9]), _bits(me[:, :9])), (save_Z, conv)
        if "stat" in case:
            what, want = case["stat"]
            assert (e.stat(what) > 0) if want is None else (e.stat(what) == want), (what, e.stat(what))
        e.close(); o.close()


@pytest.mark.parametrize("key", list(KEYS))
def test_fixed_columns_of_P_with_key(key):
    """Every column of P held fixed (bnmf_set_fixed): the oracle composed of the other conditionals, one at a time."""
    import oracle as O
    from bayesnmf_amd import Engine
    from bayesnmf_amd.setup import apply_hyperprior_params
    seed, chain = KEYS[key]
    K, G, N = 96, 60, 6
    M = _counts(K, G)
    P0 = np.asfortranarray(np.random.default_rng(17).gamma(1.0, 1.0, size=(K, N)) * (np.sqrt(M.mean() / N) / K))
    o = O.Oracle(M, N, prior="gamma", seed=seed, chain_id=chain, save_Z=True, nthreads=4)
    e = Engine(M, N, prior="gamma", seed=seed, chain_id=chain)
    for c in (o, e):
        apply_hyperprior_params(c, "gamma", M, N)
        c.set("P", P0)
    e.set_fixed("P", np.ones(N, dtype=np.int32))
    o.init(); e.init()
    for t in range(2, 8):
        for what in ("hyper", "E", "Z"):
            o.step(what, t)
        e.run(1)
        for nm in ("P", "E", "ZsumK", "ZsumG", "Alpha_e", "Beta_p"):
            assert np.array_equal(_bits(o.get(nm)), _bits(e.get(nm))), (nm, t)
    assert np.array_equal(_bits(e.get("P")), _bits(P0))
    e.close()


def test_chain_id_alone_separates_replicas():
    """run_chains gives its replicas one seed and the chain ids 0, 1, ...: with a 64-bit seed the two chains differ after one iteration,
    and each is its oracle's chain."""
    import oracle as O
    from bayesnmf_amd import Engine
    from bayesnmf_amd.setup import apply_hyperprior_params
    seed = KEYS["key_wide"][0]
    M = _counts(96, 40)
    P = []
    for chain in (0, 1):
        o = O.Oracle(M, 5, prior="gamma", seed=seed, chain_id=chain, nthreads=4)
        e = Engine(M, 5, prior="gamma", seed=seed, chain_id=chain)
        for c in (o, e):
            apply_hyperprior_params(c, "gamma", M, 5)
        o.init(); e.init()
        o.run(1); e.run(1)
        for nm in ("P", "E", "ZsumK"):
            assert np.array_equal(_bits(o.get(nm)), _bits(e.get(nm))), (nm, chain)
        P.append(e.get("P").copy())
        e.close()
    assert not (P[0] == P[1]).any()


@pytest.mark.parametrize("key", list(KEYS))
def test_chain_seed_is_the_engine_key(key, oracle_lib):
    """multichain.chain_seed names the key a chain draws with: the first uniform of a stream, drawn by the engine from (seed, chain id),
    is made of the first two words of the Philox block under chain_seed(seed, chain id)."""
    from bayesnmf_amd import engine as E
    from bayesnmf_amd.multichain import chain_seed
    seed, chain = KEYS[key]
    k = chain_seed(seed, chain)
    assert k == (seed & 0xFFFFFFFF, (seed >> 32) ^ chain) and all(0 <= w < 2 ** 32 for w in k)
    var, elem0, it = 3, 0x80000005, 0x90000000
    u = E.test_sampler("runif", n=5, seed=seed, chain=chain, var=var, elem0=elem0, it=it)
    for i in range(5):
        w = E.test_philox([0, elem0 + i, it, var], k)
        assert w == oracle_lib.philox([0, elem0 + i, it, var], k)
        assert u[i] == oracle_lib.lib().orc_t_u52(w[0], w[1])
