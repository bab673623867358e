"""Subtypes of tumours over a recorded range, the parts that need no GPU: properties of the numpy restatement of the spec
(tests/subtypes_ref.py), a planted cohort of three subtypes, the farthest-first seed helper, the library's own finish
(csrc/reduce_host.h) as a stand-alone program under the sanitizers, bayesNMF_sampler.get_subtypes over a stub engine, the two new
symbols and the refusals that need no device.

What moves exactly with the tumours.  A tumour's share profile, its distances and hence its label in a step involve its own values and
the centres only; the centres are sums over the positions of the member list (canonB), so their bits depend on the order of the members.
With n_steps = 1 the centres of the assignment are the given start: labels, membership, label, the tumour rows, together, the sizes and
the numbers of assigned tumours are whole numbers or ratios of whole numbers and move with the tumours bit for bit; the centres after the
step and the inertia are sums of m terms in another order and agree within gamma_m = m u / (1 - m u) relative to the sum of the
absolute values (shares in [0, 1]: at most n_c per coordinate before the division, hence gamma_m after it)."""
import os
import re
import subprocess

import numpy as np
import pytest

import subtypes_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53


def gamma(n):
    return n * U / (1.0 - n * U)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(x, y):
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    return x.shape == y.shape and np.array_equal(np.isnan(x), np.isnan(y)) and np.array_equal(_bits(x)[~np.isnan(x)], _bits(y)[~np.isnan(y)])


def _samples(S, K, G, N, seed, excluded=True):
    rng = np.random.default_rng(seed)
    P = rng.gamma(0.7, 1.0, size=(S, K, N))
    E = rng.gamma(0.5, 20.0, size=(S, N, G))
    A = np.ones((S, N))
    if excluded and N > 2:
        A[1, N - 1] = 0.0                                    # a sample that excludes a factor
    return P, E, A


def _start(P, E, A, seeds):
    q, _ = R.profiles(R.loads(P, E, A)[0])
    return np.asfortranarray(q[:, seeds])


def test_include_is_the_cohort_without_the_tumours():
    S, K, G, N = 5, 6, 1100, 3                                                               # two blocks of positions before, one and a rest after
    P, E, A = _samples(S, K, G, N, 21)
    inc = np.ones(G, dtype=np.int32)
    inc[[0, 17, 1023, 1024, G - 1] + list(range(40, 120))] = 0
    keep = np.where(inc == 1)[0]
    c0 = _start(P, E, A, [1, 500, 1090])
    a = R.subtypes_reference(P, E, A, c0, include=inc, query=[1, 1098])
    b = R.subtypes_reference(P, E[:, :, keep], A, c0, query=[0, len(keep) - 1])
    for k in ("membership", "tumour", "together"):
        assert _same_bits(a[k][:, keep], b[k]) and np.isnan(a[k][:, inc == 0]).all(), k
    assert np.array_equal(a["label"][keep], b["label"]) and (a["label"][inc == 0] == -1).all()
    assert np.array_equal(a["labels"][:, keep], b["labels"]) and (a["labels"][:, inc == 0] == -2).all()
    for k in ("centre", "size", "series", "mean_certainty", "least_certain", "smallest_subtype"):
        assert _same_bits(a[k], b[k]), k
    for k in ("n_certain", "n_never_assigned", "n_not_converged", "n_included", "smallest_subtype_at"):
        assert a[k] == b[k], k
    assert a["least_certain_at"] == keep[b["least_certain_at"]] and a["n_left_out"] == 85 and b["n_left_out"] == 0


def test_a_zero_total_tumour_is_unassigned_and_changes_nobody_elses_bits():
    """the tumour is the last member, so that leaving it out moves nobody's position in the member list: its +0.0 terms leave every
    accumulator's bits alone and it enters no count, so everything about the others is what the cohort without it gives"""
    S, K, G, N = 4, 6, 70, 3
    P, E, A = _samples(S, K, G, N, 2, excluded=False)
    c0 = _start(P, E, A, [3, 30, 60])
    E0 = E.copy()
    E0[2, :, G - 1] = 0.0                                                                   # no exposure in sample 2 only
    r = R.subtypes_reference(P, E0, A, c0, query=[0, G - 1])
    assert r["labels"][2, G - 1] == -1 and (r["labels"][[0, 1, 3], G - 1] >= 0).all() and r["series"][2, 2] == G - 1
    assert r["tumour"][1, G - 1] == 0.75 and (r["tumour"][1, :G - 1] == 1.0).all() and r["n_never_assigned"] == 0
    Ez = E.copy()
    Ez[:, :, G - 1] = 0.0                                                                   # no exposure anywhere: never assigned
    z = R.subtypes_reference(P, Ez, A, c0, query=[0, G - 1])
    inc = np.ones(G, dtype=np.int32)
    inc[G - 1] = 0
    w = R.subtypes_reference(P, E, A, c0, include=inc, query=[0])
    assert (z["labels"][:, G - 1] == -1).all() and z["label"][G - 1] == -1 and z["n_never_assigned"] == 1 and z["tumour"][1, G - 1] == 0.0
    assert np.isnan(z["membership"][:, G - 1]).all() and np.isnan(z["tumour"][[0, 2], G - 1]).all() and np.isnan(z["together"][:, G - 1]).all()
    assert np.isnan(z["together"][1]).all()                                                 # the row of a tumour that is never assigned
    for k in ("membership", "tumour", "labels"):
        assert _same_bits(z[k][:, :G - 1], w[k][:, :G - 1]), k
    assert _same_bits(z["together"][0, :G - 1], w["together"][0, :G - 1])
    for k in ("centre", "size", "mean_certainty", "least_certain"):
        assert _same_bits(z[k], w[k]), k
    assert _same_bits(z["series"][:2], w["series"][:2]) and (z["series"][2] == G - 1).all()


def test_nan_tie_and_empty_cluster_conventions():
    S, K, G, N = 4, 6, 40, 4
    P, E, A = _samples(S, K, G, N, 5, excluded=False)
    c0 = _start(P, E, A, [3, 11, 20])
    # a NaN or infinite load: the total is not in (0, inf), the tumour is unassigned in that sample
    En = E.copy()
    En[1, 0, 7] = np.nan
    En[3, 2, 9] = np.inf
    r = R.subtypes_reference(P, En, A, c0)
    assert r["labels"][1, 7] == -1 and r["labels"][3, 9] == -1 and not np.isnan(r["centre"]).any() and not np.isnan(r["series"]).any()
    assert r["tumour"][1, 7] == 0.75 and r["tumour"][1, 9] == 0.75
    # a sample that excludes every factor: everybody unassigned, one step, the start is kept, no inertia
    A0 = A.copy()
    A0[2] = 0.0
    r = R.subtypes_reference(P, E, A0, c0)
    assert (r["labels"][2] == -1).all() and r["series"][:, 2].tolist() == [0.0, 1.0, 0.0]
    assert _same_bits(r["sample_centres"][2], c0) and (r["sample_sizes"][2] == 0).all()
    # two equal columns: the lower label wins every tie; the empty cluster keeps its centre
    dup = np.asfortranarray(c0[:, [0, 1, 1]])
    r = R.subtypes_reference(P, E, A, dup, n_steps=1)
    assert (r["labels"] != 2).all() and (r["sample_sizes"][:, 2] == 0).all() and (r["sample_centres"][:, :, 2] == dup[:, 2]).all()
    assert (r["membership"][2] == 0.0).all() and r["smallest_subtype_at"] == 2 and r["smallest_subtype"] == 0.0
    # a NaN distance never wins: a tumour's first distance stays (the refusals keep NaN out of the start; the helper itself is total)
    q, ok = R.profiles(R.loads(P, E, A)[0])
    mu = c0.copy()
    mu[0, 1] = np.nan
    lab, dmin = R.assign(q, ok, mu)
    assert (lab != 1).all()
    mu = c0.copy()
    mu[0, 0] = np.nan
    lab, dmin = R.assign(q, ok, mu)
    assert (lab == 0).all() and np.isnan(dmin).all()
    # the count of the equal largest memberships: the lowest c is the label
    labs = np.array([[0], [1], [1], [0], [2]])
    f = R.finish(np.array([0]), 1, labs, np.zeros((5, 2, 3)), np.ones((5, 3), dtype=np.int64), np.zeros(0, dtype=np.int64), 0.5)
    assert f["label"][0] == 0 and f["tumour"][:, 0].tolist() == [0.4, 1.0, 0.4] and f["n_certain"] == 0
    # the refusals of the restatement
    for kw, code in ((dict(n_steps=0), -1), (dict(query=[G]), -1), (dict(min_certainty=1.5), -1), (dict(perm=np.zeros((S, N), dtype=int)), -1),
                     (dict(perm=np.full((S, N), -1)), -2), (dict(include=np.r_[1, 1, np.zeros(G - 2, dtype=int)]), -2)):
        with pytest.raises(R.Refused) as ei:
            R.subtypes_reference(P, E, A, c0, **kw)
        assert ei.value.code == code, kw


def test_permuting_the_tumours_inside_a_block():
    S, K, G, N = 5, 6, 300, 4
    P, E, A = _samples(S, K, G, N, 8)
    perm = np.random.default_rng(1).permutation(G)
    c0 = _start(P, E, A, [3, 100, 250])
    a = R.subtypes_reference(P, E, A, c0, n_steps=1, query=[int(perm[4])])
    b = R.subtypes_reference(P, E[:, :, perm], A, c0, n_steps=1, query=[4])
    assert np.array_equal(b["labels"], a["labels"][:, perm]) and np.array_equal(b["label"], a["label"][perm])
    for k in ("membership", "tumour", "together"):
        assert _same_bits(b[k], a[k][:, perm]), k
    assert _same_bits(b["size"], a["size"]) and _same_bits(b["series"][1:], a["series"][1:])
    for k in ("n_certain", "mean_certainty", "least_certain", "smallest_subtype", "smallest_subtype_at"):
        assert a[k] == b[k] or k == "mean_certainty", k                                        # (the mean certainty is a sum in member order)
    assert abs(a["mean_certainty"] - b["mean_certainty"]) <= gamma(G)
    assert np.abs(b["sample_centres"] - a["sample_centres"]).max() <= gamma(G)                 # the centres and the inertia: sums in another order
    assert (np.abs(b["series"][0] - a["series"][0]) <= gamma(G) * a["series"][0]).all()
    assert not _same_bits(b["sample_centres"], a["sample_centres"])                            # (the order of the sums did change)


def _planted():
    """45 tumours in three subtypes with signatures 0 - 1, 2 - 3 and 4 - 5 only, in shares near 0.7 : 0.3, at tumour burdens that vary
    widely; 10 samples: the true exposures under lognormal jitter.  Two profiles of one subtype differ by the jitter only (squared
    distance of the order 0.01), two of different subtypes have disjoint supports (squared distance above 1)."""
    rng = np.random.default_rng(20261020)
    S, K, G, N = 10, 10, 45, 6
    E0 = np.zeros((N, G))
    for c in range(3):
        E0[2 * c:2 * c + 2, 15 * c:15 * c + 15] = np.array([[70.0], [30.0]]) * rng.gamma(2.0, 1.0, size=(1, 15))
    E = E0[None] * rng.lognormal(0.0, 0.1, size=(S, N, G))
    P = rng.gamma(0.7, 1.0, size=(S, K, N))
    return P, E, np.ones((S, N))


def test_planted_subtypes():
    """the cohort was chosen (see _planted) so that the restatement alone, from farthest-first seeds, assigns every tumour to its planted
    subtype in every sample; this asserts exactly that: certainty 1.0 everywhere"""
    from bayesnmf_amd.sampler import subtype_seeds
    P, E, A = _planted()
    x = R.loads(P, E, A)
    prof = np.mean([R.profiles(x[s])[0] for s in range(len(x))], axis=0)
    seeds = subtype_seeds(prof, 3)
    truth = np.repeat(np.arange(3), 15)
    assert sorted(truth[seeds].tolist()) == [0, 1, 2]                                         # one seed in every subtype
    r = R.subtypes_reference(P, E, A, prof[:, seeds], query=[0, 20])
    want = np.argsort(truth[seeds])[truth]                                                    # subtype c is the one its seed was taken from
    print("seeds", seeds, "steps", r["series"][1], "sizes", r["size"][0], "certainty", r["tumour"][0].min())
    assert np.array_equal(r["label"], want) and (r["labels"] == want[None]).all()
    assert (r["tumour"][0] == 1.0).all() and (r["tumour"][2] == 0.0).all() and r["n_certain"] == 45 and r["mean_certainty"] == 1.0
    assert (r["size"][0] == 15.0).all() and (r["size"][1] == 0.0).all() and r["n_not_converged"] == 0
    assert (r["together"][0, 1:15] == 1.0).all() and (r["together"][0, 15:] == 0.0).all() and (r["together"][1, 15:30][np.arange(15, 30) != 20] == 1.0).all()


def test_farthest_first_seeds():
    from bayesnmf_amd.sampler import subtype_seeds
    # points on a line: the mean is 3.6, the nearest member is 4 (tumour 3); the farthest from it is 10 (tumour 4), then 0 (tumour 0)
    prof = np.array([[0.0, 1.0, 3.0, 4.0, 10.0]])
    assert subtype_seeds(prof, 3).tolist() == [3, 4, 0] and subtype_seeds(prof, 1).tolist() == [3]
    # ties go to the lower tumour: 0 and 4 are equally near the mean 2, 0 and 4 equally far from 2
    prof = np.array([[0.0, 4.0, 0.0, 4.0]])
    assert subtype_seeds(prof, 2).tolist() == [0, 1]
    # member: tumours that may not be chosen neither enter the mean nor the walk
    prof = np.array([[0.0, 1.0, 3.0, 4.0, 100.0]])
    assert subtype_seeds(prof, 2, member=[1, 1, 1, 1, 0]).tolist() == [1, 3]                   # mean 2: 1 and 3 are equally near, 1 is lower; 4 is farthest
    with pytest.raises(ValueError, match="cannot be chosen"):
        subtype_seeds(prof, 5, member=[1, 1, 1, 1, 0])


def test_finish_under_the_sanitizers_is_the_restatement(tmp_path):
    """csrc/reduce_host.h's subtypes_finish (the library's own code), built as a stand-alone program with -fsanitize=address,undefined: a
    clean run, and the outputs by tumour and the info fields the restatement's bit for bit; edge cases: tumours left out at both ends,
    a tumour that is never assigned, one that is unassigned in one sample, no query, C = 2 with m = 2, more than 64 members"""
    exe = str(tmp_path / "subtypes_reduce_check")
    cmd = ["c++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-pthread", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tools", "subtypes_reduce_check.cpp")]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr == "", p.stderr
    P, E, A = _samples(4, 6, 70, 3, 9)
    inc = np.ones(70, dtype=np.int32)
    inc[[0, 33, 69]] = 0
    Ez = E.copy()
    Ez[:, :, 5] = 0.0
    Ez[1, :, 8] = 0.0
    cases = [dict(E=E, include=inc, query=[1, 68, 1], C=3), dict(E=Ez, query=[5, 8, 2], C=4), dict(E=E, C=5), dict(E=E[:, :, :2], C=2, query=[0, 1])]
    for kw in cases:
        G, Cn = kw["E"].shape[2], kw["C"]
        c0 = _start(P, E, A, list(range(Cn)))
        ref = R.subtypes_reference(P, kw["E"], A, c0, include=kw.get("include"), query=kw.get("query"), min_certainty=0.8)
        members = np.asarray(ref["members"], dtype=np.int32)
        m, Sm, q = len(members), ref["n_matched"], np.asarray(kw.get("query", []), dtype=np.int32)
        blob = np.array([m, G, 3, Cn, Sm, len(q)], dtype=np.int64).tobytes() + np.array([0.8]).tobytes() + members.tobytes() + q.tobytes()
        blob += np.ascontiguousarray(ref["labels"][:, members], dtype=np.int32).tobytes() + np.ascontiguousarray(ref["sample_sizes"], dtype=np.int32).tobytes()
        blob += np.ascontiguousarray(ref["sample_centres"].transpose(0, 2, 1)).tobytes()                      # [Sm][C][N]: j + N c
        src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        with open(src, "wb") as f:
            f.write(blob)
        run = subprocess.run([exe, src, dst], capture_output=True, text=True)
        assert run.returncode == 0 and run.stderr == "", run.stderr
        out = np.fromfile(dst, dtype=np.float64)
        mem, lab, tu, ce, sz, tg, info = np.split(out, np.cumsum([Cn * G, G, 3 * G, 4 * 3 * Cn, 4 * Cn, len(q) * G]))
        assert _same_bits(mem.reshape(Cn, G), ref["membership"]) and np.array_equal(lab, ref["label"]) and _same_bits(tu.reshape(3, G), ref["tumour"])
        assert _same_bits(ce.reshape(4, Cn, 3).transpose(0, 2, 1), ref["centre"]) and _same_bits(sz.reshape(4, Cn), ref["size"])
        assert _same_bits(tg.reshape(len(q), G), ref["together"])
        assert [int(v) for v in info[[0, 1, 2, 3, 6, 8]]] == [ref[n] for n in ("n_included", "n_left_out", "n_certain", "n_never_assigned", "least_certain_at",
                                                                                "smallest_subtype_at")]
        assert _same_bits(info[[4, 5, 7]], np.array([ref["mean_certainty"], ref["least_certain"], ref["smallest_subtype"]]))


def test_get_subtypes_ranges_idx_names_and_frames(tmp_path):
    """bayesNMF_sampler.get_subtypes over a stub engine: the range and idx rules of get_WAIC (_recorded_range), the three ways to give the
    start, relabel's perm scattered into the range's rows, include and query as the sampler passes them on, the frames with the data's
    column names"""
    pd = pytest.importorskip("pandas")
    from test_waic_host import _NoWaicEngine
    from bayesnmf_amd.sampler import bayesNMF_sampler, subtype_seeds
    from bayesnmf_amd.convergence import new_convergence_control
    from bayesnmf_amd.setup import synth_counts

    class _SubEngine(_NoWaicEngine):
        calls = []

        def window(self, name, back):
            rng = np.random.default_rng(7)
            shp = dict(P=(self.K, self.N), E=(self.N, self.G), A=(1, self.N))[name]
            return [rng.gamma(1.0, 1.0, size=shp) if name != "A" else np.ones(shp) for _ in range(back)]

        def _relabel(self, last_n, used=None, end_iter=None, pivot_P=None, max_rounds=10, aligned=False):
            S = last_n if used is None else int(np.sum(used))
            perm = np.tile(np.arange(self.N, dtype=np.int32)[::-1], (S, 1))
            perm[1] = -1                                                                     # the second used sample is unmatched
            return dict(perm=perm, P_mean=np.ones((self.K, self.N)), E_mean=np.ones((self.N, self.G)))

        def subtypes(self, last_n, centres0, include=None, perm=None, n_steps=50, query=None, min_certainty=0.9, used=None, end_iter=None, labels=False):
            type(self).calls.append(dict(last_n=last_n, centres0=np.array(centres0), include=include, perm=perm, n_steps=n_steps, query=query,
                                         min_certainty=min_certainty, used=None if used is None else np.array(used), end_iter=end_iter, labels=labels))
            S, G, N, Cn = last_n if used is None else int(np.sum(used)), self.G, self.N, np.shape(centres0)[1]
            out = dict(n_used=S, n_matched=S - 1, n_unmatched=1, n_included=G, n_left_out=0, C=Cn, n_steps=n_steps, n_query=0 if query is None else len(query),
                       n_not_converged=0, n_certain=3, n_never_assigned=0, smallest_subtype_at=1, least_certain_at=2, mean_certainty=0.75, least_certain=0.5,
                       smallest_subtype=2.0, min_certainty=min_certainty, membership=np.full((Cn, G), 1.0 / Cn), label=np.arange(G, dtype=np.int32) % Cn,
                       tumour=np.arange(3.0 * G).reshape(3, G), centre=np.full((4, N, Cn), 4.0), size=np.full((4, Cn), 9.0), series=np.zeros((3, S)))
            if query is not None:
                out.update(together=np.full((len(query), G), 0.25), query=np.asarray(query))
            return out

    M, _, _ = synth_counts(12, 9, 2, 3, mean_total=200)
    names = [f"PD{g:03d}" for g in range(9)]
    cc = new_convergence_control()
    cc.update(MAP_over=4, MAP_every=2, maxiters=10, miniters=2)
    s = bayesNMF_sampler(pd.DataFrame(M, columns=names), 3, likelihood="poisson", prior="gamma", output_dir=str(tmp_path / "r"), engine_factory=_SubEngine,
                         convergence_control=cc, save_all_samples=True, periodic_save=False)
    s.run_gibbs_sampler()
    _SubEngine.relabel = _SubEngine._relabel                                                 # (only now: the run's own relabelling line needs more of it)
    r = s.get_subtypes(n_subtypes=2)
    c = _SubEngine.calls[-1]
    assert c["last_n"] == 4 and c["end_iter"] is None and c["n_steps"] == 50 and c["min_certainty"] == 0.9 and c["include"] is None and c["query"] is None
    assert np.array_equal(c["used"], [1, 1, 1, 1]) and c["perm"].shape == (4, 3) and (c["perm"][1] == -1).all() and c["perm"][0].tolist() == [2, 1, 0]
    assert c["centres0"].shape == (3, 2) and np.allclose(c["centres0"].sum(axis=0), 1.0) and len(r["seeds"]) == 2 and set(r["seeds"]) <= set(names)
    prof = s._mean_share_profiles(4, c["used"], c["perm"], {})
    assert np.array_equal(c["centres0"], prof[:, subtype_seeds(prof, 2)])
    t = r["tumours"]
    assert list(t.columns) == ["tumour", "label", "certainty", "runner_up", "assigned", "included", "membership_0", "membership_1"] and t["tumour"].tolist() == names
    assert np.array_equal(t["certainty"], r["tumour"][0]) and np.array_equal(t["runner_up"], r["tumour"][2]) and t["included"].all()
    assert list(r["subtypes"].columns) == ["subtype", "size", "size_sd", "size_lower", "size_upper"] and r["subtypes"].iloc[1].tolist() == [1, 9.0, 3.0, 9.0, 9.0]
    assert list(r["centres"].columns) == ["subtype", "factor", "mean", "sd", "lower", "upper"] and len(r["centres"]) == 6
    assert r["centres"].iloc[0].tolist() == [0, 0, 4.0, 2.0, 4.0, 4.0] and "consensus" not in r
    assert [r[k] for k in ("n_used", "n_matched", "n_unmatched", "C", "n_certain", "least_certain_at")] == [4, 3, 1, 2, 3, 2]
    inc = [1, 1, None, 1, 0, 1, float("nan"), 1, 1]
    r = s.get_subtypes(seeds=["PD003", "PD000", "PD008"], include=inc, query=["PD003", "PD000"], relabel=False, n_steps=7, min_certainty=0.8, end_iter=8,
                       n_samples=5, idx=[4, 6, 8], labels=True)
    c = _SubEngine.calls[-1]
    assert c["end_iter"] == 8 and c["last_n"] == 5 and np.array_equal(c["used"], [1, 0, 1, 0, 1]) and c["min_certainty"] == 0.8 and c["n_steps"] == 7
    assert c["perm"] is None and c["labels"] is True and c["centres0"].shape == (3, 3)
    assert np.array_equal(c["include"], [1, 1, 0, 1, 0, 1, 0, 1, 1]) and np.array_equal(c["query"], [3, 0]) and r["seeds"] == ["PD003", "PD000", "PD008"]
    assert list(r["consensus"].columns) == ["query", "tumour", "together"] and len(r["consensus"]) == 18 and r["consensus"].iloc[9].tolist() == ["PD000", "PD000", 0.25]
    assert r["tumours"]["included"].tolist() == [bool(v) for v in c["include"]] and r["query"] == ["PD003", "PD000"]
    start = np.array([[0.5, 0.1], [0.25, 0.2], [0.25, 0.7]])
    s.get_subtypes(centres=start, end_iter=8, n_samples=5, idx=None, relabel=False)
    assert _SubEngine.calls[-1]["used"] is None and np.array_equal(_SubEngine.calls[-1]["centres0"], start)
    with pytest.raises(ValueError, match="one of n_subtypes, centres and seeds"):
        s.get_subtypes()
    with pytest.raises(ValueError, match="names no tumour"):
        s.get_subtypes(seeds=["nobody", "PD001"])
    with pytest.raises(ValueError, match="a seed is a tumour that include leaves out"):
        s.get_subtypes(seeds=[2, 3], include=inc)
    with pytest.raises(ValueError, match="centres is"):
        s.get_subtypes(centres=np.ones((2, 2)))
    with pytest.raises(ValueError, match="n_subtypes = 3, but the start has 2"):
        s.get_subtypes(n_subtypes=3, centres=start)
    with pytest.raises(ValueError, match="include has 3 values"):
        s.get_subtypes(n_subtypes=2, include=[1, 1, 1])
    with pytest.raises(ValueError, match="not all recorded"):
        s.get_subtypes(n_subtypes=2, end_iter=12, n_samples=3)
    with pytest.raises(ValueError, match="Parameter `idx` must be"):
        s.get_subtypes(n_subtypes=2, idx="all")
    s.close()
    t = bayesNMF_sampler(M, 3, likelihood="poisson", prior="gamma", output_dir=str(tmp_path / "one"), engine_factory=_NoWaicEngine)
    with pytest.raises(ValueError, match="get_subtypes needs an engine"):
        t.get_subtypes(n_subtypes=2)
    t.close()


def test_new_symbols_declared_exported_bound_and_refused_without_a_device():
    import ctypes as C
    from bayesnmf_amd import engine
    hdr = open(os.path.join(ROOT, "include", "bnmf.h")).read()
    for name, val in (("BNMF_SUB_NTUM", 3), ("BNMF_SUB_NCROW", 4), ("BNMF_SUB_NSER", 3), ("BNMF_SUB_MAX_C", 32), ("BNMF_SUB_MAX_N", 128), ("BNMF_SUB_MAX_STEPS", 1000)):
        assert re.search(r"#define %s\s+%d\b" % (name, val), hdr), name
    assert re.search(r"#define BNMF_VERSION 100\b", hdr) and "The credible interval is fixed at 0.95" in hdr
    for sym in ("bnmf_subtypes", "bnmf_subtypes_at"):
        assert re.search(r"\bint\s+%s\s*\(\s*bnmf_handle\s*\*" % sym, hdr), f"{sym} not declared in include/bnmf.h"
        assert sym in engine.ABI_SYMBOLS
    so = os.path.join(ROOT, "bayesnmf_amd", "libbnmf.so")
    if not os.path.exists(so):
        import __graft_entry__ as g
        g.build()
    exported = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    L = engine.lib()
    for sym, nargs in (("bnmf_subtypes", 20), ("bnmf_subtypes_at", 21)):
        assert re.search(r"\bT %s$" % sym, exported, re.M), f"{sym} not exported by libbnmf.so"
        assert len(getattr(L, sym).argtypes) == nargs
    assert C.sizeof(engine.BnmfSubtypesInfo) == 88 and R.MAX_C == 32 and R.MAX_N == 128 and R.MAX_STEPS == 1000
    assert engine.SUB_TUMOUR_ROWS == ("certainty", "assigned", "runner_up") and engine.SUB_ROWS == ("mean", "var", "lower", "upper")
    assert engine.SUB_SERIES_ROWS == ("inertia", "steps", "n_assigned")
    assert hasattr(engine.Engine, "subtypes") and hasattr(engine.Engine, "subtypes_at")
    shim = open(os.path.join(ROOT, "r", "bnmf_shim.c")).read()
    for sym in ("C_bnmf_subtypes", "C_bnmf_subtypes_at"):
        assert re.search(r'\{"%s", \(DL_FUNC\)&%s, 9\}' % (sym, sym), shim), sym
    # what is refused before the handle is looked at needs no device: a null handle, a null info
    info = engine.BnmfSubtypesInfo()
    c0 = np.asfortranarray(np.ones((3, 2)))
    rest = (None, None, None, c0.ctypes.data_as(C.POINTER(C.c_double)), 2, 5, None, 0, 0.9, None, None, None, None, None, None, None, None)
    assert L.bnmf_subtypes(None, 4, *rest, C.byref(info)) == -1 and b"null" in L.bnmf_last_error()
    assert L.bnmf_subtypes_at(None, 9, 4, *rest, None) == -1 and b"bnmf_subtypes_at" in L.bnmf_last_error()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "## 25." in design and "bnmf_subtypes" in design
