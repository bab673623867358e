"""ralpha_fast_wave (csrc/dsamplers.h), the wave-cooperative form of the Gamma-shape draw of k_draw's E-side hyper sweep, through the
probe `which = 7` of bnmf_test_sampler: bit for bit the oracle's ralpha_fast and the engine's scalar ralpha_fast, on inputs that are
proven — from the oracle's attempt counts alone, before the device is touched — to reach every round shape of the exchange: every
`per` from 64 down to 1, three and more rounds with a shrinking number of pending lanes, lanes that leave for the general sampler
after 64 rejections (mode 3) or at once (mode 2) beside pending lanes, and the idle lanes of a partial wave as helpers.

wave_schedule() restates the round schedule alone (who is pending, how many attempts each gets, where the first accepted one sits);
it holds no sampler arithmetic: what is accepted comes from the oracle's `attempts`."""
import functools

import numpy as np
import pytest

FAST_ATTEMPTS = 64
WAVE = 64
# recipe: (c, tau, xprev); what the oracle makes of them (6,400 draws each):
RECIPES = dict(easy=(100.0, 5.0, 10.0),            # 6.5 % need more than one attempt, at most 4
               middling=(95000.0, 0.3, 9000.0),    # 40 % need more than one, at most 10
               never=(3e5, 10.0, 5000.0),          # 64 fast rejections, then the general sampler
               general=(0.8, 2.0, 1.0),            # c <= 1: the general sampler from block 0
               broad=(1.3, 2.0, 1.0),              # rho >= 0.35 (values only: not part of the coverage counts)
               neg=(100.0, -30.0, 10.0))           # r <= 0     (values only)
WIDE_KEY = dict(seed=0x9E3779B97F4A7C15, chain=0x80000001)
VAR, IT = 7, 8


def wave_schedule(attempts, fast):
    """The rounds of ralpha_fast_wave for one wave.  attempts[i]: the oracle's attempt count of lane i (the k-th attempt is Philox
    block k - 1; above FAST_ATTEMPTS the lane left the fast path); fast[i]: the lane is on the fast path (mode 1).  Lanes beyond
    len(attempts) have no element.  Returns (rounds, mode3, wins): rounds = [(np, per, nk)], mode3 = the lanes that end in mode 3,
    wins = [(lane, round, offset in the owner's group, per)]."""
    attempts, fast = np.asarray(attempts), np.asarray(fast, dtype=bool)
    pend = fast & (attempts > 1)                          # attempt 0 is every fast lane's own
    rounds, wins, mode3 = [], [], np.zeros(attempts.size, dtype=bool)
    nk = 1
    while pend.any():
        n_pend = int(pend.sum())
        per = 1 << int(np.floor(np.log2(WAVE // n_pend)))
        rounds.append((n_pend, per, nk))
        for lane in np.flatnonzero(pend):
            blk = attempts[lane] - 1                      # the block the sequential loop stops at
            if nk <= blk < min(nk + per, FAST_ATTEMPTS):
                wins.append((int(lane), len(rounds) - 1, int(blk - nk), per))
                pend[lane] = False
        nk += per
        if nk >= FAST_ATTEMPTS:
            mode3 |= pend
            pend[:] = False
    return rounds, mode3, wins


def _bucket(n_pend):
    return next(b for b, hi in zip(("1", "2", "3-4", "5-8", "9-16", "17-32", "33-63", "64"), (1, 2, 4, 8, 16, 32, 63, 64)) if n_pend <= hi)


def _waves():
    """The kinds of the lanes, wave by wave."""
    rng = np.random.default_rng(20251017)
    mix = lambda *parts: rng.permutation(np.concatenate([np.repeat(k, n) for k, n in parts]))   # noqa: E731
    w = []
    w += [mix(("easy", 64)) for _ in range(60)]                                   # first rounds of 0 .. 8 pending lanes
    w += [mix(("easy", 8), ("general", 56)) for _ in range(6)]                    # ... of none
    w += [mix(("middling", 64)) for _ in range(50)]                               # 17-32 pending, several rounds, per grows
    w += [mix(("middling", 24), ("easy", 40)) for _ in range(10)]                 # 9-16
    w += [mix(("middling", 1), ("general", 63)) for _ in range(8)]                # one pending lane: per = 64
    w += [mix(("middling", 2), ("general", 30), ("easy", 32)) for _ in range(8)]
    for k in (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 40, 63):
        w += [mix(("never", k), ("general", 64 - k))]                             # exactly k pending lanes, all to mode 3
        w += [mix(("never", k), ("easy", 64 - k))]                                # at least k
        w += [mix(("never", k), ("middling", 64 - k))]                            # mode 3 beside lanes decided in round 1
    w += [mix(("never", 64))]                                                     # 63 rounds of per = 1
    w += [mix(("middling", 40), ("general", 24)) for _ in range(6)]               # mode 2 beside pending lanes
    w += [mix(("broad", 8), ("neg", 8), ("easy", 24), ("middling", 24)) for _ in range(8)]   # values only
    w += [mix(("never", 1), ("middling", 30), ("general", 6))]                    # the partial last wave: 37 lanes
    return w


@functools.lru_cache(maxsize=None)
def _inputs(wide):
    """c, tau, xprev of every element, the oracle's draws and attempt counts; asserts (oracle only) that the input reaches every case."""
    import oracle as O
    waves = _waves()
    kinds = np.concatenate(waves)
    c, tau, xp = (np.array([RECIPES[k][j] for k in kinds]) for j in range(3))
    key = WIDE_KEY if wide else {}
    want, att = O.ralpha(c, tau, xp, var=VAR, it=IT, fast=True, **key)
    n = kinds.size
    assert n % WAVE not in (0,) and len(waves) >= 150
    seen = dict(buckets=set(), np0=False, three_rounds=False, mode3_beside_round1=False, all_never=False, mode2_beside_pending=False,
                off0=False, off_last=False, partial=False, pers=set())
    for wv in range(len(waves)):
        kd, a = kinds[wv * WAVE:(wv + 1) * WAVE], att[wv * WAVE:(wv + 1) * WAVE]
        if np.isin(kd, ("broad", "neg")).any():
            continue                                      # which path those lanes take is the sampler's business: not counted
        fast = kd != "general"
        rounds, mode3, wins = wave_schedule(a, fast)
        assert np.array_equal(mode3, fast & (a > FAST_ATTEMPTS)) and (a[kd == "never"] > FAST_ATTEMPTS).all()
        seen["pers"] |= {r[1] for r in rounds}
        if not rounds:
            seen["np0"] = True
            continue
        seen["buckets"].add(_bucket(rounds[0][0]))
        seen["three_rounds"] |= len(rounds) >= 3 and len({r[1] for r in rounds}) >= 2 and rounds[-1][0] < rounds[0][0]
        seen["mode3_beside_round1"] |= bool(mode3.any()) and any(r == 0 for _, r, _, _ in wins)
        seen["all_never"] |= (kd == "never").all() and kd.size == WAVE and rounds == [(64, 1, k) for k in range(1, 64)]
        seen["mode2_beside_pending"] |= bool((~fast).any())
        seen["off0"] |= any(off == 0 and per >= 2 for _, _, off, per in wins)
        seen["off_last"] |= any(off == per - 1 and per >= 2 for _, _, off, per in wins)
        seen["partial"] |= kd.size < WAVE
    assert seen["buckets"] == {"1", "2", "3-4", "5-8", "9-16", "17-32", "33-63", "64"}, seen["buckets"]
    assert seen["pers"] == {64, 32, 16, 8, 4, 2, 1}, seen["pers"]
    for what in ("np0", "three_rounds", "mode3_beside_round1", "all_never", "mode2_beside_pending", "off0", "off_last", "partial"):
        assert seen[what], what
    for a in (c, tau, xp, want, att):
        a.setflags(write=False)
    return c, tau, xp, want, att


def _small(wide):
    """n < 64: one partial wave, with pending lanes, a mode 3 lane and a mode 2 lane."""
    import oracle as O
    kinds = np.array(["middling"] * 20 + ["never", "general", "easy", "never"] + ["middling"] * 13)
    c, tau, xp = (np.array([RECIPES[k][j] for k in kinds]) for j in range(3))
    want, att = O.ralpha(c, tau, xp, var=VAR, it=IT, elem0=1000003, fast=True, **(WIDE_KEY if wide else {}))
    rounds, mode3, wins = wave_schedule(att, kinds != "general")
    assert kinds.size < WAVE and len(rounds) >= 2 and mode3.sum() == 2 and wins
    return c, tau, xp, want


@pytest.mark.gpu
@pytest.mark.parametrize("wide", [False, True], ids=["key_1_0", "key_wide"])
def test_wave_alpha_draw_bitexact(wide):
    """About 200 waves of recipes: the wave form equals the oracle and the scalar form bit for bit, with the default key and with a key
    whose two words both have their top bit set."""
    c, tau, xp, want, _ = _inputs(wide)
    cs, ts, xs, want_s = _small(wide)                     # (every coverage assertion has passed before the first device call)
    from bayesnmf_amd import engine as E
    key = WIDE_KEY if wide else {}
    got = E.test_sampler("ralpha_fast_wave", c, tau, xp, var=VAR, it=IT, **key)
    bad = np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))
    assert bad.size == 0, f"{bad.size} of {c.size} differ from the oracle, first in wave {bad[0] >> 6} lane {bad[0] & 63}"
    scalar = E.test_sampler("ralpha_fast", c, tau, xp, var=VAR, it=IT, **key)
    assert np.array_equal(got.view(np.uint64), scalar.view(np.uint64))
    got = E.test_sampler("ralpha_fast_wave", cs, ts, xs, var=VAR, it=IT, elem0=1000003, **key)
    assert np.array_equal(got.view(np.uint64), want_s.view(np.uint64)), "n < 64"
    assert np.array_equal(got.view(np.uint64), E.test_sampler("ralpha_fast", cs, ts, xs, var=VAR, it=IT, elem0=1000003, **key).view(np.uint64))
