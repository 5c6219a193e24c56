"""Pins the wide plain-C oracle (oracle/env_oracle_wide.c: any odd 3 <= d <= 15, matching referee inside the step) against the Python
matching referee, the look-up referee, the golden traces from the reference and the Python environment.  CPU only.  This oracle is the
checker of the wide HIP environment at full batch (tests/test_env_wide_gpu.py)."""
import functools
import operator

import numpy as np
import pytest

from conftest import load_golden, TRACES, STICKY_TRACES, BIG_TRACES, trace_config
from oracle import c_oracle, env_oracle, lattice, matching_referee, philox, referee

COMPONENTS = ((0, 3), (1, 1))          # (C component index, plaquette type): 0 = X part, 1 = Z part


def _bits(defects):
    v = sum(1 << int(i) for i in defects)
    return [v & (2 ** 64 - 1), v >> 64]


@pytest.mark.parametrize("d", [3, 5, 7, 9, 11, 13, 15])
def test_wide_referee_tables_equal_python(d):
    """dist / distB / w10 of both components equal ComponentGraph's."""
    m = c_oracle.CWideMatch(d)
    for comp, typ in COMPONENTS:
        g = matching_referee.ComponentGraph(d, typ)
        dist, distB, w10 = m.tables(comp)
        assert np.array_equal(dist, g.dist) and np.array_equal(distB, g.distB) and w10 == g.w10, (d, comp)
        # no plaquette is equally far from the boundaries of both classes, so the fallbacks' tie rule (-> class 0) never decides
        assert (distB[:, 0] != distB[:, 1]).all(), (d, comp)


def _ball(g, center, k):
    """k nodes around `center` in breadth-first order over distance-1 neighbours: one cluster (adjacent defects are always worth matching)."""
    order, seen, i = [center], {center}, 0
    while len(order) < k:
        u = order[i]
        i += 1
        for v in range(g.n):
            if v not in seen and min(g.dist[u, v]) == 1:
                seen.add(v)
                order.append(v)
    return sorted(order[:k])


@pytest.mark.parametrize("d", [9, 11, 13, 15])
def test_wide_referee_equals_python_referee(d):
    """(w_0, w_1, exact) of the C referee == ComponentGraph.weights, both components: the empty syndrome, every single defect, random sets of
    2..12, 13..21, 32, 33 and 33..40 defects, and sets built to put more than MAX_DEFECTS defects into one cluster.  The C side's fallback flags
    must equal what the Python clustering says, and every path (exact, cluster fallback, list fallback) must be hit."""
    rng = np.random.default_rng(1000 + d)
    m = c_oracle.CWideMatch(d)
    hits = {"exact": 0, "cluster": 0, "list": 0}
    for comp, typ in COMPONENTS:
        g = matching_referee.ComponentGraph(d, typ)
        cases = [[]] + [[u] for u in range(g.n)]
        cases += [sorted(rng.choice(g.n, rng.integers(2, 13), replace=False)) for _ in range(60)]
        cases += [sorted(rng.choice(g.n, rng.integers(13, 22), replace=False)) for _ in range(6)]
        cases += [sorted(rng.choice(g.n, rng.integers(33, 41), replace=False))]
        cases += [sorted(rng.choice(g.n, k, replace=False)) for k in (32, 33)]          # the MAX_LIST edge: the flag tells them apart
        cases += [_ball(g, int(rng.integers(g.n)), int(rng.integers(21, 25)))]
        # fast batch path (classes) for all cases at once; per-case weights below
        cls, w, fl = m.classify_bits(comp, np.array([_bits(c) for c in cases], dtype=np.uint64))
        for k, D in enumerate(cases):
            w0, w1, exact = g.weights(D)
            assert (int(w[k, 0]), int(w[k, 1]), int(fl[k]) == 0) == (w0, w1, exact), (d, comp, D)
            assert int(cls[k]) == int(w1 < w0) == g.classify(sum(1 << int(i) for i in D))
            big_cluster = any(len(cl) > matching_referee.MAX_DEFECTS for cl in g.clusters(D[:matching_referee.MAX_LIST]))
            beyond = len(D) > matching_referee.MAX_LIST
            assert int(fl[k]) == (c_oracle.CWideMatch.CLUSTER_FALLBACK if big_cluster else 0) | (c_oracle.CWideMatch.LIST_FALLBACK if beyond else 0)
            hits["exact"] += exact
            hits["cluster"] += big_cluster
            hits["list"] += beyond
    assert hits["exact"] >= 100 and hits["cluster"] >= 2 and hits["list"] >= 2, hits


@pytest.mark.parametrize("d", [3, 5, 7])
def test_wide_referee_equals_the_lookup_referee(d):
    """At d = 3, 5 every syndrome of both components gets the look-up referee's class, exactly.  At d = 7 (2^24 syndromes per component) a
    random sample of 3000 per component does wherever the answer is exact; a cluster of more than MAX_DEFECTS = 20 of the 24 plaquettes is the
    fallback's (not minimum-weight) answer and must be flagged."""
    m = c_oracle.CWideMatch(d)
    n = (d * d - 1) // 2
    idx = np.arange(1 << n, dtype=np.uint64) if d < 7 else np.random.default_rng(7).integers(0, 1 << n, 3000).astype(np.uint64)
    bits = np.stack([idx, np.zeros_like(idx)], axis=1)
    for comp, typ in COMPONENTS:
        lut = c_oracle.build_lut(d, typ)
        if d < 7:
            assert np.array_equal(lut, referee.build_lut(d, typ))
        cls, _, fl = m.classify_bits(comp, bits)
        exact = fl == 0
        assert np.array_equal(cls[exact], lut[idx.astype(np.int64)][exact]), (d, comp)
        n_defects = np.array([bin(int(i)).count("1") for i in idx])
        assert np.array_equal(fl != 0, n_defects > matching_referee.MAX_DEFECTS) if d == 7 else exact.all()


def _big(words):
    return sum(int(w) << (64 * k) for k, w in enumerate(np.atleast_1d(words)))


def _replay(name, auto_reset):
    g = load_golden("trace_" + name)
    cfg, n_envs, n_steps, seed = trace_config(g)
    env = c_oracle.COracleWideEnv(n_envs=n_envs, seed=seed, **cfg)
    d, n_act = cfg["d"], env.num_actions
    m = lattice.Masks(d)

    def check(t):
        assert np.array_equal(env.obs, g["obs"][:, t]), (name, "obs", t)
        assert np.array_equal(env.done, g["done"][:, t]), (name, "done", t)
        assert np.array_equal(env.lifetime, g["lifetime"][:, t]), (name, "lifetime", t)
        for e, s in enumerate(env.export()):
            assert _big(env.legal[e]) == _big(g["legal"][e, t]) == s["legal"], (name, "legal", e, t)
            assert np.array_equal(env_oracle.masks_to_codes(d, s["xmask"], s["zmask"]), g["hidden"][e, t]), (name, "hidden", e, t)
            assert np.array_equal(m.word_to_grid(s["true_word"]), g["true_syndrome"][e, t]), (name, "true_syndrome", e, t)
            assert np.array_equal(m.word_to_grid(s["summed"]), g["summed_nonzero"][e, t]), (name, "summed", e, t)
            assert s["acted"] == _big(g["acted"][e, t]) and s["round"] == int(g["rounds"][e, t]), (name, "acted/round", e, t)
            assert [(s["completed"] >> a) & 1 for a in range(n_act)] == list(g["completed"][e, t]), (name, "completed", e, t)
            assert s["lifetime"] == g["lifetime"][e, t] and s["done"] == g["done"][e, t]
            assert s["summed"] == functools.reduce(operator.or_, s["volume"], 0)

    env.reset()
    check(0)
    events = dict(reward=0, done=0)
    for t in range(n_steps):
        env.step(g["action"][:, t], auto_reset=auto_reset)
        assert np.array_equal(env.reward, g["reward"][:, t]), (name, "reward", t)
        if auto_reset:
            assert np.array_equal(env.was_reset, g["was_reset"][:, t]), (name, "was_reset", t)
        else:
            assert not env.was_reset.any()
        events["reward"] += int(env.reward.sum())
        events["done"] += int(env.done.sum())
        check(t + 1)
    return events


@pytest.mark.parametrize("name", TRACES + BIG_TRACES)
def test_wide_c_oracle_replays_golden_traces(name):
    ev = _replay(name, True)
    assert ev["done"] > 0 or name.startswith("x3"), ev


@pytest.mark.parametrize("name", STICKY_TRACES)
def test_wide_c_oracle_replays_sticky_traces(name):
    _replay(name, False)


class _PyRef:
    """MatchingReferee that also records whether a fallback was used by its last answer."""

    def __init__(self, d, error_model):
        self.r = matching_referee.MatchingReferee(d, error_model)
        self.inexact = False

    def classify_word(self, word):
        r = self.r
        _, _, ex = r.gx.weights([i for i in range(r.gx.n) if (r.masks.referee_index(word, 3) >> i) & 1])
        if r.error_model != "X":
            _, _, ez = r.gz.weights([i for i in range(r.gz.n) if (r.masks.referee_index(word, 1) >> i) & 1])
            ex = ex and ez
        self.inexact = not ex
        return r.classify_word(word)


@pytest.mark.parametrize("cfg,n_envs,steps", [
    (dict(d=9, error_model="DP", use_Y=False, volume_depth=9, p_phys=0.01, p_meas=0.01), 3, 30),
    (dict(d=9, error_model="IIDXZ", use_Y=False, volume_depth=16, p_phys=0.004, p_meas=0.004), 2, 20),
    (dict(d=11, error_model="DP", use_Y=True, volume_depth=4, p_phys=0.006, p_meas=0.006), 3, 25),
    (dict(d=13, error_model="X", use_Y=False, volume_depth=5, p_phys=0.002, p_meas=0.02), 3, 30),
    (dict(d=15, error_model="DP", use_Y=True, volume_depth=3, p_phys=0.004, p_meas=0.004), 2, 20),
    (dict(d=15, error_model="X", use_Y=False, volume_depth=2, p_phys=0.06, p_meas=0.06), 2, 6),
], ids=["d9dp", "d9iidxz-deep", "d11dpy", "d13x-meas", "d15dpy", "d15x-hot"])
def test_wide_c_vs_python_oracle_random_walk(cfg, n_envs, steps):
    """Free-running cross-check of the wide C oracle and OracleEnv + MatchingReferee under the uniform-over-legal policy: action choice,
    reward, done, lifetime, observation, legal set, inexact flag and the whole hidden state, at every step."""
    seed, base = (11, 13), 2 ** 31 - 2
    ce = c_oracle.COracleWideEnv(n_envs=n_envs, seed=seed, env_id_base=base, **cfg)
    refs = [_PyRef(cfg["d"], cfg["error_model"]) for _ in range(n_envs)]
    pes = [env_oracle.OracleEnv(referee=refs[e], seed=seed, env_id=(base + e) & 0xFFFFFFFF, **cfg) for e in range(n_envs)]
    ce.reset()
    for p in pes:
        p.reset()
    n_inexact = 0
    for t in range(steps):
        a = ce.policy_uniform_legal(t)
        for e, p in enumerate(pes):
            assert _big(ce.legal[e]) == p.legal
            legal = sorted(p.legal_actions)
            w = philox.site_words(seed, (base + e) & 0xFFFFFFFF, t, 0, stream=philox.STREAM_POLICY)
            assert a[e] == legal[philox.bounded(w[0], len(legal))]
        ce.step(a, auto_reset=True)
        for e, p in enumerate(pes):
            refs[e].inexact = False
            if p.done:
                p.reset()
                r = 0.0
            else:
                _, r, _, _ = p.step(int(a[e]))
            assert r == ce.reward[e] and p.done == bool(ce.done[e]) and p.lifetime == ce.lifetime[e], (t, e)
            assert refs[e].inexact == bool(ce.inexact[e]), (t, e)
            n_inexact += refs[e].inexact
            assert np.array_equal(p.board_state, ce.obs[e]), (t, e)
        for p, s in zip(pes, ce.export()):
            assert (s["xmask"], s["zmask"], s["acted"], s["round"], s["completed"]) == (p.xmask, p.zmask, p.acted, p.round, p.completed)
            assert s["volume"] == p.volume
    if cfg["p_phys"] > 0.05:
        assert n_inexact > 0


def test_wide_c_oracle_rejects_bad_configurations():
    for kw in (dict(d=17), dict(d=10), dict(d=1), dict(d=9, volume_depth=17), dict(d=9, volume_depth=0)):
        with pytest.raises(ValueError):
            c_oracle.COracleWideEnv(n_envs=2, **kw)
