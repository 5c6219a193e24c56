"""The union-find decoder as a policy and a teacher of the wide environment, host side (VectorEnv.uf_select_wide / guided_select_wide,
decoder_wide.WideUnionFindAgent, guided_actions_wide, completed_from_state, DQNCore.guided_act_and_step_wide): the rule replayed on
the C oracle environment with the event minimums of every configuration, the numpy statements against decoder.guided_actions and the oracle's
select_action, argument validation before any library call, the agent's plumbing on stub environments, and the C ABI.

replay(name) is also the reference of tests/test_wide_env_uf_gpu.py: it is computed once per configuration and never modified."""
import ctypes
import functools
import importlib
import os
import types

import numpy as np
import pytest

import wide_uf_ref as W

SEED = (0x5EED, 0xD0DEC0DE)

# name: (lattice, lattices, steps); env_id_base 0, p_meas = p_phys
CONFIGS = {
    "d9dp": (dict(d=9, error_model="DP", use_Y=False, volume_depth=9, p_phys=0.008), 64, 24),
    "d9hot": (dict(d=9, error_model="DP", use_Y=False, volume_depth=4, p_phys=0.03), 64, 24),
    "d11x": (dict(d=11, error_model="X", use_Y=False, volume_depth=5, p_phys=0.02), 48, 24),
    "d13iid": (dict(d=13, error_model="IIDXZ", use_Y=False, volume_depth=4, p_phys=0.015), 32, 24),
    "d15dpy": (dict(d=15, error_model="DP", use_Y=True, volume_depth=3, p_phys=0.02), 32, 24),
    "d15deep": (dict(d=15, error_model="DP", use_Y=False, volume_depth=16, p_phys=0.01), 8, 12),
    "d5wide": (dict(d=5, error_model="DP", use_Y=False, volume_depth=5, p_phys=0.011), 64, 40),
}
# conditions on the events of a run, beyond those every configuration has: done-lattice visits, reward = 1
MIN_DONE = {"d9hot": 20, "d11x": 15, "d15deep": 10}
MIN_REWARD = {"d9dp": 100, "d5wide": 100}


def env_kwargs(name):
    cfg, n, steps = CONFIGS[name]
    return dict(cfg, p_meas=cfg["p_phys"]), n, steps


@functools.lru_cache(maxsize=None)
def _order(d):
    from oracle import lattice
    return tuple(lattice.Masks(d).order)


def volume_grids(d, volume):
    """One lattice's volume (a Python integer per round, bit s = stabilizer s in measurement order) -> uint8 [depth, d+1, d+1]."""
    g = np.zeros((len(volume), d + 1, d + 1), dtype=np.uint8)
    for t, w in enumerate(volume):
        for s, (a, b) in enumerate(_order(d)):
            g[t, a, b] = (w >> s) & 1
    return g


def rule_action(dq, cfg, rec):
    """The rule of dq_envb_uf_select for one lattice of COracleWideEnv.export(): union-find on the whole volume as one last window, then
    decoder.frame_to_actions against the completed set; the identity where done."""
    d, depth = cfg["d"], cfg["volume_depth"]
    layers = dq.decoder.action_layers(cfg["error_model"], cfg["use_Y"])
    if rec["done"]:
        return layers * d * d
    frame = W.decode(d, volume_grids(d, rec["volume"])[None], depth, depth)[0][0]
    completed = {a for a in range(layers * d * d + 1) if (rec["completed"] >> a) & 1}
    return dq.decoder.frame_to_actions(frame, completed, d, cfg["error_model"], cfg["use_Y"])[1]


@functools.lru_cache(maxsize=None)
def replay(name):
    """The oracle environment played by the numpy rule with auto-reset.  Returns dict(state: uint64 [steps + 1, n, state_words] exported in front of each
    step and after the last, action int32 [steps, n], reward, done, legal of after each step, events)."""
    from oracle import c_oracle
    dq = importlib.import_module("deepq-decoding_amd")
    kw, n, steps = env_kwargs(name)
    ref = c_oracle.COracleWideEnv(n_envs=n, seed=SEED, env_id_base=0, **kw)
    identity = ref.num_actions - 1
    ref.reset()
    ev = dict(live=0, done_visits=0, flips=0, second_flips=0, reward=0)
    out = dict(state=[], action=[], reward=[], done=[], legal=[], legal0=ref.legal.copy())
    for _ in range(steps):
        out["state"].append(ref.export_state())
        recs = ref.export()
        a = np.array([rule_action(dq, kw, r) for r in recs], dtype=np.int32)
        for r, ai in zip(recs, a):
            if r["done"]:
                ev["done_visits"] += 1
                assert ai == identity
                continue
            ev["live"] += 1
            if ai != identity:
                ev["flips"] += 1
                ev["second_flips"] += int(r["completed"] != 0)
        ref.step(a, auto_reset=True, want_obs=False)
        ev["reward"] += int((ref.reward == 1.0).sum())
        out["action"].append(a)
        out["reward"].append(ref.reward.copy())
        out["done"].append(ref.done.copy())
        out["legal"].append(ref.legal.copy())
    out["state"].append(ref.export_state())
    out = {k: np.stack(v) if isinstance(v, list) else v for k, v in out.items()}
    for v in out.values():
        v.setflags(write=False)
    out["events"] = ev
    out["identity"] = identity
    return out


def assert_minimums(name, ev):
    _, n, steps = CONFIGS[name]
    assert ev["live"] + ev["done_visits"] == n * steps
    assert ev["flips"] >= n * steps / 2, (name, ev)
    assert ev["second_flips"] >= ev["flips"] / 2, (name, ev)
    assert ev["done_visits"] >= max(1, MIN_DONE.get(name, 0)), (name, ev)
    assert ev["reward"] >= MIN_REWARD.get(name, 0), (name, ev)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_the_rule_on_the_oracle_environment_meets_the_event_minimums(dq, name):
    r = replay(name)
    _, n, steps = CONFIGS[name]
    assert r["action"].shape == (steps, n) and hasattr(dq.decoder_wide, "WideUnionFindAgent")
    assert_minimums(name, r["events"])


# ---- the numpy statements ---------------------------------------------------------------------------------------------------------------------------
def _random_legal(rng, n, LW, n_actions):
    words = np.zeros((n, LW), dtype=np.uint64)
    sets = []
    for i in range(n):
        s = sorted(set(rng.choice(n_actions - 1, size=int(rng.integers(1, 12)), replace=False).tolist()) | {n_actions - 1})
        sets.append(s)
        for a in s:
            words[i, a >> 6] |= np.uint64(1) << np.uint64(a & 63)
    return words, sets


def test_guided_actions_wide_is_guided_actions_on_two_words(dq):
    rng = np.random.default_rng(11)
    n, A = 400, 99
    words, _ = _random_legal(rng, n, 2, A)
    q = rng.standard_normal((n, A)).astype(np.float32)
    q[:, 7] = q[:, 3]                                                                   # ties
    teacher = rng.integers(0, A, size=n)
    for eps, share, masked, t, base, qq in ((0.5, 0.5, False, 3, 0, q), (0.3, 0.0, True, (1 << 40) + 1, 77, q), (1.0, 1.0, False, 9, 5, q), (0.2, 0.9, True, 0, 2 ** 32 - 100, None)):
        want = dq.decoder.guided_actions(qq, words.view(np.int64), teacher, eps, share, masked, SEED, base, t)
        got = dq.decoder_wide.guided_actions_wide(qq, words.view(np.int64), teacher, eps, share, masked, SEED, base, t)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[0].dtype == np.int32 and got[1].dtype == np.uint8
    for bad in (dict(eps=1.5, guide_share=0.5), dict(eps=0.5, guide_share=-0.1), dict(eps=float("nan"), guide_share=0.5)):
        with pytest.raises(ValueError):
            dq.decoder_wide.guided_actions_wide(q, words, teacher, masked_greedy=False, seed=SEED, env_id_base=0, t=0, **bad)
    with pytest.raises(ValueError):
        dq.decoder_wide.guided_actions_wide(q, words, teacher[:5], 0.5, 0.5, False, SEED, 0, 0)


def test_guided_actions_wide_on_eleven_words_restates_select_action(dq):
    from oracle import dqn_oracle, philox
    rng = np.random.default_rng(12)
    n, A, LW, eps, share, t, base = 600, 676, 11, 0.5, 0.4, 21, 4000                    # d = 15 with use_Y: 3 x 225 + 1 actions
    words, _ = _random_legal(rng, n, LW, A)
    q = rng.standard_normal((n, A)).astype(np.float32)
    teacher = rng.integers(0, A, size=n)
    seen = set()
    for masked in (False, True):
        a, g = dq.decoder_wide.guided_actions_wide(q, words, teacher, eps, share, masked, SEED, base, t)
        for i in range(n):
            w = philox.site_words(SEED, base + i, t, 0, stream=philox.STREAM_POLICY)
            explore = int(w[1]) < philox.threshold(eps)
            guided = explore and int(w[2]) < philox.threshold(share)
            assert g[i] == int(guided)
            mask = sum(int(x) << (64 * k) for k, x in enumerate(words[i]))
            assert a[i] == (teacher[i] if guided else dqn_oracle.select_action(q[i], mask, eps, masked, w))
            seen.add("guided" if guided else "uniform" if explore else "greedy")
    assert seen == {"guided", "uniform", "greedy"}


@pytest.mark.parametrize("name", ["d9hot", "d15dpy"])
def test_completed_from_state_reads_the_export_layout(dq, name):
    r = replay(name)
    from oracle import c_oracle
    kw, n, _ = env_kwargs(name)
    LW = c_oracle.COracleWideEnv(n_envs=1, seed=SEED, **kw).legal_words
    W_ = (kw["d"] ** 2 + 63) // 64
    nonempty = 0
    for row in r["state"][7]:
        want = sum(int(row[5 * W_ + 1 + k]) << (64 * k) for k in range(LW))
        got = dq.decoder_wide.completed_from_state(row, kw["d"], LW)
        assert got == {a for a in range(64 * LW) if (want >> a) & 1}
        assert dq.decoder_wide.completed_from_state(row.view(np.int64), kw["d"], LW) == got          # (VectorEnv.export_state is int64)
        nonempty += bool(got)
    assert nonempty >= n // 2


# ---- validation before any library call -------------------------------------------------------------------------------------------------------------------
def _no_library(monkeypatch):
    _lib = importlib.import_module("deepq-decoding_amd._lib")

    def no_library(*a, **k):
        raise AssertionError("a library call was made before the arguments were validated")
    monkeypatch.setattr(_lib, "lib", no_library)
    monkeypatch.setattr(_lib, "require_gpu", no_library)
    monkeypatch.setattr(_lib, "check", no_library)
    env_mod = importlib.import_module("deepq-decoding_amd.env")
    monkeypatch.setattr(env_mod, "check", no_library)
    return env_mod


def _wide_ev(**kw):
    return types.SimpleNamespace(**dict(dict(d=9, error_model="DP", window=5, chunk=64, _h=1), **kw))


def test_arguments_are_validated_before_the_library_is_touched(dq, monkeypatch):
    env_mod = _no_library(monkeypatch)
    e = object.__new__(env_mod.VectorEnv)

    def lattice(**kw):
        base = dict(d=9, error_model="DP", use_Y=False, volume_depth=5, wide=True, n_envs=4, num_actions=163)
        base.update(kw)
        for k, v in base.items():
            setattr(e, k, v)
        return e

    ev = _wide_ev()
    narrow_ev = types.SimpleNamespace(d=9, error_model="DP", use_Y=False, volume_depth=5, _h=1)
    for call in (lambda env, x, **kw: env.uf_select_wide(x, **kw), lambda env, x, **kw: env.guided_select_wide(x, 0, **kw)):
        with pytest.raises(NotImplementedError, match=r'match_select\(method="union_find"\)'):
            call(lattice(d=5, wide=False), _wide_ev(d=5))                            # a narrow handle
        with pytest.raises(ValueError):
            call(lattice(), narrow_ev)                                                 # a decoder.Evaluator: no window
        with pytest.raises(ValueError):
            call(lattice(), _wide_ev(d=11))                                            # another d
        with pytest.raises(ValueError):
            call(lattice(), _wide_ev(error_model="X"))                                 # another error model
        with pytest.raises(ValueError):
            call(lattice(), _wide_ev(window=4))                                        # a window below the depth
        with pytest.raises(ValueError):
            call(lattice(), ev, out=np.zeros(4, np.int32))                             # outputs live on the device
    for kw in (dict(guide_share=1.5), dict(guide_share=-0.01), dict(guide_share=float("nan")), dict(eps=2.0), dict(eps=True), dict(guide_share="0.5")):
        with pytest.raises(ValueError):
            lattice().guided_select_wide(ev, 0, **kw)
    for t in (-1, 1.5, True):
        with pytest.raises(ValueError):
            lattice().guided_select_wide(ev, t)
    with pytest.raises(ValueError):
        lattice().guided_select_wide(ev, 0, q=np.zeros((4, 163), np.float32))          # q lives on the device
    with pytest.raises(ValueError):
        lattice().guided_select_wide(ev, 0, out_guided=np.zeros(4, np.uint8))
    # the agent validates the lattice it is asked to play, before any library call
    A = dq.decoder_wide.WideUnionFindAgent
    stub = lambda **kw: types.SimpleNamespace(**dict(dict(d=9, error_model="DP", use_Y=False, volume_depth=5, wide=True, n_envs=8, identity_index=162), **kw))
    for how in (lambda a, s: a.evaluator_for(s), lambda a, s: a.test(s, verbose=0), lambda a, s: a.test_error_rates(s, [0.01], verbose=0)):
        with pytest.raises(NotImplementedError, match="MatchingAgent"):
            how(A(), stub(d=5, wide=False))
        with pytest.raises(NotImplementedError):
            how(A(), stub(volume_depth=17))
        with pytest.raises(ValueError):
            how(A(evaluator=_wide_ev(window=4)), stub())
        with pytest.raises(ValueError):
            how(A(evaluator=_wide_ev(d=11)), stub())
        with pytest.raises(ValueError):
            how(A(evaluator=narrow_ev), stub())
    assert A(evaluator=ev).evaluator_for(stub()) == (ev, False)                        # its own evaluator stays the agent's to close
    assert A(evaluator=_wide_ev(window=16)).evaluator_for(stub())[1] is False          # a wider window serves
    with pytest.raises(ValueError):
        A(policy="greedy")
    with pytest.raises(ValueError):
        A(chunk=0)


def test_the_narrow_entry_points_still_refuse_a_wide_handle(dq, monkeypatch):
    env_mod = _no_library(monkeypatch)
    e = object.__new__(env_mod.VectorEnv)
    for k, v in dict(d=9, error_model="DP", use_Y=False, volume_depth=5, wide=True, n_envs=4, num_actions=163).items():
        setattr(e, k, v)
    narrow_ev = types.SimpleNamespace(d=9, error_model="DP", use_Y=False, volume_depth=5, _h=1)
    for method in ("matching", "union_find"):
        with pytest.raises(NotImplementedError):
            e.match_select(narrow_ev, method=method)
        with pytest.raises(NotImplementedError):
            e.guided_select(narrow_ev, 0, method=method)
        stub = types.SimpleNamespace(d=9, error_model="DP", use_Y=False, volume_depth=5, wide=True, n_envs=8, identity_index=162)
        with pytest.raises(NotImplementedError):
            dq.decoder.MatchingAgent(method=method).test(stub, verbose=0)
        with pytest.raises(NotImplementedError):
            dq.decoder.MatchingAgent(method=method).evaluator_for(stub)
    core = object.__new__(dq.DQNCore)
    core._wide, core.world_size = True, 1
    with pytest.raises(NotImplementedError):
        core.guided_act_and_step(narrow_ev, 1.0, 1.0)
    core._wide = False
    with pytest.raises(NotImplementedError):
        core.guided_act_and_step_wide(_wide_ev(), 1.0, 1.0)                            # ... and the wide step refuses a narrow core
    core._wide, core.world_size = True, 2
    with pytest.raises(NotImplementedError):
        core.guided_act_and_step_wide(_wide_ev(), 1.0, 1.0)


# ---- the agent's plumbing on stub environments ----------------------------------------------------------------------------------------------------------
class _StubEnv:
    """What WideUnionFindAgent._records and MatchingAgent.test_error_rates touch of a VectorEnv, recording the calls."""
    wide, d, error_model, use_Y, volume_depth, identity_index, device, L = True, 9, "DP", False, 5, 162, "cpu", None

    def __init__(self, n_envs):
        self.n_envs, self.calls, self._h = n_envs, [], 1
        self.done = self.was_reset = self.reward = self.lifetime = None
        self.rates = (0.5, 0.5)

    def _stream(self):
        return 0

    def reset(self, write_obs=True):
        self.calls.append(("reset", write_obs))

    def uf_select_wide(self, ev, out=None):
        self.calls.append(("select", ev, out))
        return out

    def step(self, action, auto_reset=False, write_obs=True):
        self.calls.append(("step", action, auto_reset, write_obs))

    def _rate_forms(self):
        return self.rates

    def set_rates(self, ph, pm=None):
        self.calls.append(("rates", None if np.ndim(ph) == 0 else np.asarray(ph).copy()))
        self.rates = (ph, pm)


def _stub_episodes(monkeypatch, n_steps):
    episodes = importlib.import_module("deepq-decoding_amd.episodes")
    seen = {}

    def episode_records(L, dev, stream, N, quota, step, extra, cap):
        seen.update(N=N, quota=np.asarray(quota).copy(), cap=cap)
        for k in range(n_steps):
            step(k)
        return np.zeros((0, 5), dtype=np.int32)
    monkeypatch.setattr(episodes, "episode_records", episode_records)
    return seen


class _FakeTorch:
    """torch.full / torch.cuda.device for a run without a device: the action buffer is a numpy array."""
    int32 = np.int32

    class cuda:
        @staticmethod
        def device(dev):
            import contextlib
            return contextlib.nullcontext()

    @staticmethod
    def full(shape, value, dtype=None, device=None):
        return np.full(shape, value, dtype=dtype)


def test_agent_plumbing_select_then_step(dq, monkeypatch):
    import sys
    assert dq.DQNAgent and dq.decoder_wide                                            # (imported with the real torch, before the stand-in below)
    monkeypatch.setitem(sys.modules, "torch", _FakeTorch)
    seen = _stub_episodes(monkeypatch, 3)
    ev = _wide_ev()
    env = _StubEnv(8)
    agent = dq.decoder_wide.WideUnionFindAgent(evaluator=ev)
    assert isinstance(agent, dq.decoder.MatchingAgent) and agent.method == "union_find" and agent.policy == "matching"
    rec, inexact = agent._records(env, np.full(8, 2), 1500)
    kinds = [c[0] for c in env.calls]
    assert kinds == ["reset", "select", "step", "select", "step", "select", "step"] and env.calls[0] == ("reset", False)
    assert all(c[1] is ev for c in env.calls if c[0] == "select")
    sel = [c[2] for c in env.calls if c[0] == "select"]
    stp = [c for c in env.calls if c[0] == "step"]
    assert all(s[1] is sel[0] and s[2] is True and s[3] is False for s in stp) and all(x is sel[0] for x in sel)
    assert sel[0].dtype == np.int32 and (sel[0] == 162).all()
    assert seen["N"] == 8 and seen["cap"] == 1500 and agent.last_vector_steps == 3
    assert inexact.shape == (8,) and not inexact.any()
    # the identity row: no select
    env2 = _StubEnv(8)
    ident = dq.decoder_wide.WideUnionFindAgent(policy="identity")
    ident._records(env2, np.full(8, 2), None)
    assert [c[0] for c in env2.calls] == ["reset", "step", "step", "step"]


def test_agent_error_rate_blocks(dq, monkeypatch):
    import sys
    assert dq.DQNAgent and dq.decoder_wide                                            # (imported with the real torch, before the stand-in below)
    monkeypatch.setitem(sys.modules, "torch", _FakeTorch)
    episodes = importlib.import_module("deepq-decoding_amd.episodes")
    seen = _stub_episodes(monkeypatch, 1)
    env = _StubEnv(12)
    agent = dq.decoder_wide.WideUnionFindAgent(evaluator=_wide_ev())
    rates, m, ph, pm, quota = episodes.rate_blocks(12, [0.004, 0.008, 0.012], 5, None)
    out = agent.test_error_rates(env, [0.004, 0.008, 0.012], nb_episodes=5, verbose=0)
    assert list(out) == [0.004, 0.008, 0.012] and agent.last_inexact_steps == 0 and agent.last_inexact_by_rate == {0.004: 0, 0.008: 0, 0.012: 0}
    set_calls = [c for c in env.calls if c[0] == "rates"]
    assert np.array_equal(set_calls[0][1], np.asarray(ph)) and m == 4 and np.array_equal(set_calls[0][1][:4], [0.004] * 4)
    assert set_calls[-1][1] is None and env.rates == (0.5, 0.5)                          # the previous rates are restored
    assert np.array_equal(seen["quota"], quota)
    # the same quota the narrow agent hands down
    h = agent.test(env, nb_episodes=24, verbose=0)
    assert np.array_equal(seen["quota"], episodes.share_quota(12, 24)) and hasattr(h, "history")


def test_the_policy_accepts_the_wide_agent(dq):
    guide = dq.decoder_wide.WideUnionFindAgent()
    pol = dq.EpsGreedyQPolicy(masked_greedy=True, guide=guide, guide_share=0.25)
    assert pol.guide is guide and pol.guide_share == 0.25
    outer = dq.LinearAnnealedPolicy(pol, attr="eps", value_max=1.0, value_min=0.0, value_test=0.0, nb_steps=100)
    assert outer.guide is guide
    with pytest.raises(ValueError):
        dq.EpsGreedyQPolicy(guide=dq.decoder_wide.WideUnionFindAgent(policy="identity"))
    assert dq.WideUnionFindAgent is dq.decoder_wide.WideUnionFindAgent and dq.guided_actions_wide is dq.decoder_wide.guided_actions_wide
    assert dq.completed_from_state is dq.decoder_wide.completed_from_state


def test_abi_is_declared_and_bound():
    L = importlib.import_module("deepq-decoding_amd._lib")
    lib = L.lib()
    assert lib.dq_version() == 8
    header = open(os.path.join(os.path.dirname(L.__file__), "..", "include", "deepq_hip.h")).read()
    vp, dbl, i32 = ctypes.c_void_p, ctypes.c_double, ctypes.c_int
    assert "dq_envb_uf_select(dq_envb* env, dq_wide_uf* h, int32_t* action_dev, void* stream)" in header and hasattr(lib, "dq_envb_uf_select")
    assert "dq_envb_guided_select_uf(dq_envb* env, dq_wide_uf* h, const float* q_dev, double eps, double guide_share, int masked_greedy," in header
    assert hasattr(lib, "dq_envb_guided_select_uf")
    assert L.SIGNATURES["dq_envb_uf_select"] == (i32, [vp, vp, vp, vp])
    assert L.SIGNATURES["dq_envb_guided_select_uf"] == (i32, [vp, vp, vp, dbl, dbl, i32, ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint64, vp, vp, vp])
    seed = (ctypes.c_uint32 * 2)(1, 2)
    assert lib.dq_envb_uf_select(None, None, None, None) == -1                         # DQ_ERR_INVALID on null handles, no device touched
    assert lib.dq_envb_guided_select_uf(None, None, None, 0.5, 0.5, 0, seed, 0, None, None, None) == -1
    digest = importlib.import_module("deepq-decoding_amd._digest")
    import glob
    names = {os.path.basename(f) for f in glob.glob(os.path.join(digest.HERE, "csrc", "*"))}
    assert {"env_wide_uf.hip", "env_big_view.h", "uf_wide.h"} <= names
    assert lib.dq_build_digest().decode() == digest.csrc_digest()
