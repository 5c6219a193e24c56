"""The correlated union-find decoder as a policy and a teacher of the wide environment, host side (VectorEnv.uf_select_wide / guided_select_wide(correlated=),
decoder_wide.WideUnionFindAgent(correlated=), DQNCore.guided_act_and_step_wide(correlated=)): the rule replayed on the C oracle
environment (tests/correlated_env_uf_ref.py) -- its reduction to the weighted rule, how often it acts differently, the event minimums that keep the device's
lockstep from being vacuous --, validation before any library call, what every entry point hands the library, the two "rates" caches, and the C ABI.

Figures of the replays (SEED, env_id_base 0), the rule under uf_weights_correlated of the rates against the weighted rule of the same pair on the same records:
    d = 5, DP, depth 5, 0.004 / 0.04, 64 x 40          (7, 4, 1)   202 / 2553 live lattice-steps differ (7.9 %)
    d = 5, DP, use_Y, depth 5, 0.01 / 0.01, 64 x 40    (8, 7, 1)   399 / 2546 (15.7 %)
    d = 9, DP, depth 5, 0.004 / 0.04, 32 x 24          (7, 4, 1)   66 / 768 (8.6 %)"""
import ctypes
import importlib
import os
import types

import numpy as np
import pytest

import correlated_env_uf_ref as R
from test_weighted_env_uf_cpu import _lattice, _WeightedStubEnv
from test_wide_env_uf_cpu import _FakeTorch, _no_library, _stub_episodes, _wide_ev


# ---- 1. the rule ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.CPU_CONFIGS)
def test_w_corr_equal_to_w_space_is_the_weighted_rule(dq, name):
    """On every record of the run the three passes under (w_space, w_time, w_space) choose weighted_env_uf_ref.rule_action's action under (w_space, w_time)."""
    r = R.replay(name)
    _, n, steps, _ = R.CONFIGS[name]
    assert r["triple"] == R.run_triple(dq, name) and r["action"].shape == r["weighted"].shape == (steps, n)
    assert np.array_equal(R.at_w_space(r), r["weighted"]), name
    R.assert_minimums(name, r["events"])


def test_under_the_x_model_w_corr_changes_nothing(dq):
    """d = 5, X: component 1 is not decoded, so there is no mask; under every triple the action is the weighted rule's under the triple's pair."""
    r = R.replay("d5x")
    assert r["triple"] == (5, 3, 5) and r["events"]["differ"] == 0 and np.array_equal(r["action"], r["weighted"])
    assert set(r["weighted_other"]) == set(r["other"]) >= {(4, 4, 1), (8, 7, 2), (15, 15, 1), (15, 1, 1)}
    for p, a in r["other"].items():
        assert np.array_equal(a, r["weighted_other"][p]), p
    assert (r["other"][(4, 4, 1)] != r["action"]).any()                                  # (the pairs matter on these records)
    assert r["events"]["done_visits"] >= 20


@pytest.mark.parametrize("name", R.DP_CONFIGS)
def test_the_correlated_rule_differs_from_the_weighted_rule_often_enough(dq, name):
    r = R.replay(name)
    ev = r["events"]
    assert r["triple"] == R.run_triple(dq, name) and r["triple"][2] == 1 < r["triple"][0]
    print(f"{name} {r['triple']}: {ev['differ']} / {ev['live']} live lattice-steps differ from the weighted rule, {ev['ended']} episodes ended")
    assert ev["differ"] >= ev["live"] / 20, (name, ev)
    assert ev["differ"] == int((r["weighted"] != r["action"]).sum())                     # (a done lattice gets the identity under every rule)
    R.assert_minimums(name, ev)
    # the triples launched beside the run's own are not copies of it or of one another on these records
    assert (r["other"][(4, 4, 1)] != r["action"]).any() and (r["other"][(8, 7, 2)] != r["other"][(4, 4, 1)]).any(), name


def test_the_configurations_are_the_ones_asked_for(dq):
    assert [R.run_triple(dq, k) for k in ("d5dp", "d5dpy", "d9dp", "d13iid_321", "d13iid_442", "d15dpy", "d15deep")] == [
        (7, 4, 1), (8, 7, 1), (7, 4, 1), (3, 2, 1), (4, 4, 2), (5, 3, 1), (5, 3, 1)]
    assert R.CONFIGS["d15deep"][0]["volume_depth"] == 16 and R.CONFIGS["d15deep"][1:3] == (4, 8)
    assert R.CONFIGS["d15dpy"][0]["volume_depth"] == 3 and R.CONFIGS["d15dpy"][1:3] == (16, 12)
    cfg = R.CONFIGS["d13iid_321"][0]
    assert dq.uf_weights_correlated(cfg["p_phys"], cfg["p_meas"], "IIDXZ")[2] == dq.uf_weights(cfg["p_phys"], cfg["p_meas"], "IIDXZ")[0]      # a no-op
    assert set(R.DIFFERING) == {"d5dp", "d5dpy", "d9dp", "d15dpy", "d15deep"}


# ---- 2. validation before any library call -----------------------------------------------------------------------------------------------------------
# (weights, correlated) that no entry point takes
BAD = [(None, 1), ("rates", 1), ((4, 2), 5), ((4, 2), 0), ((4, 2), 16), ((4, 2), 1.0), ((4, 2), True), ((4, 2), "rate"), ((4, 2), "rates"), ((4, 2), (1,)),
       (np.array([[4, 2], [2, 2], [4, 4], [4, 1]]), 3), ([[4, 2]] * 4, "rates"), ((4, 2, 1), None), ((4, 2, 1), 1), (None, "RATES"), (None, -1),
       (np.array([[4, 2, 1]] * 4), None)]
GOOD = [((4, 2), 1), ((4, 2), 4), ([15, 15], 15), ((1, 1), 1), (None, "rates"), ("rates", "rates"), (np.array([[4, 2], [2, 2], [4, 4], [4, 1]]), 2),
        ([[4, 2]] * 4, np.int64(4))]


def _corr_lattice(env_mod, **kw):
    return _lattice(env_mod, **dict(dict(_uf_rate_triples=None), **kw))


def test_correlated_is_validated_before_the_library_is_touched(dq, monkeypatch):
    env_mod = _no_library(monkeypatch)
    DW = dq.decoder_wide
    ev = _wide_ev()
    core = object.__new__(dq.DQNCore)
    core._wide, core.world_size = True, 1
    stub = types.SimpleNamespace(d=9, error_model="DP", use_Y=False, volume_depth=5, wide=True, n_envs=4, identity_index=162)
    for w, c in BAD:
        with pytest.raises(ValueError):
            _corr_lattice(env_mod).uf_select_wide(ev, weights=w, correlated=c)
        with pytest.raises(ValueError):
            _corr_lattice(env_mod).guided_select_wide(ev, 0, weights=w, correlated=c)
        core.env = _corr_lattice(env_mod)
        with pytest.raises(ValueError):
            core.guided_act_and_step_wide(ev, 1.0, 1.0, weights=w, correlated=c)
        with pytest.raises(ValueError):                                                  # (an array of another lattice count: refused with the lattices in sight)
            a = DW.WideUnionFindAgent(evaluator=ev, weights=w, correlated=c)
            a.test(stub, verbose=0)
    with pytest.raises(ValueError):                                                      # "rates" reads the wide handle's per-lattice rates
        _corr_lattice(env_mod, d=5, wide=False).uf_select_wide(_wide_ev(d=5), correlated="rates")
    with pytest.raises(ValueError):
        _corr_lattice(env_mod, d=5, wide=False).guided_select_wide(_wide_ev(d=5), 0, correlated="rates")
    with pytest.raises(NotImplementedError):                                             # ... and a triple does not make a narrow handle a wide one
        _corr_lattice(env_mod, d=5, wide=False).uf_select_wide(_wide_ev(d=5), weights=(2, 1), correlated=1)
    with pytest.raises(ValueError):
        DW.WideUnionFindAgent(policy="identity", correlated="rates")
    with pytest.raises(ValueError):
        DW.WideUnionFindAgent(policy="identity", weights=(4, 2), correlated=1)
    # the other arguments are still checked under correlated
    with pytest.raises(ValueError):
        _corr_lattice(env_mod).uf_select_wide(_wide_ev(window=4), weights=(4, 2), correlated=1)
    with pytest.raises(ValueError):
        _corr_lattice(env_mod).guided_select_wide(ev, 0, guide_share=1.5, correlated="rates")
    # what passes: the next thing touched is the library, through the correlated symbols
    for w, c in GOOD:
        with pytest.raises(AssertionError, match="library call was made: dq_envb_uf_select_correlated$"):
            _corr_lattice(env_mod).uf_select_wide(ev, weights=w, correlated=c)
        with pytest.raises(AssertionError, match="library call was made: dq_envb_guided_select_uf_correlated$"):
            _corr_lattice(env_mod).guided_select_wide(ev, 0, weights=w, correlated=c)
        a = DW.WideUnionFindAgent(evaluator=ev, weights=w, correlated=c)
        assert a.evaluator_for(stub) == (ev, False) and a.correlated == c
    # correlated=None: the entry points of before are the ones touched
    with pytest.raises(AssertionError, match="dq_envb_uf_select$"):
        _corr_lattice(env_mod).uf_select_wide(ev, correlated=None)
    with pytest.raises(AssertionError, match="dq_envb_uf_select_weighted$"):
        _corr_lattice(env_mod).uf_select_wide(ev, weights=(4, 2), correlated=None)
    with pytest.raises(AssertionError, match="dq_envb_guided_select_uf_weighted$"):
        _corr_lattice(env_mod).guided_select_wide(ev, 0, weights="rates")
    # ... also on a handle made before the triples had a cache
    with pytest.raises(AssertionError, match="dq_envb_uf_select_correlated$"):
        _lattice(env_mod).uf_select_wide(ev, correlated="rates")


def test_a_device_tensor_of_triples_is_checked_by_shape_and_type(dq):
    """check_policy_weights on stand-ins for device tensors: uint8 [n, 2] and [n, 3] pass as they are, everything else is a ValueError."""
    DW = dq.decoder_wide

    def dev(shape, dtype="torch.uint8"):
        return types.SimpleNamespace(is_cuda=True, shape=shape, dtype=dtype)

    for shape in ((4, 2), (4, 3)):
        t = dev(shape)
        assert DW.check_policy_weights(t, 4) is t and DW.check_policy_weights(t) is t
    for t in (dev((4, 4)), dev((4,)), dev((3, 3)), dev((4, 3), "torch.int32")):
        with pytest.raises(ValueError):
            DW.check_policy_weights(t, 4)
    assert DW.is_correlated(dev((4, 3))) and not DW.is_correlated(dev((4, 2)))
    with pytest.raises(ValueError, match="triples already"):
        DW.WideUnionFindAgent(weights=dev((4, 3)), correlated=1)


# ---- 3. what the entry points hand the library -----------------------------------------------------------------------------------------------------------
def _recording(env_mod, monkeypatch):
    monkeypatch.setattr(env_mod, "check", lambda status: None)
    monkeypatch.setattr(env_mod.VectorEnv, "_check_outputs", lambda self, who, *pairs: None)       # (the outputs of these tests live on the host)
    calls = []
    names = dict(dq_envb_uf_select="select", dq_envb_uf_select_weighted="select_w", dq_envb_uf_select_correlated="select_c",
                 dq_envb_guided_select_uf="guided", dq_envb_guided_select_uf_weighted="guided_w", dq_envb_guided_select_uf_correlated="guided_c")
    L = types.SimpleNamespace(**{sym: (lambda *a, tag=tag: calls.append((tag,) + a)) for sym, tag in names.items()})
    return calls, L


def test_the_entry_points_hand_the_triple_to_the_library(dq, monkeypatch):
    import torch
    env_mod = importlib.import_module("deepq-decoding_amd.env")
    calls, L = _recording(env_mod, monkeypatch)
    e = _corr_lattice(env_mod, L=L, _stream=lambda: "stream")
    ev = _wide_ev(_h="uf")
    DW = dq.decoder_wide
    out, flag = torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.uint8)
    assert e.uf_select_wide(ev, out=out, weights=(7, 4), correlated=1) is out
    assert calls.pop() == ("select_c", 1, "uf", 7, 4, 1, None, out.data_ptr(), "stream")
    e.uf_select_wide(ev, out=out, weights=[[4, 2], [3, 4], [5, 6], [7, 8]], correlated=3)
    got = calls.pop()
    assert got[:6] == ("select_c", 1, "uf", 1, 1, 1) and got[6] is not None and got[7:] == (out.data_ptr(), "stream")
    e.guided_select_wide(ev, 7, eps=0.5, guide_share=0.25, masked_greedy=True, out=out, out_guided=flag, weights=(7, 4), correlated=2)
    got = calls.pop()
    assert got[:7] == ("guided_c", 1, "uf", None, 0.5, 0.25, 1) and list(got[7]) == [1, 2]
    assert got[8:] == (7, 7, 4, 2, None, out.data_ptr(), flag.data_ptr(), "stream")
    # correlated=None: the calls of before, argument for argument
    e.uf_select_wide(ev, out=out)
    assert calls.pop() == ("select", 1, "uf", out.data_ptr(), "stream")
    e.uf_select_wide(ev, out=out, weights=(5, 3))
    assert calls.pop() == ("select_w", 1, "uf", 5, 3, None, out.data_ptr(), "stream")
    e.guided_select_wide(ev, 7, eps=0.5, guide_share=0.25, out=out, out_guided=flag, weights=(7, 4))
    assert calls.pop()[0] == "guided_w"
    # "rates": rate_weights_correlated of the rates as they stand, uploaded once in a cache of its own
    triple = DW.uf_weights_correlated(0.004, 0.04, "DP")
    e.uf_select_wide(ev, out=out, correlated="rates")
    first = e._uf_rate_triples
    assert first.dtype == torch.uint8 and first.tolist() == [list(triple)] * 4 and triple == (7, 4, 1)
    assert calls.pop() == ("select_c", 1, "uf", 1, 1, 1, first.data_ptr(), out.data_ptr(), "stream")
    e.guided_select_wide(ev, 0, out=out, weights="rates", correlated="rates")
    assert e._uf_rate_triples is first and calls.pop()[12] == first.data_ptr() and e._uf_rate_weights is None
    # the weighted cache and the correlated one on one handle each survive the other ...
    e.uf_select_wide(ev, out=out, weights="rates")
    pairs = e._uf_rate_weights
    assert calls.pop() == ("select_w", 1, "uf", 1, 1, pairs.data_ptr(), out.data_ptr(), "stream") and pairs.tolist() == [[7, 4]] * 4
    e.uf_select_wide(ev, out=out, correlated="rates")
    assert e._uf_rate_triples is first and e._uf_rate_weights is pairs and calls.pop()[6] == first.data_ptr()
    e.uf_select_wide(ev, out=out, weights="rates")
    assert e._uf_rate_triples is first and e._uf_rate_weights is pairs and calls.pop()[5] == pairs.data_ptr()
    # ... and die on set_rates
    e.L.dq_envb_set_rates = lambda *a: 0
    e._pfx = "dq_envb_"
    e.set_rates(0.01, 0.01)
    assert e._uf_rate_weights is None and e._uf_rate_triples is None
    e.uf_select_wide(ev, out=out, correlated="rates")
    assert calls.pop()[6] == e._uf_rate_triples.data_ptr() and e._uf_rate_triples.tolist() == [[8, 7, 1]] * 4 and e._uf_rate_weights is None
    # per-lattice rates: every lattice its own triple
    ph = np.array([0.004, 0.004, 0.012, 0.012])
    e._rates_arr, e._uf_rate_triples = (ph, np.full(4, 0.04)), None
    e.uf_select_wide(ev, out=out, correlated="rates")
    assert e._uf_rate_triples.tolist() == [list(DW.uf_weights_correlated(p, 0.04, "DP")) for p in ph]
    assert e._uf_rate_triples[0].tolist() != e._uf_rate_triples[2].tolist()


def test_the_guided_step_resolves_once_and_hands_the_triple_on(dq, monkeypatch):
    """DQNCore.guided_act_and_step_wide validates through the environment before its forward; what it would hand guided_select_wide is the pair with the
    integer, or the device tensor of triples."""
    env_mod = _no_library(monkeypatch)
    core = object.__new__(dq.DQNCore)
    core._wide, core.world_size = True, 1
    core.env = _corr_lattice(env_mod)
    seen = []

    def stop():
        seen.append("forward next")
        raise AssertionError("validated")
    core._flush_stats = stop
    with pytest.raises(AssertionError, match="validated"):
        core.guided_act_and_step_wide(_wide_ev(), 1.0, 1.0, weights=(7, 4), correlated=1)
    with pytest.raises(ValueError):
        core.guided_act_and_step_wide(_wide_ev(), 1.0, 1.0, weights=(7, 4), correlated=8)
    assert seen == ["forward next"]                                                      # the refusal came in front of it


# ---- 4. the agent's plumbing on stub environments ----------------------------------------------------------------------------------------------------------
class _CorrelatedStubEnv(_WeightedStubEnv):
    """_WeightedStubEnv whose select takes correlated= too and records it behind the weights."""

    def uf_select_wide(self, ev, out=None, weights=None, correlated=None):
        ph, pm = self.rates
        self.calls.append(("select", ev, out, weights, None if np.ndim(ph) == 0 else (np.asarray(ph).copy(), np.asarray(pm).copy()), correlated))
        return out


def test_the_correlated_agent_hands_every_rate_block_its_triple(dq, monkeypatch):
    import sys
    assert dq.DQNAgent and dq.decoder_wide
    monkeypatch.setitem(sys.modules, "torch", _FakeTorch)
    episodes = importlib.import_module("deepq-decoding_amd.episodes")
    _stub_episodes(monkeypatch, 2)
    DW = dq.decoder_wide
    env = _CorrelatedStubEnv(12)
    agent = DW.WideUnionFindAgent(evaluator=_wide_ev(), correlated="rates")
    rates = [0.004, 0.008, 0.012]
    _, m, ph, pm, _ = episodes.rate_blocks(12, rates, 5, 0.04)
    out = agent.test_error_rates(env, rates, nb_episodes=5, p_meas=0.04, verbose=0)
    assert list(out) == rates and m == 4
    sel = [c for c in env.calls if c[0] == "select"]
    # the string: the environment resolves it after the sweep set its rates, every block its own triple in the same launches
    assert len(sel) == 2 and all(c[3] is None and c[5] == "rates" for c in sel)
    for c in sel:
        assert np.array_equal(c[4][0], np.asarray(ph)) and np.array_equal(c[4][1], np.asarray(pm))
    triples = [DW.uf_weights_correlated(r, 0.04, "DP") for r in rates]
    assert len(set(triples)) > 1 and agent.last_weights == sorted(set(triples)) and all(len(t) == 3 for t in agent.last_weights)
    assert env.rates == (0.5, 0.5)                                                       # the previous rates are restored
    # weights="rates" beside it goes down as the string too; a pair with its integer as they are
    env2 = _CorrelatedStubEnv(8)
    both = DW.WideUnionFindAgent(evaluator=_wide_ev(), weights="rates", correlated="rates")
    both._records(env2, np.full(8, 2), None)
    assert [(c[3], c[5]) for c in env2.calls if c[0] == "select"] == [("rates", "rates")] * 2
    assert both.last_weights == DW.uf_weights_correlated(0.5, 0.5, "DP")
    env3 = _CorrelatedStubEnv(8)
    a = DW.WideUnionFindAgent(evaluator=_wide_ev(), weights=[7, 4], correlated=2)
    a._records(env3, np.full(8, 2), None)
    assert [(c[3], c[5]) for c in env3.calls if c[0] == "select"] == [((7, 4), 2)] * 2 and a.last_weights == (7, 4, 2)
    # no correlated: the weighted call of before, argument for argument (a select that takes no correlated=)
    env4 = _WeightedStubEnv(8)
    w = DW.WideUnionFindAgent(evaluator=_wide_ev(), weights=[5, 3])
    w._records(env4, np.full(8, 2), None)
    assert [c[3] for c in env4.calls if c[0] == "select"] == [(5, 3)] * 2 and w.last_weights == (5, 3) and w.correlated is None


def test_fit_passes_the_guides_triple_to_the_guided_step(dq):
    DW = dq.decoder_wide
    calls = []
    core = types.SimpleNamespace(_wide=True, guided_act_and_step_wide=lambda *a, **k: calls.append(("wide", a, k)))
    venv = types.SimpleNamespace(n_envs=8, device="cpu")
    dq.DQNAgent._guided_step(DW.WideUnionFindAgent(correlated="rates"), core, venv)("ev", 0.5, 0.25, masked_greedy=True)
    assert calls.pop() == ("wide", ("ev", 0.5, 0.25), dict(masked_greedy=True, correlated="rates"))
    dq.DQNAgent._guided_step(DW.WideUnionFindAgent(weights="rates", correlated="rates"), core, venv)("ev", 0.5, 0.25)
    assert calls.pop() == ("wide", ("ev", 0.5, 0.25), dict(weights="rates", correlated="rates"))
    dq.DQNAgent._guided_step(DW.WideUnionFindAgent(weights=[7, 4], correlated=1), core, venv)("ev", 1.0, 1.0, record_stats=False)
    assert calls.pop() == ("wide", ("ev", 1.0, 1.0), dict(record_stats=False, weights=(7, 4), correlated=1))
    dq.DQNAgent._guided_step(DW.WideUnionFindAgent(weights=[7, 4]), core, venv)("ev", 1.0, 1.0)                       # the weighted guide: as before
    assert calls.pop() == ("wide", ("ev", 1.0, 1.0), dict(weights=(7, 4)))
    assert dq.DQNAgent._guided_step(DW.WideUnionFindAgent(), core, venv) is core.guided_act_and_step_wide
    with pytest.raises(ValueError):
        dq.DQNAgent._guided_step(DW.WideUnionFindAgent(weights=[[4, 1]] * 4, correlated=2), core, venv)              # four pairs for eight lattices
    pol = dq.EpsGreedyQPolicy(guide=DW.WideUnionFindAgent(correlated="rates"), guide_share=0.5)
    assert pol.guide.correlated == "rates" and pol.guide.weights is None


# ---- 5. the C ABI ------------------------------------------------------------------------------------------------------------------------------------------
def test_abi_is_declared_and_bound():
    L = importlib.import_module("deepq-decoding_amd._lib")
    lib = L.lib()
    assert lib.dq_version() == 8
    header = " ".join(open(os.path.join(os.path.dirname(L.__file__), "..", "include", "deepq_hip.h")).read().split())
    vp, dbl, i32 = ctypes.c_void_p, ctypes.c_double, ctypes.c_int
    assert ("dq_status dq_envb_uf_select_correlated(dq_envb* env, dq_wide_uf* h, int w_space, int w_time, int w_corr, const uint8_t* weights_each_dev, "
            "int32_t* action_dev, void* stream);") in header
    assert ("dq_status dq_envb_guided_select_uf_correlated(dq_envb* env, dq_wide_uf* h, const float* q_dev, double eps, double guide_share, "
            "int masked_greedy, const uint32_t seed[2], uint64_t t, int w_space, int w_time, int w_corr, const uint8_t* weights_each_dev, "
            "int32_t* action_dev, uint8_t* guided_dev, void* stream);") in header
    assert hasattr(lib, "dq_envb_uf_select_correlated") and hasattr(lib, "dq_envb_guided_select_uf_correlated")
    assert L.SIGNATURES["dq_envb_uf_select_correlated"] == (i32, [vp, vp, i32, i32, i32, vp, vp, vp])
    assert L.SIGNATURES["dq_envb_guided_select_uf_correlated"] == (
        i32, [vp, vp, vp, dbl, dbl, i32, ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint64, i32, i32, i32, vp, vp, vp, vp])
    # the entry points of before keep their lists
    assert L.SIGNATURES["dq_envb_uf_select_weighted"] == (i32, [vp, vp, i32, i32, vp, vp, vp]) and L.SIGNATURES["dq_envb_uf_select"] == (i32, [vp, vp, vp, vp])
    seed = (ctypes.c_uint32 * 2)(1, 2)
    # DQ_ERR_INVALID before any device work: null handles; a uniform pair outside 1 .. 15 or a uniform w_corr outside 1 .. w_space without an array
    assert lib.dq_envb_uf_select_correlated(None, None, 1, 1, 1, None, None, None) == -1
    assert lib.dq_envb_guided_select_uf_correlated(None, None, None, 0.5, 0.5, 0, seed, 0, 1, 1, 1, None, None, None, None) == -1
    for ws, wt, wc, word in ((0, 1, 1, b"weights"), (16, 1, 1, b"weights"), (4, 16, 1, b"weights"), (4, 2, 0, b"w_corr"), (4, 2, 5, b"w_corr"),
                             (4, 2, -1, b"w_corr"), (15, 15, 16, b"w_corr")):
        assert lib.dq_envb_uf_select_correlated(None, None, ws, wt, wc, None, None, None) == -1
        assert word in lib.dq_last_error(), (ws, wt, wc, lib.dq_last_error())
        assert lib.dq_envb_guided_select_uf_correlated(None, None, None, 0.5, 0.5, 0, seed, 0, ws, wt, wc, None, None, None, None) == -1
        assert word in lib.dq_last_error(), (ws, wt, wc, lib.dq_last_error())
    digest = importlib.import_module("deepq-decoding_amd._digest")
    assert lib.dq_build_digest().decode() == digest.csrc_digest()
