"""The matching decoder as a policy of the environment, host side (decoder.frame_to_actions / MatchingAgent, VectorEnv.match_select; DESIGN.md
section 14): the numpy statement of the rule on hand-written and random frames, argument validation before any library call, the shared episode
loop's quota / cap helpers and the C ABI."""
import ctypes
import importlib
import os
import types

import numpy as np
import pytest

from oracle import env_oracle, lattice

CONFIGS = [("X", False), ("DP", True), ("DP", False)]


def _xor_of_moves(d, actions, model, use_Y):
    """XOR (Pauli product up to phase) of index_to_move over the actions, as (X part, Z part) 0/1 planes."""
    x, z = np.zeros((d, d), dtype=bool), np.zeros((d, d), dtype=bool)
    for a in actions:
        mv = env_oracle.index_to_move(d, a, model, use_Y)
        x ^= (mv == 1) | (mv == 2)
        z ^= (mv == 2) | (mv == 3)
    return x, z


def _play(dq, frame, d, model, use_Y):
    """The sequence the policy emits for one volume: frame_to_actions with the growing completed set, up to the identity."""
    F = dq.decoder.frame_to_actions
    identity = lattice.num_actions(d, model, use_Y)[0] - 1
    done, seq = set(), []
    for _ in range(3 * d * d + 2):
        wanted, a = F(frame, done, d, model, use_Y)
        if a == identity:
            return wanted, seq
        assert a not in done
        seq.append(a)
        done.add(a)
    raise AssertionError("the policy did not reach the identity")


def test_hand_written_frames(dq):
    F = dq.decoder.frame_to_actions
    d = 3
    frame = np.array([[0, 1, 0], [2, 0, 3], [0, 0, 1]])                 # X at 1 and 8, Y at 3, Z at 5
    # X model: component 0 only (the X parts of X and Y cells), one layer; the Z cell has no action
    assert F(frame, None, d, "X", False) == ([1, 3, 8], 1)
    assert F(frame, {1}, d, "X", False) == ([1, 3, 8], 3)
    assert F(frame, [1, 3, 8], d, "X", False) == ([1, 3, 8], 9)        # fully completed: the identity
    # DP with use_Y: code 1 / 2 / 3 -> layer 0 / 1 / 2
    assert F(frame, None, d, "DP", True) == ([1, 8, 9 + 3, 18 + 5], 1)
    assert F(frame, {1, 8}, d, "DP", True)[1] == 12 and F(frame, {1, 8, 12, 23}, d, "DP", True)[1] == 27
    # DP without use_Y: the Y cell is the X action first, then the Z action of its qubit
    assert F(frame, None, d, "DP", False) == ([1, 3, 8, 9 + 3, 9 + 5], 1)
    y_only = np.zeros((3, 3), dtype=int)
    y_only[1, 0] = 2
    assert F(y_only, None, d, "DP", False) == ([3, 12], 3) and F(y_only, {3}, d, "DP", False)[1] == 12 and F(y_only, {3, 12}, d, "DP", False)[1] == 18
    # completed actions outside the frame change nothing; an empty frame is the identity at once
    assert F(frame, {0, 4}, d, "DP", False)[1] == 1
    assert F(np.zeros((3, 3), int), None, d, "DP", True) == ([], 27)
    # component form [2, d, d]: component 1 is ignored under X
    comps = np.zeros((2, 3, 3), dtype=int)
    comps[1, 2, 2] = 1
    assert F(comps, None, d, "X", False) == ([], 9)
    comps[0, 0, 2] = 1
    assert F(comps, None, d, "X", False) == ([2], 2) and F(comps, None, d, "DP", False) == ([2, 9 + 8], 2)
    # the flat form and bad input
    assert F(frame.reshape(-1), None, d, "DP", True)[0] == [1, 8, 12, 23]
    with pytest.raises(ValueError):
        F(np.full((3, 3), 4), None, d, "DP", True)
    with pytest.raises(ValueError):
        F(np.zeros((4, 4)), None, d, "DP", True)
    with pytest.raises(ValueError):
        F(frame, None, d, "XYZ", True)


@pytest.mark.parametrize("model,use_Y", CONFIGS)
@pytest.mark.parametrize("d", [3, 5, 7])
def test_emitted_sequence_xors_to_the_frame(dq, d, model, use_Y):
    rng = np.random.default_rng(d * 10 + len(model) + use_Y)
    for trial in range(200):
        frame = rng.integers(0, 4, size=(d, d)) * (rng.random((d, d)) < rng.choice([0.1, 0.5, 1.0]))
        wanted, seq = _play(dq, frame, d, model, use_Y)
        assert seq == wanted == sorted(set(wanted))                         # ascending, never a repeat
        x, z = _xor_of_moves(d, seq, model, use_Y)
        assert np.array_equal(x, (frame == 1) | (frame == 2))
        if model == "X":
            assert not z.any()
        else:
            assert np.array_equal(z, (frame == 2) | (frame == 3))


def test_completed_from_words(dq):
    C = dq.decoder.completed_from_words
    assert C(0, 0) == set() and C(5, 1) == {0, 2, 64} and C(np.int64(-1), 0) == set(range(64))


def _no_library(monkeypatch):
    _lib = importlib.import_module("deepq-decoding_amd._lib")

    def no_library(*a, **k):
        raise AssertionError("a library call was made before the arguments were validated")
    monkeypatch.setattr(_lib, "lib", no_library)
    monkeypatch.setattr(_lib, "require_gpu", no_library)
    monkeypatch.setattr(_lib, "check", no_library)


def _stub_env(**kw):
    base = dict(d=5, error_model="DP", use_Y=False, volume_depth=5, wide=False, n_envs=8, identity_index=50)
    base.update(kw)
    return types.SimpleNamespace(**base)


def test_arguments_are_validated_before_the_library_is_touched(dq, monkeypatch):
    _no_library(monkeypatch)
    D = dq.decoder
    ev5 = types.SimpleNamespace(d=5, error_model="DP", use_Y=False, volume_depth=5, _h=None)
    ev3 = types.SimpleNamespace(d=5, error_model="DP", use_Y=False, volume_depth=3, _h=None)
    for call in (lambda a, e: a.test(e, nb_episodes=4, verbose=0), lambda a, e: a.test_error_rates(e, [0.01, 0.02], nb_episodes=4, verbose=0)):
        with pytest.raises(NotImplementedError):
            call(D.MatchingAgent(), _stub_env(d=9, wide=True))                       # d = 9
        with pytest.raises(NotImplementedError):
            call(D.MatchingAgent(), _stub_env(wide=True))                            # the wide environment at d = 5
        with pytest.raises(NotImplementedError):
            call(D.MatchingAgent(), _stub_env(volume_depth=17))
        with pytest.raises(ValueError):
            call(D.MatchingAgent(evaluator=ev3), _stub_env())                        # an evaluator of another depth
        with pytest.raises(ValueError):
            call(D.MatchingAgent(evaluator=ev5), _stub_env(use_Y=True))              # ... of another use_Y
        with pytest.raises(ValueError):
            call(D.MatchingAgent(), _stub_env(error_model="XZ"))
        with pytest.raises(ValueError):
            D.MatchingAgent().test(_stub_env(), nb_episodes=4, verbose=0, nb_max_episode_steps=0)
    for rates, kw in (([], {}), ([0.01] * 2, {}), ([0.01, 1.5], {}), ([0.001 * k for k in range(1, 10)], {}), ([0.01, 0.02], dict(p_meas=[0.1]))):
        with pytest.raises(ValueError):
            D.MatchingAgent().test_error_rates(_stub_env(), rates, nb_episodes=4, verbose=0, **kw)
    with pytest.raises(ValueError):
        D.MatchingAgent(policy="greedy")
    with pytest.raises(ValueError):
        D.MatchingAgent(chunk=0)
    with pytest.raises(ValueError):
        D.MatchingAgent().test(None, verbose=0)
    # the wrapper on the environment: the same conventions
    env_mod = importlib.import_module("deepq-decoding_amd.env")
    e = object.__new__(env_mod.VectorEnv)
    e.d, e.error_model, e.use_Y, e.volume_depth, e.wide, e.n_envs = 9, "DP", False, 5, True, 4
    with pytest.raises(NotImplementedError):
        e.match_select(ev5)
    e.d, e.wide = 5, False
    with pytest.raises(ValueError):
        e.match_select(ev3)


def test_quota_blocks_and_step_cap():
    E = importlib.import_module("deepq-decoding_amd.episodes")
    assert E.share_quota(4, 10).tolist() == [3, 3, 2, 2] and E.share_quota(4, 2).tolist() == [1, 1, 0, 0]
    rates, m, ph, pm, quota = E.rate_blocks(7, [0.01, 0.02, 0.03], 3, p_meas=0.5)
    assert rates == [0.01, 0.02, 0.03] and m == 2 and ph.tolist() == [0.01, 0.01, 0.02, 0.02, 0.03, 0.03, 0.03] and (pm == 0.5).all()
    assert quota.tolist() == [2, 1, 2, 1, 2, 1, 0]
    rec = np.array([[0, 0, 0, 1, 5], [0, 3, 0, 1, 5], [1, 2, 0, 1, 5], [2, 6, 0, 1, 5]])
    assert E.block_records(rec, 1, 2)[:, 1].tolist() == [3, 2] and len(E.block_records(rec, 2, 2)) == 0
    assert E.check_step_cap(None, quota) == 2 * E.STEPS_PER_EPISODE_CAP and E.check_step_cap(7, quota) == 7
    assert E.check_step_cap(None, np.zeros(0, dtype=np.int64)) == E.STEPS_PER_EPISODE_CAP
    for bad in (0, -1, 1.5, True, "3"):
        with pytest.raises(ValueError):
            E.check_step_cap(bad, quota)


def test_match_select_abi_is_declared_and_bound():
    L = importlib.import_module("deepq-decoding_amd._lib")
    lib = L.lib()
    assert lib.dq_version() >= 7
    header = open(os.path.join(os.path.dirname(L.__file__), "..", "include", "deepq_hip.h")).read()
    assert "dq_env_match_select(" in header and hasattr(lib, "dq_env_match_select")
    assert L.SIGNATURES["dq_env_match_select"] == (ctypes.c_int, [ctypes.c_void_p] * 5)
    assert lib.dq_env_match_select(None, None, None, None, None) == -1            # DQ_ERR_INVALID on null handles, no device touched
    digest = importlib.import_module("deepq-decoding_amd._digest")
    import glob
    names = {os.path.basename(f) for f in glob.glob(os.path.join(digest.HERE, "csrc", "*"))}
    assert {"env_match.hip", "match_st_dev.h"} <= names                           # (the digest and the build list csrc/ by glob)
    assert lib.dq_build_digest().decode() == digest.csrc_digest()
