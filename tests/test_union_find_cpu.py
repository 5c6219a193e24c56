"""The union-find decoder, host side: tests/union_find_ref.py -- the numpy statement the device is compared with bit for bit in
tests/test_union_find_gpu.py -- checked on its own against match_st_ref.py's subset DPs and on hand cases; then the `method` argument's validation
before any library call, the C ABI and the plumbing of the method through MatchingAgent, the policies, DQNCore and decode_benchmark."""
import ctypes
import importlib
import os
import types

import numpy as np
import pytest

import match_st_ref as M
import union_find_ref as U

UF = "union_find"


def _planes(d, comp, mask):
    """The component's frame plane [1, d2] of a qubit mask, as hidden_state codes that Component.plane reads back."""
    q = np.arange(d * d)
    bits = (mask >> q) & 1
    return (bits * (1 if comp == 0 else 3)).astype(np.uint8)[None]


# ---- 1. every pattern of d = 3: a valid correction, never below the minimum ------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [1, 2])
def test_every_d3_pattern_is_a_valid_correction_no_lighter_than_the_minimum(depth):
    tight = total = 0
    for comp in (0, 1):
        C = M.Component(3, comp)
        n = C.n
        for pat in range(1 << (n * depth)):
            rows = np.array([(pat >> i) & 1 for i in range(n * depth)], dtype=np.int64).reshape(depth, n)
            mask, W, ndef, rounds = U.decode_component(3, comp, rows, depth)
            assert ndef == rows.sum() and (rounds == 0) == (ndef == 0)
            sig, cls = C.frame_syndrome_class(_planes(3, comp, mask))
            s_last = np.bitwise_xor.reduce(rows, axis=0)
            # some fault history no heavier than W reproduces the volume with the frame's class and last-round measurement errors
            assert M.dp_history(C, rows, sig[0] ^ s_last, int(cls[0]), depth) <= W, (comp, pat, W)
            w_min = M.dp_open(C, rows, depth)
            assert W >= w_min, (comp, pat, W, w_min)
            tight += W == w_min
            total += 1
    print(f"d = 3, depth {depth}: weight equals the minimum on {tight} of {total} patterns")
    assert total == 2 * (1 << (4 * depth))


# ---- 2. hand cases ------------------------------------------------------------------------------------------------------------------------------
def test_hand_cases():
    seen = set()
    for name, d, comp, depth, rows, want in U.hand_cases():
        mask, W, ndef, rounds = U.decode_component(d, comp, rows, depth)
        got = dict(M=mask, W=W, rounds=rounds)
        for key, v in want.items():
            assert got[key] == v, (name, key, got, want)
        assert ndef == rows.sum()
        C = M.Component(d, comp)
        if ndef <= 10:                                                              # (the subset DP of the checker is exponential in the defects)
            assert W >= M.dp_open(C, rows, depth), name
        # the frame closes the volume: its syndrome differs from the last round's by what measurement errors of the last round explain, at most W of them
        sig, _ = C.frame_syndrome_class(_planes(d, comp, mask))
        assert int((sig[0] ^ np.bitwise_xor.reduce(rows, axis=0)).sum()) <= W, name
        seen.add(name.split("_", 3)[3].split("_u")[0])
    assert seen == {"none", "lone", "time_pair", "space_pair", "central", "full_slice", "everything"}
    # the dense patterns: every node a defect -> every defect leaves by its time edge or pairs with a neighbour; no round beyond the first is needed
    mask, W, ndef, rounds = U.decode_component(7, 0, np.ones((16, 24), dtype=np.int64), 16)
    assert ndef == 384 and rounds == 1 and W == 192 and mask == 0


# ---- 3. sparse samples: almost always the minimum (printed, not barred) -------------------------------------------------------------------------------
def test_sparse_samples_mostly_reach_the_minimum():
    d, depth, n_vol, p = 5, 5, 300, 0.007
    rng = np.random.default_rng(20)
    equal = nonzero = 0
    for i in range(n_vol):
        comp = i & 1
        C = M.Component(d, comp)
        data = rng.random((depth, d * d)) < 2 * p / 3                               # depolarising: two of the three Paulis flip a component
        meas = rng.random((depth, C.n)) < p
        s = ((np.cumsum(data, axis=0) % 2) @ C.H) % 2 ^ meas
        rows = s.copy()
        rows[1:] ^= s[:-1]
        mask, W, ndef, rounds = U.decode_component(d, comp, rows, depth)
        w_min = M.dp_open(C, rows, depth)
        assert W >= w_min
        equal += W == w_min
        nonzero += ndef > 0
    print(f"d5 depth 5 p = {p}: union-find weight equals the minimum on {equal} of {n_vol} components ({nonzero} with defects)")
    assert nonzero > 20


# ---- 4. a function of the volume alone ----------------------------------------------------------------------------------------------------------------
def test_results_are_a_function_of_the_volume():
    rng = np.random.default_rng(4)
    for d, depth in ((5, 5), (7, 7)):
        C = M.Component(d, 0)
        rows = (rng.random((depth, C.n)) < 0.15).astype(np.int64)
        first = U.decode_component(d, 0, rows, depth)
        assert first == U.decode_component(d, 0, rows.copy(), depth) and first[2] > 0 and first[1] > 0
    vol = (rng.random((6, 5, 6, 6)) < 0.1).astype(np.uint8)
    a, b = U.decode(5, vol, 5), U.decode(5, vol[::-1], 5)
    assert all(np.array_equal(x, y[::-1]) for x, y in zip(a, b))


# ---- 5. validation before any library call -------------------------------------------------------------------------------------------------------------
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


def test_arguments_are_validated_before_the_library_is_touched(dq, monkeypatch):
    env_mod = _no_library(monkeypatch)
    D = dq.decoder
    ev5 = types.SimpleNamespace(d=5, error_model="DP", use_Y=False, volume_depth=5, _h=None)
    ev3 = types.SimpleNamespace(d=5, error_model="DP", use_Y=False, volume_depth=3, _h=None)
    stub = lambda **kw: types.SimpleNamespace(**dict(dict(d=5, error_model="DP", use_Y=False, volume_depth=5, wide=False, n_envs=8, identity_index=50,
                                                            p_phys=0.01, p_meas=0.01, seed=(1, 2)), **kw))
    vol = np.zeros((2, 5, 6, 6), dtype=np.uint8)
    assert D.METHODS == ("matching", "union_find")
    # a bad method, everywhere it is taken
    for bad in ("uf", "MATCHING", None, 1, ("matching",)):
        with pytest.raises(ValueError):
            D.matching_decode(vol, stub(), method=bad)
        with pytest.raises(ValueError):
            D.score_matching(stub(), 16, method=bad)
        with pytest.raises(ValueError):
            D.MatchingAgent(method=bad) if bad is not None else D.check_method(bad)
    e = object.__new__(env_mod.VectorEnv)

    def lattice(**kw):
        base = dict(d=5, error_model="DP", use_Y=False, volume_depth=5, wide=False, n_envs=4, num_actions=51)
        base.update(kw)
        for k, v in base.items():
            setattr(e, k, v)
        return e

    for bad in ("uf", None, 2):
        with pytest.raises(ValueError):
            lattice().match_select(ev5, method=bad)
        with pytest.raises(ValueError):
            lattice().guided_select(ev5, 0, method=bad)
    # the scope limits are the matching's: the same exceptions from the same validators
    for call in (lambda env, ev: env.match_select(ev, method=UF), lambda env, ev: env.guided_select(ev, 0, method=UF)):
        with pytest.raises(NotImplementedError):
            call(lattice(wide=True), ev5)
        with pytest.raises(NotImplementedError):
            call(lattice(d=9), types.SimpleNamespace(d=9, error_model="DP", use_Y=False, volume_depth=5, _h=None))
        with pytest.raises(NotImplementedError):
            call(lattice(volume_depth=17), types.SimpleNamespace(d=5, error_model="DP", use_Y=False, volume_depth=17, _h=None))
        with pytest.raises(ValueError):
            call(lattice(), ev3)                                                       # a foreign evaluator
    with pytest.raises(NotImplementedError):
        D.matching_decode(vol, stub(wide=True), method=UF)
    with pytest.raises(NotImplementedError):
        D.matching_decode(np.zeros((2, 5, 10, 10), dtype=np.uint8), stub(d=9), method=UF)
    with pytest.raises(NotImplementedError):
        D.score_matching(stub(wide=True), 16, method=UF)
    agent = D.MatchingAgent(method=UF)
    assert agent.method == UF and agent.policy == "matching" and D.MatchingAgent().method == "matching"
    with pytest.raises(NotImplementedError):
        agent.test(stub(wide=True))
    with pytest.raises(NotImplementedError):
        agent.test(stub(d=9, wide=True))
    with pytest.raises(NotImplementedError):
        agent.test_error_rates(stub(volume_depth=17), [0.01])
    with pytest.raises(NotImplementedError):
        agent.evaluator_for(stub(volume_depth=17))
    with pytest.raises(ValueError):
        D.MatchingAgent(evaluator=ev3, method=UF).evaluator_for(stub())
    assert D.MatchingAgent(evaluator=ev5, method=UF).evaluator_for(stub()) == (ev5, False)
    with pytest.raises(ValueError):
        D.MatchingAgent(policy="identity", method=UF)                                  # the identity policy plays no decoder
    with pytest.raises(ValueError):
        D.MatchingAgent(policy="identity", method="matching")
    with pytest.raises(ValueError):
        object.__new__(dq.DQNAgent).decode_benchmark(stub(), 16, baseline="mwpm")
    with pytest.raises(ValueError):
        object.__new__(dq.DQNAgent).decode_benchmark(stub(), 16, baseline=("matching", "uf"))
    with pytest.raises(ValueError):
        object.__new__(dq.DQNAgent).decode_benchmark(stub(), 16, baseline=())


# ---- 6. the C ABI ------------------------------------------------------------------------------------------------------------------------------------
def test_union_find_abi_is_declared_and_bound():
    L = importlib.import_module("deepq-decoding_amd._lib")
    lib = L.lib()
    assert lib.dq_version() == 8                                                       # new capability = the presence of the new symbols
    header = open(os.path.join(os.path.dirname(L.__file__), "..", "include", "deepq_hip.h")).read()
    vp, i, dbl = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    want = {"dq_decode_uf": (i, [vp, vp, i, vp, vp, vp, vp, vp]),
            "dq_env_uf_select": (i, [vp, vp, vp, vp]),
            "dq_env_guided_select_uf": (i, [vp, vp, vp, dbl, dbl, i, ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint64, vp, vp, vp, vp])}
    for name, sig in want.items():
        assert name + "(" in header and hasattr(lib, name) and L.SIGNATURES[name] == sig, name
    assert "int32_t* rounds_dev, void* stream);" in header and "not thread-safe" in header.split("dq_decode_uf:")[1].split("dq_status dq_decode_uf")[0]
    seed = (ctypes.c_uint32 * 2)(1, 2)
    assert lib.dq_decode_uf(None, None, 1, None, None, None, None, None) == -1          # DQ_ERR_INVALID on null handles, no device touched
    assert lib.dq_env_uf_select(None, None, None, None) == -1
    assert lib.dq_env_guided_select_uf(None, None, None, 0.5, 0.5, 0, seed, 0, None, None, None, None) == -1
    assert L.SIGNATURES["dq_decode_match"] == (i, [vp, vp, i, vp, vp, vp, vp, vp]) and L.SIGNATURES["dq_env_match_select"] == (i, [vp, vp, vp, vp, vp])
    digest = importlib.import_module("deepq-decoding_amd._digest")
    import glob
    names = {os.path.basename(f) for f in glob.glob(os.path.join(digest.HERE, "csrc", "*"))}
    assert {"uf_dev.h", "uf_st.hip"} <= names
    assert lib.dq_build_digest().decode() == digest.csrc_digest()


# ---- 7. plumbing ------------------------------------------------------------------------------------------------------------------------------------------
def test_match_result_keeps_its_four_positional_fields(dq):
    R = dq.decoder.MatchResult
    r = R(1, 2, 3, 4)
    assert (r.frame, r.weight, r.n_defects, r.inexact, r.rounds) == (1, 2, 3, 4, None)
    assert R(1, 2, 3, 4, 5).rounds == 5


def test_method_reaches_the_select_calls(dq, monkeypatch):
    import torch
    D = dq.decoder
    guide = D.MatchingAgent(method=UF)
    inner = dq.EpsGreedyQPolicy(masked_greedy=True, guide=guide, guide_share=0.25)
    outer = dq.LinearAnnealedPolicy(inner, attr="eps", value_max=1.0, value_min=0.0, value_test=0.0, nb_steps=100)
    assert inner.guide.method == UF and outer.guide is guide
    # MatchingAgent._records: the union-find form of match_select, no flag buffer involved
    calls = []

    class Venv:
        device, n_envs, identity_index, d, error_model, use_Y, volume_depth, L = "cpu", 4, 50, 5, "DP", False, 5, None
        done = was_reset = reward = lifetime = None

        def match_select(self, ev, out=None, out_inexact=None, method="matching"):
            calls.append(("select", method, out_inexact is not None))

        def step(self, action, auto_reset, write_obs):
            calls.append(("step",))

        def reset(self, write_obs):
            pass

        def _stream(self):
            return None

    episodes = importlib.import_module("deepq-decoding_amd.episodes")

    def fake_records(L, dev, stream, n, quota, step, *a):
        step(0)
        step(1)
        return np.zeros((0, 4))
    monkeypatch.setattr(episodes, "episode_records", fake_records)
    monkeypatch.setattr(torch.cuda, "device", lambda dev: __import__("contextlib").nullcontext())
    for method, want in ((UF, ("select", UF, False)), ("matching", ("select", "matching", True))):
        calls.clear()
        agent = D.MatchingAgent(evaluator=object(), method=method)
        rec, inexact = agent._records(Venv(), None, None)
        assert calls == [want, ("step",), want, ("step",)] and agent.last_vector_steps == 2 and not inexact.any()
    # DQNCore.guided_act_and_step hands the method to guided_select
    core_mod = importlib.import_module("deepq-decoding_amd.core")
    seen = {}
    ring = types.SimpleNamespace(cur=0, next_slot=lambda: 1, action=torch.zeros((2, 4), dtype=torch.int32), reward=torch.zeros((2, 4)),
                                 terminal=torch.zeros((2, 4), dtype=torch.uint8), store=torch.zeros((2, 4), dtype=torch.uint8), compact=False,
                                 advance=lambda: None)
    env = types.SimpleNamespace(guided_select=lambda ev, t, **kw: seen.update(kw), _launch=lambda *a: None, _h=None, legal=None, lifetime=None, was_reset=None)
    fake = types.SimpleNamespace(_wide=False, world_size=1, _flush_stats=lambda: None, ring=ring, env=env, N=4, params=None, params_pk=None, q_act=None,
                                 net=types.SimpleNamespace(forward_multi=lambda jobs: ["q"]), _obs_job=lambda **kw: None,
                                 _guide_flags=torch.zeros((2, 4), dtype=torch.uint8), guide_counts=torch.zeros(2, dtype=torch.int64),
                                 L=types.SimpleNamespace(dq_env_step=None), _stream=lambda: None, defer_stats=True, vector_steps=0, device="cpu")
    core_mod.DQNCore.guided_act_and_step(fake, "ev", 0.5, 0.25, method=UF)
    assert seen["method"] == UF and seen["eps"] == 0.5 and seen["guide_share"] == 0.25 and fake.vector_steps == 1
    core_mod.DQNCore.guided_act_and_step(fake, "ev", 0.5, 0.25)
    assert seen["method"] == "matching"


def test_decode_benchmark_rows(dq, monkeypatch):
    D = dq.decoder
    env = types.SimpleNamespace(d=5, error_model="DP", use_Y=False, volume_depth=5, wide=False, p_phys=0.01, p_meas=0.01, seed=(1, 2))
    dec = types.SimpleNamespace(evaluate=lambda *a, **k: "agent", _eval="handle")
    agent = object.__new__(dq.DQNAgent)
    agent.nb_actions, agent.model = 51, types.SimpleNamespace(input_shape=(7, 11, 11))
    agent._bind, agent._decoder_for, agent._core = (lambda e: None), (lambda *a: dec), types.SimpleNamespace(params=None)
    monkeypatch.setattr(D, "score_matching", lambda env, n, method="matching", evaluator=None, **kw: (method, n, evaluator))
    assert agent.decode_benchmark(env, 64) == "agent"
    assert agent.decode_benchmark(env, 64, baseline="matching") == ("agent", ("matching", 64, "handle"))
    assert agent.decode_benchmark(env, 64, baseline=UF) == ("agent", (UF, 64, "handle"))
    assert agent.decode_benchmark(env, 64, baseline=("matching", UF)) == ("agent", ("matching", 64, "handle"), (UF, 64, "handle"))
