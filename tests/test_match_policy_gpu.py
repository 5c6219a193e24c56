"""The matching decoder as a policy of the environment on the device (VectorEnv.match_select / decoder.MatchingAgent, csrc/env_match.hip; DESIGN.md
section 14).  The kernel's action must be the rule decoder.frame_to_actions states, applied to matching_decode's frame of the lattice's exported
volume, on every live lattice of every step; the frames a run applies pass tests/match_st_ref.py's certificate; the refactoring behind it moved
neither match_st_kernel nor DQNAgent.test (arrays recorded with the previous library); the evaluation surface keeps DQNAgent's layout."""
import numpy as np
import pytest

import match_st_ref as M
import shipped
from conftest import load_golden
from oracle import env_oracle, lattice

pytestmark = pytest.mark.gpu

SEED = (1234, 5678)
CONFIGS = {
    "a_d3_x_2": (dict(d=3, error_model="X", use_Y=False, volume_depth=2), 0.02),
    "b_d5_dp_5_y": (dict(d=5, error_model="DP", use_Y=True, volume_depth=5), 0.011),
    "b_d5_dp_5": (dict(d=5, error_model="DP", use_Y=False, volume_depth=5), 0.011),
    "c_d5_dp_9": (dict(d=5, error_model="DP", use_Y=False, volume_depth=9), 0.011),      # the 32-word record
    "d_d7_x_7": (dict(d=7, error_model="X", use_Y=False, volume_depth=7), 0.011),
}
N = 256


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return torch


def _env(dq, cfg, p, n=N, base=0, referee="lut"):
    return dq.VectorEnv(n_envs=n, p_phys=p, p_meas=p, seed=SEED, env_id_base=base, referee=referee, **cfg)


def _state(dq, env):
    """(volumes uint8 [N, depth, d+1, d+1], completed sets, done flags, lifetimes) of the lattices as they stand."""
    st = env.export_state().cpu().numpy().view(np.uint64)
    d, depth = env.d, env.volume_depth
    order = lattice.Masks(d).order
    vol = np.zeros((len(st), depth, d + 1, d + 1), dtype=np.uint8)
    for s, (a, b) in enumerate(order):
        vol[:, :, a, b] = ((st[:, 11:11 + depth] >> np.uint64(s)) & np.uint64(1)).astype(np.uint8)
    completed = [dq.decoder.completed_from_words(w0, w1) for w0, w1 in st[:, 6:8]]
    return vol, completed, ((st[:, 10] >> np.uint64(32)) & np.uint64(1)).astype(bool), (st[:, 10] & np.uint64(0xFFFFFFFF)).astype(np.int64)


# ---- 1. the action is the rule, on every live lattice of every step ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_action_equals_the_rule_on_every_live_lattice(dq, torch_mod, name):
    torch = torch_mod
    cfg, p = CONFIGS[name]
    D = dq.decoder
    d, model, use_Y, depth = cfg["d"], cfg["error_model"], cfg["use_Y"], cfg["volume_depth"]
    env = _env(dq, cfg, p)
    ev = D.Evaluator(d, model, use_Y, depth, chunk=N, device=env.device)
    identity, d2 = env.identity_index, d * d
    flag = torch.zeros(N, dtype=torch.uint8, device=env.device)
    env.reset()
    second = y_pairs = live_steps = dead_steps = nonzero = inexact_seen = 0
    try:
        for t in range(40):
            vol, completed, done, _ = _state(dq, env)
            res = D.matching_decode(vol, env, to_host=True, evaluator=ev)
            act = env.match_select(ev, out_inexact=flag)
            got, got_flag = act.cpu().numpy(), flag.cpu().numpy()
            for i in range(N):
                if done[i]:
                    assert got[i] == identity and got_flag[i] == 0, (name, t, i)
                    dead_steps += 1
                    continue
                wanted, a = D.frame_to_actions(res.frame[i], completed[i], d, model, use_Y)
                assert got[i] == a, (name, t, i, wanted, sorted(completed[i]), int(got[i]))
                assert got_flag[i] == res.inexact[i], (name, t, i)
                assert completed[i] <= set(wanted), (name, t, i)                  # what the policy did earlier on this volume belongs to its frame
                live_steps += 1
                nonzero += a != identity
                second += a != identity and len(completed[i]) > 0
                y_pairs += (model == "DP" and not use_Y and d2 <= a < 2 * d2 and (a - d2) in completed[i] and res.frame[i].reshape(-1)[a - d2] == 2)
                inexact_seen += int(res.inexact[i])
            env.step(act, auto_reset=True)
    finally:
        ev.close()
    print(name, dict(live=live_steps, dead=dead_steps, flips=int(nonzero), second_flips=int(second), y_pairs=int(y_pairs), inexact=inexact_seen))
    assert live_steps > 30 * N and second > 0
    if d <= 5:                                                              # (lattices die within the run: the done branch took part)
        assert dead_steps > 0
    if name == "b_d5_dp_5":
        assert y_pairs > 0


# ---- 2. the frames a run applies pass the certificate ------------------------------------------------------------------------------------------------
def test_applied_frames_pass_the_certificate(dq, torch_mod):
    cfg, p = CONFIGS["a_d3_x_2"]
    D = dq.decoder
    d, depth = cfg["d"], cfg["volume_depth"]
    env = _env(dq, cfg, p)
    ev = D.Evaluator(d, "X", False, depth, chunk=N, device=env.device)
    identity = env.identity_index
    env.reset()
    held = [None] * N                                                        # per lattice: (volume, weight, X plane so far) of the volume in progress
    checked = flips = 0
    try:
        for t in range(24):
            vol, completed, done, _ = _state(dq, env)
            res = D.matching_decode(vol, env, to_host=True, evaluator=ev)
            act = env.match_select(ev).cpu().numpy()
            for i in range(N):
                if done[i]:
                    held[i] = None
                    continue
                if not completed[i]:                                         # a new volume (completed_actions is cleared with it)
                    held[i] = [vol[i].copy(), int(res.weight[i, 0]), np.zeros((d, d), dtype=np.int64)]
                assert held[i] is not None and np.array_equal(held[i][0], vol[i])        # the volume stays until the identity
                if act[i] != identity:
                    held[i][2] ^= (env_oracle.index_to_move(d, int(act[i]), "X", False) == 1).astype(np.int64)
                    flips += 1
                else:                                                        # the volume is finished: the XOR of the actions between two identities
                    ok, w_min, hist = M.certify(d, 0, held[i][0], held[i][2], held[i][1], depth)
                    assert ok, (t, i, held[i][1], w_min, hist)
                    checked += 1
                    held[i] = None
            env.step(torch_mod.from_numpy(act).to(env.device), auto_reset=True)
    finally:
        ev.close()
    print("certified volumes", checked, "flips", flips)
    assert checked > 8 * N and flips > N


# ---- 3. / 6. the refactoring moved neither match_st_kernel nor the agent's evaluation -----------------------------------------------------------------
def test_match_st_kernel_is_unchanged(dq, torch_mod):
    """matching_decode against arrays recorded with the library of the commit before mst_component moved into match_st_dev.h (1024 sample_volumes
    volumes of configuration (b); at p = 0.06 the 14 / 32 fallback paths take part)."""
    g = load_golden("match_st_d5_dp_before_policy")
    D = dq.decoder
    for tag, p in (("p011", 0.011), ("p06", 0.06)):
        env = dq.VectorEnv(n_envs=1, p_phys=p, p_meas=p, seed=SEED, referee=None, d=5, error_model="DP", use_Y=True, volume_depth=5)
        vol, hid, triv = D.sample_volumes(env, 1024, seed=SEED, env_id_base=9, to_host=True)
        res = D.matching_decode(vol, env, to_host=True)
        for key in ("frame", "weight", "n_defects", "inexact"):
            assert np.array_equal(getattr(res, key), g[f"{tag}_{key}"]), (tag, key)
    assert g["p06_inexact"].sum() > 0 and g["p011_frame"].any()


def _shipped_agent(dq, env, family, p):
    weights, _ = shipped.shipped_weights(family, p)
    model = dq.build_convolutional_nn(shipped.C_LAYERS, shipped.FF_LAYERS, env.observation_space.shape, env.num_actions)
    agent = dq.DQNAgent(model=model, nb_actions=env.num_actions, memory=dq.SequentialMemory(limit=1000, window_length=1), nb_steps_warmup=100,
                        target_model_update=100, policy=dq.GreedyQPolicy(masked_greedy=True), test_policy=dq.GreedyQPolicy(masked_greedy=True),
                        gamma=0.99, enable_dueling_network=True)
    agent.compile(dq.Adam(lr=1e-4))
    agent._bind(env)
    agent.model.set_weights(weights)
    return agent


def test_shared_loop_did_not_move_the_agent(dq, torch_mod):
    """DQNAgent.test of the shipped d5_x 0.007 weights at p = 0.011, 64 episodes on 16 lattices, against the History recorded with the tree and
    library of the commit before the loop was shared."""
    g = load_golden("agent_test_d5_x_0.007_at_0.011_before_policy")
    env = dq.VectorEnv(n_envs=16, p_phys=0.011, p_meas=0.011, seed=SEED, referee="lut", **shipped.CONFIGS["d5_x"])
    h = _shipped_agent(dq, env, "d5_x", "0.007").test(env, nb_episodes=64, visualize=False, verbose=0)
    assert sorted(h.history) == sorted(g.files)
    for key in g.files:
        assert np.array_equal(np.asarray(h.history[key], dtype=np.float64), g[key]), key
    assert len(h.history["episode_lifetime"]) == 64


# ---- 4. / 5. the evaluation surface ----------------------------------------------------------------------------------------------------------------------
def test_results_depend_on_global_ids_only(dq, torch_mod):
    E = __import__("importlib").import_module("deepq-decoding_amd.episodes")
    cfg, p = CONFIGS["b_d5_dp_5"]
    agent = dq.decoder.MatchingAgent()
    whole = _env(dq, cfg, p, n=64)
    rec, inexact = agent._records(whole, E.share_quota(64, 128), None)
    h = agent.test(_env(dq, cfg, p, n=64), nb_episodes=128, verbose=0)
    parts = []
    for base in (0, 32):
        r, _ = agent._records(_env(dq, cfg, p, n=32, base=base), E.share_quota(32, 64), None)
        r = r.copy()
        r[:, 1] += base
        parts.append(r)
    both = np.concatenate(parts)
    both = both[np.lexsort((both[:, 1], both[:, 0]))]
    assert len(rec) == 128 and np.array_equal(rec, both)
    assert h.history == dq.DQNAgent._history_from_records(both, False, 100).history
    assert sorted(h.history) == ["episode_lifetime", "episode_lifetimes_rolling_avg", "episode_reward", "nb_steps"]
    assert agent.last_vector_steps > 0 and agent.last_inexact_steps == int(inexact.sum())


def test_error_rate_sweep_equals_separate_test_runs(dq, torch_mod):
    cfg, _ = CONFIGS["b_d5_dp_5"]
    rates, m, nb = [0.004, 0.012, 0.03], 32, 40
    env = _env(dq, cfg, 0.02, n=3 * m + 2, base=40)                       # (two idle lattices beyond the blocks: m = N // K stays 32)
    agent = dq.decoder.MatchingAgent()
    res = agent.test_error_rates(env, rates, nb_episodes=nb, verbose=0)
    assert list(res) == rates and env.p_phys == 0.02 and env.p_meas == 0.02      # previous rates restored
    assert sorted(agent.last_inexact_by_rate) == rates and sum(agent.last_inexact_by_rate.values()) == agent.last_inexact_steps
    for k, p in enumerate(rates):
        sub = _env(dq, cfg, p, n=m, base=40 + k * m)
        h = dq.decoder.MatchingAgent().test(sub, nb_episodes=nb, verbose=0)
        assert h.history == res[p].history, (k, p)
        assert len(h.history["episode_lifetime"]) == nb
    means = [np.mean(res[p].history["episode_lifetime"]) for p in rates]
    assert means[0] > means[-1], means


# ---- 7. ordering: a condition, not a tolerance -----------------------------------------------------------------------------------------------------------
def test_matching_outlives_the_identity_policy(dq, torch_mod):
    """d5_dp at p = 0.007, 512 lattices with one episode each, the same ids and seed for every policy: matching's mean lifetime must exceed the
    identity-only policy's (per volume it fails on 0.093 against 0.583 of 2^20 volumes).  The shipped agent's mean is
    printed beside them and not judged."""
    cfg, p, n = shipped.CONFIGS["d5_dp"], 0.007, 512
    D = dq.decoder
    mean = lambda h: float(np.mean(h.history["episode_lifetime"]))
    matching = D.MatchingAgent()
    m = mean(matching.test(_env(dq, cfg, p, n=n), nb_episodes=n, verbose=0))
    inexact, steps = matching.last_inexact_steps, matching.last_vector_steps
    ident = mean(D.MatchingAgent(policy="identity").test(_env(dq, cfg, p, n=n), nb_episodes=n, verbose=0))
    env = _env(dq, cfg, p, n=n)
    agent = mean(_shipped_agent(dq, env, "d5_dp", "0.007").test(env, nb_episodes=n, visualize=False, verbose=0))
    print(f"d5_dp p = {p}, {n} episodes: mean lifetime matching {m:.2f} (inexact steps {inexact}, vector steps {steps}), identity only {ident:.2f}, "
          f"shipped agent {agent:.2f}, 1 / p = {1 / p:.1f}")
    assert m > ident, (m, ident)


# ---- 8. the step cap ---------------------------------------------------------------------------------------------------------------------------------------
def test_step_cap_raises(dq, torch_mod):
    cfg, _ = CONFIGS["b_d5_dp_5"]
    env = _env(dq, cfg, 0.001, n=8)
    with pytest.raises(RuntimeError, match="cap of 1 vector steps"):
        dq.decoder.MatchingAgent().test(env, nb_episodes=8, verbose=0, nb_max_episode_steps=1)
    with pytest.raises(RuntimeError, match="cap of 3 vector steps"):
        dq.decoder.MatchingAgent().test_error_rates(env, [0.001, 0.002], nb_episodes=4, verbose=0, nb_max_episode_steps=3)
    assert env.p_phys == 0.001                                               # the rates are restored on the way out of a raised sweep too
