"""GPU tests of the device loop and the keras-rl-compatible agent surface."""
import importlib
import json
import os
import pickle

import numpy as np
import pytest

from oracle import c_oracle, dqn_oracle as O, philox

pytestmark = pytest.mark.gpu

C_LAYERS, FF_LAYERS = [[64, 3, 2], [32, 2, 1], [32, 2, 1]], [[512, 0.2]]
C1 = dict(d=3, error_model="X", use_Y=False, volume_depth=3, p_phys=0.005, p_meas=0.005)
C3 = dict(d=5, error_model="DP", use_Y=False, volume_depth=5, p_phys=0.011, p_meas=0.011)


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


C5 = dict(d=7, error_model="DP", use_Y=False, volume_depth=7, p_phys=0.005, p_meas=0.005)
C2 = dict(d=5, error_model="X", use_Y=False, volume_depth=5, p_phys=0.007, p_meas=0.007)


# beside BASELINE.json's configurations: Y moves (use_Y=True: three action planes, 76 actions at d = 5 -- a 128-bit legal-move mask and the wider Dense(|A|) tiling),
# the IIDXZ error model through the whole loop, and X noise at d = 7
C3Y = dict(d=5, error_model="DP", use_Y=True, volume_depth=5, p_phys=0.011, p_meas=0.011)
CXZ = dict(d=5, error_model="IIDXZ", use_Y=False, volume_depth=5, p_phys=0.008, p_meas=0.008)
C7X = dict(d=7, error_model="X", use_Y=False, volume_depth=7, p_phys=0.006, p_meas=0.006)


@pytest.mark.parametrize("name,C1,N,B,steps", [("c1", C1, 16, 8, 13), ("c3", C3, 64, 32, 12), ("c5", C5, 32, 16, 11), ("c2", C2, 48, 40, 11),
                                               ("c3y", C3Y, 40, 24, 11), ("iidxz", CXZ, 40, 24, 11), ("d7x", C7X, 24, 16, 10)],
                         ids=["c1", "c3", "c5", "c2", "c3y", "iidxz", "d7x"])
def test_device_loop_matches_oracle_loop(dq, torch_mod, name, C1, N, B, steps):
    """The whole loop -- Q forward, epsilon-greedy over legal moves, environment step into the ring, replay sampling,
    double-DQN update, Adam -- against the same loop assembled from the CPU oracles (C environment oracle, float64 network oracle,
    keras-rl memory oracle for the validity of the sampled rows), for several vector steps incl. the ring wrapping around, at every
    BASELINE.json lattice configuration.  Actions / observations / rewards must be identical; parameters agree to fp32 round-off."""
    torch = torch_mod
    from oracle import memory_oracle as M
    eps, gamma, lr = 0.3, 0.99, 1e-3
    seed = (0x5EED, 0xD0DEC0DE)
    env = dq.VectorEnv(n_envs=N, seed=seed, **C1)
    net = dq.QNetwork(env.obs_shape, C_LAYERS, FF_LAYERS, env.num_actions, max_batch=max(N, B))
    core = dq.DQNCore(env, net, batch_size=B, memory_limit=N * 8, gamma=gamma, lr=lr, seed=seed)
    spec = O.QNetSpec(env.obs_shape, C_LAYERS, FF_LAYERS, env.num_actions)
    p = core.params.cpu().numpy().astype(np.float64)
    assert np.array_equal(core.params.cpu().numpy(), O.glorot_init(spec, seed))
    p_t = p.copy()
    m, v = np.zeros_like(p), np.zeros_like(p)
    ref = c_oracle.COracleEnv(n_envs=N, seed=seed, **C1)
    T = core.T
    ring_obs = np.zeros((T, N) + env.obs_shape, np.uint8)
    ring_a, ring_r, ring_t = np.zeros((T, N), np.int32), np.zeros((T, N), np.float32), np.zeros((T, N), np.uint8)
    core.reset_env()
    ref.reset()
    cur, filled, n_updates = 0, 1, 0
    ring_obs[0] = ref.obs
    for t in range(steps):
        # --- act (+ update): the three ways of driving the device loop give the same draws and the same arithmetic
        will_update = min(T, filled + 1) >= 4                    # keras-rl: nb_entries >= window_length + 2
        fused = will_update and t % 3 == 2                       # acting forward + the update's forwards in one pair of launches
        if fused:
            core.step_and_update(eps, presample_next=(t % 2 == 0))
        else:
            core.act_and_step(eps, presample=(t % 2 == 0))          # the sampling rides on the env launch every other step
        q, _ = O.forward(spec, p, ring_obs[cur])
        acts = np.zeros(N, np.int32)
        for i in range(N):
            w = philox.philox4x32((t, 0, i, philox.STREAM_POLICY << 16), seed)
            mask = int(ref.legal[i, 0]) | (int(ref.legal[i, 1]) << 64)
            acts[i] = O.select_action(q[i], mask, eps, False, w)
        assert np.array_equal(core.action_ring[cur].cpu().numpy(), acts), ("actions", t)
        ref.step(acts, auto_reset=True)
        nxt = (cur + 1) % T
        ring_a[cur], ring_r[cur], ring_t[cur], ring_obs[nxt] = acts, ref.reward, ref.done, ref.obs
        assert np.array_equal(core.obs_ring[nxt].cpu().numpy(), ref.obs), ("obs", t)
        assert np.array_equal(core.reward_ring[cur].cpu().numpy(), ref.reward) and np.array_equal(core.terminal_ring[cur].cpu().numpy(), ref.done)
        cur, filled = nxt, min(T, filled + 1)
        # --- update
        if not will_update:
            continue
        if not fused:
            core.update()
        n_updates += 1
        u = n_updates
        assert core.updates == u
        idx = core.index.cpu().numpy()
        # replay rows follow the device sampler's definition (first draws: a keyed permutation of the candidate rows, redraws: Philox)
        assert np.array_equal(idx, M.device_replay_rows(ring_t, N, T, cur, filled, B, seed, u))
        assert set(idx.tolist()) <= M.valid_transitions(ring_t, N, T, cur, filled)   # rows keras-rl's sample() can return
        rows = T * N
        flat_obs = ring_obs.reshape(rows, *env.obs_shape)
        s0, s1 = flat_obs[idx], flat_obs[(idx + N) % rows]
        y = O.td_targets(O.forward(spec, p, s1)[0], O.forward(spec, p_t, s1)[0], ring_r.reshape(-1)[idx], ring_t.reshape(-1)[idx], gamma)
        keep = O.dropout_keep_mask(seed, u, np.arange(B), 512, 0.2)
        q0, cache = O.forward(spec, p, s0, training=True, keep_masks=[keep])
        loss, mean_q, dq_ = O.loss_and_grad(q0, ring_a.reshape(-1)[idx], y)
        g = O.backward(spec, p, cache, dq_)
        p, m, v = O.adam_step(p, g, m, v, u, lr)
        met = np.array(core.read_metrics())
        assert abs(met[0] - loss) < 1e-5 and abs(met[1] - mean_q) < 1e-5, (met, loss, mean_q)
        assert np.abs(core.grads.cpu().numpy() - g).max() < 1e-5 * max(1.0, np.abs(g).max())
        big = np.abs(g) > 1e-6
        assert np.abs(core.params.cpu().numpy() - p)[big].max() < 5e-6
        if u % 3 == 0:
            core.update_target_hard()
            p_t = p.copy()
        # keep the oracle's weights glued to the device's fp32 values so round-off cannot accumulate into an action flip
        p = core.params.cpu().numpy().astype(np.float64)
        m, v = core.m.cpu().numpy().astype(np.float64), core.v.cpu().numpy().astype(np.float64)
        if u % 3 == 0:
            p_t = p.copy()


def test_device_loop_with_three_updates_per_vector_step(dq, torch_mod):
    """updates_per_vector_step = 3 (the knob that restores the reference's replay ratio: one minibatch per ENVIRONMENT step in keras-rl,
    TRAIN:119-127, is N minibatches per vector step of N lattices): per vector step one acting step and three double-DQN updates on the
    same ring state, update numbers u, u + 1, u + 2 -- against the same sequence assembled from the oracles."""
    torch = torch_mod
    from oracle import memory_oracle as M
    cfg, N, B, steps, k = C3, 48, 32, 9, 3
    eps, gamma, lr = 0.3, 0.99, 1e-3
    seed = (0x5EED, 0xD0DEC0DE)
    env = dq.VectorEnv(n_envs=N, seed=seed, **cfg)
    net = dq.QNetwork(env.obs_shape, C_LAYERS, FF_LAYERS, env.num_actions, max_batch=max(N, B))
    core = dq.DQNCore(env, net, batch_size=B, memory_limit=N * 8, gamma=gamma, lr=lr, seed=seed)
    spec = O.QNetSpec(env.obs_shape, C_LAYERS, FF_LAYERS, env.num_actions)
    p = core.params.cpu().numpy().astype(np.float64)
    p_t = p.copy()
    m, v = np.zeros_like(p), np.zeros_like(p)
    ref = c_oracle.COracleEnv(n_envs=N, seed=seed, **cfg)
    T = core.T
    ring_obs = np.zeros((T, N) + env.obs_shape, np.uint8)
    ring_a, ring_r, ring_t = np.zeros((T, N), np.int32), np.zeros((T, N), np.float32), np.zeros((T, N), np.uint8)
    core.reset_env()
    ref.reset()
    cur, filled, u = 0, 1, 0
    ring_obs[0] = ref.obs
    for t in range(steps):
        will_update = min(T, filled + 1) >= 4
        # the parameters the acting forward sees: those before this step's updates
        q, _ = O.forward(spec, p, ring_obs[cur])
        if will_update and t % 2 == 0:
            core.step_and_update(eps, extra_updates=k - 1)
            seq = None                                               # (all three updates already ran)
        else:
            core.act_and_step(eps, presample=will_update)
            seq = k if will_update else 0
        acts = np.zeros(N, np.int32)
        for i in range(N):
            w = philox.philox4x32((t, 0, i, philox.STREAM_POLICY << 16), seed)
            acts[i] = O.select_action(q[i], int(ref.legal[i, 0]) | (int(ref.legal[i, 1]) << 64), eps, False, w)
        assert np.array_equal(core.action_ring[cur].cpu().numpy(), acts), ("actions", t)
        ref.step(acts, auto_reset=True)
        nxt = (cur + 1) % T
        ring_a[cur], ring_r[cur], ring_t[cur], ring_obs[nxt] = acts, ref.reward, ref.done, ref.obs
        assert np.array_equal(core.obs_ring[nxt].cpu().numpy(), ref.obs), ("obs", t)
        cur, filled = nxt, min(T, filled + 1)
        if not will_update:
            continue
        rows = T * N
        flat_obs = ring_obs.reshape(rows, *env.obs_shape)
        for j in range(k):
            if seq:
                core.update()
            u += 1
            idx = M.device_replay_rows(ring_t, N, T, cur, filled, B, seed, u)
            s0, s1 = flat_obs[idx], flat_obs[(idx + N) % rows]
            y = O.td_targets(O.forward(spec, p, s1)[0], O.forward(spec, p_t, s1)[0], ring_r.reshape(-1)[idx], ring_t.reshape(-1)[idx], gamma)
            keep = O.dropout_keep_mask(seed, u, np.arange(B), 512, 0.2)
            q0, cache = O.forward(spec, p, s0, training=True, keep_masks=[keep])
            loss, mean_q, dq_ = O.loss_and_grad(q0, ring_a.reshape(-1)[idx], y)
            g = O.backward(spec, p, cache, dq_)
            p, m, v = O.adam_step(p, g, m, v, u, lr)
            if seq:                                                  # update by update: glue the oracle to the device's fp32 state
                assert np.array_equal(core.index.cpu().numpy(), idx)
                met = np.array(core.read_metrics())
                assert abs(met[0] - loss) < 1e-5 and abs(met[1] - mean_q) < 1e-5
                p = core.params.cpu().numpy().astype(np.float64)
                m, v = core.m.cpu().numpy().astype(np.float64), core.v.cpu().numpy().astype(np.float64)
        assert core.updates == u
        assert np.array_equal(core.last_index.cpu().numpy(), idx)   # the last update's rows (extra updates beyond the first read a row of ONE multi-update draw)
        met = np.array(core.read_metrics())
        assert abs(met[0] - loss) < 2e-5 and abs(met[1] - mean_q) < 2e-5, (met, loss, mean_q)
        big = np.abs(g) > 1e-6
        assert np.abs(core.params.cpu().numpy() - p)[big].max() < 2e-5     # three updates' round-off (Adam)
        p = core.params.cpu().numpy().astype(np.float64)
        m, v = core.m.cpu().numpy().astype(np.float64), core.v.cpu().numpy().astype(np.float64)


@pytest.mark.gpu
def test_extra_updates_in_pairs_and_on_the_side_stream_change_no_bit(dq, torch_mod):
    """The extra updates of a vector step in their three orders -- three forwards per launch pair (the plain order), in PAIRS (DQNCore.pair_targets, the
    default: the second update's target forward rides on the first one's launch pair), and with the target forwards on a second stream
    (DQNCore.target_ahead: a second network handle, one event per update) --: the same parameters, optimizer state and last minibatch, bit for bit, at the
    headline's per-GPU shape in small (256 lattices, minibatch 256, five and four updates per vector step, a hard target copy in between)."""
    torch = torch_mod
    seed = (0xA11CE, 0xB0B)
    out = []
    for pairs, ahead in ((False, False), (True, False), (False, True)):
        env = dq.VectorEnv(n_envs=256, seed=seed, **C3)
        net = dq.QNetwork(env.obs_shape, C_LAYERS, FF_LAYERS, env.num_actions, max_batch=256)
        core = dq.DQNCore(env, net, batch_size=256, memory_limit=256 * 16, lr=1e-3, seed=seed)
        core.pair_targets, core.target_ahead = pairs, ahead
        core.reset_env()
        for _ in range(4):
            core.act_and_step(1.0)
        for t in range(6):
            core.step_and_update(0.3, extra_updates=4 if t & 1 else 3)      # (three extra updates beyond the first: a pair and a single)
            if t == 2:
                core.update_target_hard()
        torch.cuda.synchronize()
        assert (core._side is not None) == ahead and (core._q1_pair is not None) == pairs
        out.append([x.cpu().numpy().copy() for x in (core.params, core.m, core.v, core.last_index)] + [core.read_metrics(), core.updates])
    for other in out[1:]:
        for a, b in zip(out[0][:4], other[:4]):
            assert np.array_equal(a, b)
        assert out[0][4] == other[4] and out[0][5] == other[5] == 27


class _PyVecEnv:
    """N independent oracle lattices (oracle/env_oracle.py, any d) behind the batched C-oracle's interface: the CPU side of the d >= 9 loop."""

    def __init__(self, n_envs, seed, **cfg):
        from oracle import env_oracle, matching_referee
        ref = matching_referee.MatchingReferee(cfg["d"], cfg["error_model"])
        self.envs = [env_oracle.OracleEnv(referee=ref, seed=seed, env_id=i, **cfg) for i in range(n_envs)]
        self.obs = np.zeros((n_envs,) + self.envs[0].board_state.shape, np.uint8)
        self.reward, self.done = np.zeros(n_envs, np.float32), np.zeros(n_envs, np.uint8)

    def _pull(self):
        for i, e in enumerate(self.envs):
            self.obs[i], self.done[i] = e.board_state, e.done

    def reset(self):
        for e in self.envs:
            e.reset()
        self._pull()

    def legal_mask(self, i):
        return self.envs[i].legal

    def step(self, acts, auto_reset=True):
        for i, e in enumerate(self.envs):
            if auto_reset and e.done:
                e.reset()
                self.reward[i] = 0.0
            else:
                self.reward[i] = e.step(int(acts[i]))[1]
        self._pull()


def test_device_loop_at_distance_nine_matches_oracle_loop(dq, torch_mod):
    """The loop of test_device_loop_matches_oracle_loop on a lattice beyond one 64-bit word per plane (d = 9: 81 qubits, 163 actions,
    19 x 19 observations): wide environment with the matching referee inside the step (csrc/env_big.hip), wide action selection, the
    Q-network on whichever path covers the architecture -- against the Python environment oracle + float64 network oracle."""
    cfg = dict(d=9, error_model="DP", use_Y=False, volume_depth=3, p_phys=0.006, p_meas=0.006)
    N, B, steps, eps, gamma, lr = 6, 4, 9, 0.4, 0.99, 1e-3
    seed = (0x5EED, 0xD0DEC0DE)
    env = dq.VectorEnv(n_envs=N, seed=seed, **cfg)
    assert env.wide and env.legal_words == 3 and env.obs_shape == (5, 19, 19)
    net = dq.QNetwork(env.obs_shape, C_LAYERS, FF_LAYERS, env.num_actions, max_batch=max(N, B))
    core = dq.DQNCore(env, net, batch_size=B, memory_limit=N * 6, gamma=gamma, lr=lr, seed=seed)
    spec = O.QNetSpec(env.obs_shape, C_LAYERS, FF_LAYERS, env.num_actions)
    p = core.params.cpu().numpy().astype(np.float64)
    p_t = p.copy()
    m, v = np.zeros_like(p), np.zeros_like(p)
    ref = _PyVecEnv(N, seed, **cfg)
    T = core.T
    ring_obs = np.zeros((T, N) + env.obs_shape, np.uint8)
    ring_a, ring_r, ring_t = np.zeros((T, N), np.int32), np.zeros((T, N), np.float32), np.zeros((T, N), np.uint8)
    core.reset_env()
    ref.reset()
    cur, filled, n_updates = 0, 1, 0
    ring_obs[0] = ref.obs
    assert np.array_equal(core.obs_ring[0].cpu().numpy(), ref.obs)
    for t in range(steps):
        will_update = min(T, filled + 1) >= 4
        fused = will_update and t % 2 == 0
        if fused:
            core.step_and_update(eps)
        else:
            core.act_and_step(eps, presample=True)
        q, _ = O.forward(spec, p, ring_obs[cur])
        acts = np.zeros(N, np.int32)
        for i in range(N):
            w = philox.philox4x32((t, 0, i, philox.STREAM_POLICY << 16), seed)
            acts[i] = O.select_action(q[i], ref.legal_mask(i), eps, False, w)
        assert np.array_equal(core.action_ring[cur].cpu().numpy(), acts), ("actions", t)
        ref.step(acts, auto_reset=True)
        nxt = (cur + 1) % T
        ring_a[cur], ring_r[cur], ring_t[cur], ring_obs[nxt] = acts, ref.reward, ref.done, ref.obs
        assert np.array_equal(core.obs_ring[nxt].cpu().numpy(), ref.obs), ("obs", t)
        assert np.array_equal(core.reward_ring[cur].cpu().numpy(), ref.reward) and np.array_equal(core.terminal_ring[cur].cpu().numpy(), ref.done)
        cur, filled = nxt, min(T, filled + 1)
        if not will_update:
            continue
        if not fused:
            core.update()
        n_updates += 1
        u = n_updates
        idx = core.index.cpu().numpy()
        rows = T * N
        flat_obs = ring_obs.reshape(rows, *env.obs_shape)
        s0, s1 = flat_obs[idx], flat_obs[(idx + N) % rows]
        y = O.td_targets(O.forward(spec, p, s1)[0], O.forward(spec, p_t, s1)[0], ring_r.reshape(-1)[idx], ring_t.reshape(-1)[idx], gamma)
        keep = O.dropout_keep_mask(seed, u, np.arange(B), 512, 0.2)
        q0, cache = O.forward(spec, p, s0, training=True, keep_masks=[keep])
        loss, mean_q, dq_ = O.loss_and_grad(q0, ring_a.reshape(-1)[idx], y)
        g = O.backward(spec, p, cache, dq_)
        p, m, v = O.adam_step(p, g, m, v, u, lr)
        met = np.array(core.read_metrics())
        assert abs(met[0] - loss) < 1e-5 and abs(met[1] - mean_q) < 1e-5, (met, loss, mean_q)
        assert np.abs(core.grads.cpu().numpy() - g).max() < 1e-5 * max(1.0, np.abs(g).max())
        p = core.params.cpu().numpy().astype(np.float64)
        m, v = core.m.cpu().numpy().astype(np.float64), core.v.cpu().numpy().astype(np.float64)
    assert n_updates >= 5


def test_a_td_error_beyond_the_host_known_scale_switches_the_loop_to_the_measured_scale(dq, torch_mod, monkeypatch):
    """with default settings a TD error of ~1e6 (rewards poisoned) no longer ends the run -- the updates that met it are
    discarded whole, read_metrics() warns ONCE and switches DQNCore.auto_scale on for good (the gradient scale measured per minibatch carries any finite
    TD error: keras-rl's delta_clip = inf), after which updates on the same poisoned memory move the parameters, finite.  DQ_TD_AUTOSCALE=0 keeps
    the host-known scale: the same situation raises DQ_ERR_RANGE (tests/test_distributed_gpu.py covers that path under two ranks and inside fit())."""
    torch = torch_mod
    import warnings
    monkeypatch.delenv("DQ_TD_AUTOSCALE", raising=False)
    N = 64
    env = dq.VectorEnv(n_envs=N, d=5, error_model="DP", use_Y=False, volume_depth=5, p_phys=0.011, p_meas=0.011)
    net = dq.QNetwork(env.obs_shape, [[64, 3, 2], [32, 2, 1], [32, 2, 1]], [[512, 0.2]], env.num_actions, max_batch=N)
    core = dq.DQNCore(env, net, batch_size=N, memory_limit=N * 8, gamma=0.99, lr=1e-3, seed=(5, 6))
    core.reset_env()
    for _ in range(4):
        core.act_and_step(1.0, use_q=False)
    for _ in range(3):
        core.step_and_update(0.5)
    core.read_metrics()
    assert core.auto_scale is False
    before = core.params.clone()
    core.reward_ring.fill_(1e6)
    core.step_and_update(0.5)
    torch.cuda.synchronize()
    assert torch.equal(core.params, before)                         # discarded whole
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        core.read_metrics()
    assert core.auto_scale is True and any("measures the gradient scale" in str(x.message) and "1 of the 1 updates" in str(x.message) for x in w)
    assert core.discarded_updates == 1                              # counted on the device (dq_qnet_range_discarded), logged in the warning
    core.reward_ring.fill_(1e6)                                     # (the step above wrote a fresh slot)
    for _ in range(3):
        core.step_and_update(0.5)
    loss, mean_q = core.read_metrics()                              # no warning, no error: carried
    assert bool(torch.isfinite(core.params).all()) and not torch.equal(core.params, before) and np.isfinite(loss)
    # the explicit switch keeps the error
    monkeypatch.setenv("DQ_TD_AUTOSCALE", "0")
    core2 = dq.DQNCore(env, net, batch_size=N, memory_limit=N * 8, gamma=0.99, lr=1e-3, seed=(5, 6))
    core2.reset_env()
    for _ in range(4):
        core2.act_and_step(1.0, use_q=False)
    core2.reward_ring.fill_(1e6)
    core2.step_and_update(0.5)
    with pytest.raises(dq.DeepQError) as ei:
        core2.read_metrics()
    assert ei.value.status == -6 and core2.auto_scale is False and core2.discarded_updates == 1


def _make_agent(dq, model_shape, n_actions, batch_size=32, warmup=64, target=200, limit=5000, seed=(1, 2)):
    model = dq.build_convolutional_nn(C_LAYERS, FF_LAYERS, model_shape, n_actions)
    memory = dq.SequentialMemory(limit=limit, window_length=1)
    policy = dq.LinearAnnealedPolicy(dq.EpsGreedyQPolicy(masked_greedy=False), attr="eps", value_max=1.0, value_min=0.02,
                                     value_test=0.0, nb_steps=2000)
    agent = dq.DQNAgent(model=model, nb_actions=n_actions, memory=memory, nb_steps_warmup=warmup, target_model_update=target,
                        policy=policy, test_policy=dq.GreedyQPolicy(masked_greedy=True), gamma=0.99, enable_dueling_network=True,
                        batch_size=batch_size, seed=seed)
    agent.compile(dq.Adam(lr=1e-4))
    return agent


def test_fit_and_test_single_lattice_facade(dq, torch_mod, tmp_path):
    """configs[0]: d=3 X p=0.005 batch=1 through the reference's reset()/step()/fit()/test() surface."""
    env = dq.Surface_Code_Environment_Multi_Decoding_Cycles(static_decoder=None, **C1)
    agent = _make_agent(dq, env.observation_space.shape, env.num_actions)
    log = dq.FileLogger(str(tmp_path / "training_history.json"), interval=10)
    hist = agent.fit(env, nb_steps=400, action_repetition=1, callbacks=[log], verbose=0, visualize=False, nb_max_start_steps=0,
                     start_step_policy=None, log_interval=50, nb_max_episode_steps=None, episode_averaging_length=20,
                     success_threshold=10000, stopping_patience=10000, min_nb_steps=100, single_cycle=False)
    h = hist.history
    for key in ("episode_reward", "nb_episode_steps", "nb_steps", "episode_lifetimes_rolling_avg", "best_rolling_avg", "best_episode",
                "time_since_best", "has_succeeded", "stopped_improving", "loss", "mean_q", "mean_eps", "duration", "episode"):
        assert key in h and len(h[key]) == len(h["episode"]) > 0, key
    assert agent.step >= 400 and np.isfinite([x for x in h["loss"] if x == x]).all()
    assert any(x == x for x in h["loss"]), "no update happened after warm-up"
    data = json.loads((tmp_path / "training_history.json").read_text())
    assert set(h) <= set(data) | {"episode"}
    # key order and value types of the reference's own files (trained_models/d5_dp/0.007/training_history.json)
    assert list(data) == ["loss", "mean_q", "mean_eps", "episode_reward", "nb_episode_steps", "nb_steps", "episode_lifetimes_rolling_avg",
                          "best_rolling_avg", "best_episode", "time_since_best", "has_succeeded", "stopped_improving", "episode", "duration"]
    for key, typ in (("episode_reward", float), ("nb_episode_steps", int), ("nb_steps", int), ("episode_lifetimes_rolling_avg", float),
                     ("best_rolling_avg", float), ("best_episode", int), ("time_since_best", int), ("has_succeeded", bool),
                     ("stopped_improving", bool), ("episode", int), ("duration", float)):
        assert all(type(v) is typ for v in data[key]), key
    assert data["episode"] == list(range(len(data["episode"])))
    # weights: save / load round trip through the reference's file name; memory pickles (TRAIN:156-160)
    w_before = agent.model.get_weights()
    wfile = str(tmp_path / "final_dqn_weights.h5f")
    agent.save_weights(wfile, overwrite=True)
    agent.model.set_weights([w * 0 for w in w_before])
    agent.model.load_weights(wfile)
    assert all(np.array_equal(a, b) for a, b in zip(w_before, agent.model.get_weights()))
    mem = pickle.loads(pickle.dumps(agent.memory))
    assert mem._saved is not None and mem._saved["filled"] == agent._core.filled
    # evaluation
    env.p_phys = env.p_meas = 0.003                                           # TRAIN:200-201
    core = agent._core
    before = (core.cur, core.filled, core.T, core.updates, core.obs_ring.clone(), core.action_ring.clone(), core.terminal_ring.clone())
    th = agent.test(env, nb_episodes=7, visualize=False, verbose=0, interval=10, single_cycle=False)
    # keras-rl stores nothing in test mode: the replay memory is exactly what training left
    assert (core.cur, core.filled, core.T, core.updates) == before[:4]
    assert all(bool((a == b).all()) for a, b in zip((core.obs_ring, core.action_ring, core.terminal_ring), before[4:]))
    assert len(th.history["episode_lifetime"]) == 7 and th.history["episode_lifetimes_rolling_avg"][-1] == np.mean(th.history["episode_lifetime"])
    assert all(l >= 3 and l % 3 == 0 for l in th.history["episode_lifetime"])     # lifetimes advance in volumes of depth 3
    a = agent.forward(env.reset())
    assert 0 <= a < env.num_actions and agent.compute_q_values(env.board_state).shape == (env.num_actions,)


def test_log_text_follows_the_readme(dq, torch_mod, capsys):
    """verbose=2 output of fit() / test() against the transcript in the reference's README.md:408-480,638-672: same lines, same
    labels, same number formats (values differ, so digits are masked)."""
    import re
    env = dq.Surface_Code_Environment_Multi_Decoding_Cycles(static_decoder=None, **C1)
    agent = _make_agent(dq, env.observation_space.shape, env.num_actions, warmup=20)
    agent.fit(env, nb_steps=150, action_repetition=1, callbacks=[], verbose=2, visualize=False, nb_max_start_steps=0, start_step_policy=None,
              log_interval=5, nb_max_episode_steps=None, episode_averaging_length=20, success_threshold=10000, stopping_patience=10000,
              min_nb_steps=100, single_cycle=False)
    out = capsys.readouterr().out.split("\n")
    assert out[0] == "Training for 150 steps ..."
    num, f3, f6 = r"\d+", r"\d+\.\d{3}", r"(nan|-?\d+\.\d{6})"
    block = [r"-----------------", r" {16}", rf"Episode: {num}", rf"Step: {num}/150", rf"This Episode Steps: {num}", r"This Episode Reward: \d+\.\d+",
             rf"This Episode Duration: {f3}s", rf"Rolling Lifetime length: {f3}", r"Best Lifetime Rolling Avg: \d+\.\d+", rf"Best Episode: {num}",
             rf"Time Since Best: {num}", r"Has Succeeded: False", r"Stopped Improving: False",
             rf"Metrics: loss: {f6}, mean_q: {f6}, mean_eps: {f6}", rf"Total Training Time: {f3}s", r""]
    n_blocks = 0
    i = 1
    while out[i] == "-----------------":
        for pat, line in zip(block, out[i:i + len(block)]):
            assert re.fullmatch(pat, line), (pat, line)
        i += len(block)
        n_blocks += 1
    assert n_blocks >= 2
    tail = out[i:]
    assert re.fullmatch(rf"Training Finished in {f3} seconds", tail[0]) and tail[1] == " " * 8
    assert re.fullmatch(r"Final Step: \d+", tail[2]) and tail[3] == "Succeeded: False" and tail[4] == "Stopped_Improving: False"
    assert re.fullmatch(rf"Final Episode Lifetimes Rolling Avg: {f3}", tail[5]) and tail[6:] == [""]
    agent.test(env, nb_episodes=3, visualize=False, verbose=2, interval=2, single_cycle=False)
    out = capsys.readouterr().out.split("\n")
    assert out[0] == "Testing for 3 episodes ..." and out[1] == "-----------------" and out[2] == "Episode: 1"
    assert re.fullmatch(r"This Episode Length: \d+", out[3]) and re.fullmatch(r"This Episode Reward: \d+\.\d", out[4])
    assert re.fullmatch(r"This Episode Lifetime: \d+", out[5]) and out[6] == "" and re.fullmatch(r"Episode Lifetimes Avg: \d+\.\d{3}", out[7])
    assert out[8] == "" and out[9] == "-----------------" and out[10] == "Episode: 3"


def test_fit_vector_env_is_deterministic(dq, torch_mod):
    """Two identical runs (same seeds) produce bit-identical weights: fixed-order reductions + counter RNG."""
    torch = torch_mod
    out = []
    for _ in range(2):
        env = dq.VectorEnv(n_envs=128, **C3)
        agent = _make_agent(dq, env.obs_shape, env.num_actions, batch_size=64, warmup=256, target=2048, limit=128 * 40)
        hist = agent.fit(env, nb_steps=128 * 40, verbose=0, episode_averaging_length=100, success_threshold=None, stopping_patience=None,
                         min_nb_steps=0, single_cycle=False, sync_interval=8)
        assert agent._core.updates >= 30 and len(hist.history["episode"]) >= 2
        out.append(agent._core.params.clone())
        th = agent.test(env, nb_episodes=200, visualize=False, verbose=0, single_cycle=False)
        assert len(th.history["episode_lifetime"]) == 200
    assert torch.equal(out[0], out[1])


def test_fit_and_test_at_distance_nine(dq, torch_mod):
    """DQNAgent.fit / test on 81-qubit lattices (wide environment, matching referee, 163 actions): runs, learns from its replay ring,
    and two identical runs give bit-identical weights."""
    torch = torch_mod
    cfg = dict(d=9, error_model="DP", use_Y=False, volume_depth=3, p_phys=0.003, p_meas=0.003)
    out = []
    for _ in range(2):
        env = dq.VectorEnv(n_envs=64, **cfg)
        agent = _make_agent(dq, env.obs_shape, env.num_actions, batch_size=32, warmup=128, target=512, limit=64 * 30)
        hist = agent.fit(env, nb_steps=64 * 30, verbose=0, episode_averaging_length=50, success_threshold=None, stopping_patience=None,
                         min_nb_steps=0, single_cycle=False, sync_interval=8)
        assert agent._core.updates >= 20 and len(hist.history["episode"]) >= 1
        out.append(agent._core.params.clone())
        th = agent.test(env, nb_episodes=64, visualize=False, verbose=0, single_cycle=False)
        assert len(th.history["episode_lifetime"]) == 64 and min(th.history["episode_lifetime"]) >= 3
    assert torch.equal(out[0], out[1]) and torch.isfinite(out[0]).all()


def test_early_stopping_rule(dq, torch_mod):
    env = dq.VectorEnv(n_envs=64, **C3)
    agent = _make_agent(dq, env.obs_shape, env.num_actions, batch_size=32, warmup=10 ** 9)
    hist = agent.fit(env, nb_steps=64 * 2000, verbose=0, episode_averaging_length=50, success_threshold=5.0, stopping_patience=None,
                     min_nb_steps=64 * 16, single_cycle=False, sync_interval=4)
    assert hist.history["has_succeeded"][-1] is True and agent.step < 64 * 2000


ALL_SHIPPED = [("d5_x", p) for p in ("0.001", "0.003", "0.005", "0.007", "0.009", "0.011", "0.013", "0.015")] + \
              [("d5_dp", p) for p in ("0.001", "0.003", "0.005", "0.007", "0.009", "0.011")]


def _spearman(a, b):
    ra, rb = np.argsort(np.argsort(a)).astype(float), np.argsort(np.argsort(b)).astype(float)
    return float(np.corrcoef(ra, rb)[0, 1])


def test_all_shipped_agents_over_the_reference_sweeps(dq, torch_mod):
    """Every agent the reference ships (trained_models/d5_x/0.001 .. 0.015, d5_dp/0.001 .. 0.011: 14 weight sets, committed as data
    fixtures) over the test-rate sweep the reference recorded for it (all_results.p = the final rolling
    averages of detailed_results/results_<p>.p -- 130 episodes at p = 0.001 up to 75 000 at 0.011 in the shipped files -- with the authors' NN referee), rates >= 0.003 (below, single episodes last 10^4 - 10^5 rounds: the two 0.007 agents
    additionally run 0.002) -- 1024 lattices x 1 episode per point, one batched device-resident evaluation each (DQNAgent.test: the
    episode records stay on the device, one host look per 64 vector steps).  Asserted: every point within x1.2 of the reference's mean
    lifetime and the median ratio within 3 % of 1 (measured, round 3: 125 points, ours / reference between 0.924 and 1.081, median 1.005 -- the
    built-in minimum-weight referee and the authors' NN referee evidently agree on what a logical error is); the rank correlation of log-lifetimes over all
    points; per agent the lifetimes fall monotonically with the rate as the reference's do; and across the agents of a family at the
    common rate 0.005 (the highest every agent was swept to) the reference's clear ordering (the agent trained at 0.001 is far the worst) is reproduced."""
    from conftest import load_golden
    ours, theirs, tags = [], [], []
    table = {}
    for family, p_train in ALL_SHIPPED:
        fx = load_golden(f"keras_weights_{family}_{p_train}")
        weights = [fx[f"w{i}"] for i in range(12)]
        ref = dict(zip((round(float(x), 3) for x in fx["ref_test_p"]), (float(x) for x in fx["ref_lifetime"])))
        cfg = dict(C3 if family == "d5_dp" else C2)
        lo = 0.002 if p_train == "0.007" else 0.003
        env = dq.VectorEnv(n_envs=1024, **cfg)
        agent = _make_agent(dq, env.obs_shape, env.num_actions)
        agent._bind(env)
        agent.model.set_weights(weights)
        seq = []
        for p in sorted(ref):
            if p < lo - 1e-9:
                continue
            env.p_phys = env.p_meas = p
            th = agent.test(env, nb_episodes=1024, visualize=False, verbose=0, single_cycle=False)
            life = float(np.mean(th.history["episode_lifetime"]))
            assert len(th.history["episode_lifetime"]) == 1024
            ours.append(life); theirs.append(ref[p]); tags.append((family, p_train, p)); seq.append(life)
            table[(family, p_train, p)] = (life, ref[p])
        assert all(a > b for a, b in zip(seq, seq[1:])), (family, p_train, seq)          # lifetimes fall with the error rate
        print(f"{family}/{p_train}: " + "  ".join(f"{t[2]:.3f}: {o:.0f}/{r:.0f}" for t, o, r in zip(tags[-len(seq):], ours[-len(seq):], theirs[-len(seq):])))
    ours, theirs = np.array(ours), np.array(theirs)
    ratio = ours / theirs
    print(f"{len(ours)} (agent, rate) points: ours / reference min {ratio.min():.3f} median {np.median(ratio):.3f} max {ratio.max():.3f}; "
          f"Spearman {_spearman(ours, theirs):.4f}")
    assert len(ours) >= 110
    assert _spearman(ours, theirs) > 0.99
    worst = int(np.argmax(np.abs(np.log(ratio))))
    assert 1 / 1.2 < ratio.min() and ratio.max() < 1.2, (tags[worst], ours[worst], theirs[worst])
    assert abs(np.median(ratio) - 1.0) < 0.03
    for family, n_agents in (("d5_x", 8), ("d5_dp", 6)):
        at = [(table[k][0], table[k][1], k[1]) for k in table if k[0] == family and abs(k[2] - 0.005) < 1e-9]
        assert len(at) == n_agents
        o, r = np.array([a[0] for a in at]), np.array([a[1] for a in at])
        assert int(np.argmin(o)) == int(np.argmin(r))                                  # the agent trained at 0.001 is the worst, in both
        print(family, "agents at test rate 0.005: Spearman", round(_spearman(o, r), 3))
        assert _spearman(o, r) > 0.6


def test_training_from_scratch_learns_to_decode(dq, torch_mod):
    """The whole device loop through the reference's API (build_convolutional_nn, DQNAgent.fit / test) learns: 4096 d=5 bit-flip
    lattices at p = 0.007, ~25 M environment steps (a few seconds), then greedy lifetimes far above the untrained policy's ~13
    measurement rounds.  (tools/train_demo.py runs the long version: 82 M steps in 7 s -> lifetime ~800; the reference's best
    agent reports 347 with its own referee.)"""
    from importlib import import_module
    ag = import_module("deepq-decoding_amd.agent")
    N, vsteps = 4096, 6000
    env = dq.VectorEnv(n_envs=N, d=5, error_model="X", use_Y=False, volume_depth=5, p_phys=0.007, p_meas=0.007)
    model = ag.build_convolutional_nn([[64, 3, 2], [32, 2, 1], [32, 2, 1]], [[512, 0.2]], env.obs_shape, env.num_actions)
    policy = ag.LinearAnnealedPolicy(ag.EpsGreedyQPolicy(masked_greedy=False), attr="eps", value_max=1.0, value_min=0.02, value_test=0.0,
                                     nb_steps=N * vsteps // 4)
    dqn = ag.DQNAgent(model=model, nb_actions=env.num_actions, memory=ag.SequentialMemory(limit=1 << 20, window_length=1),
                      nb_steps_warmup=N * 8, target_model_update=N * 250, policy=policy, test_policy=ag.GreedyQPolicy(masked_greedy=True),
                      gamma=0.99, enable_dueling_network=True, batch_size=N)
    dqn.compile(ag.Adam(lr=3e-4))
    dqn.fit(env, nb_steps=N * vsteps, verbose=0, log_interval=N * 1000, episode_averaging_length=2000, min_nb_steps=N * vsteps,
            single_cycle=False, sync_interval=500)
    th = dqn.test(env, nb_episodes=1024, visualize=False, verbose=0, single_cycle=False)
    life = float(np.mean(th.history["episode_lifetime"]))
    print("lifetime after 25 M steps:", life)
    assert life > 100.0, life


def test_driver_style_script_on_the_dropin_tree(dq, torch_mod, tmp_path):
    """The call sequence of the reference's single-point driver (build the network with keras.models.Sequential, SequentialMemory,
    annealed epsilon-greedy policy, DQNAgent(...).compile(Adam), fit with the fork's keywords, pickle the memory, save_weights to
    final_dqn_weights.h5f, a fresh agent that loads them, mutate env.p_phys / p_meas, test) through the reference-named modules under
    dropin/ only -- what a maintainer gets by putting that directory on PYTHONPATH."""
    import pickle
    import sys
    dropin = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "deepq-decoding_amd", "dropin")
    sys.path.insert(0, dropin)
    try:
        from keras.layers import Activation, Conv2D, Dense, Dropout, Flatten
        from keras.models import Sequential
        from keras.optimizers import Adam
        from rl.agents.dqn import DQNAgent
        from rl.callbacks import FileLogger
        from rl.memory import SequentialMemory
        from rl.policy import EpsGreedyQPolicy, GreedyQPolicy, LinearAnnealedPolicy
        from Environments import Surface_Code_Environment_Multi_Decoding_Cycles

        def network(cc, ff, input_shape, num_actions):
            m = Sequential()
            m.add(Conv2D(filters=cc[0][0], kernel_size=cc[0][1], strides=cc[0][2], input_shape=input_shape, data_format="channels_first"))
            m.add(Activation("relu"))
            for f, k, st in cc[1:]:
                m.add(Conv2D(filters=f, kernel_size=k, strides=st, data_format="channels_first"))
                m.add(Activation("relu"))
            m.add(Flatten())
            for units, rate in ff:
                m.add(Dense(units))
                m.add(Activation("relu"))
                m.add(Dropout(rate=rate))
            m.add(Dense(num_actions))
            m.add(Activation("linear"))
            return m

        env = Surface_Code_Environment_Multi_Decoding_Cycles(d=3, p_phys=0.005, p_meas=0.005, error_model="X", use_Y=False, volume_depth=3,
                                                             static_decoder=None)

        def agent(policy):
            a = DQNAgent(model=network(C_LAYERS, FF_LAYERS, env.observation_space.shape, env.num_actions), nb_actions=env.num_actions,
                         memory=SequentialMemory(limit=5000, window_length=1), nb_steps_warmup=50, target_model_update=100, policy=policy,
                         test_policy=GreedyQPolicy(masked_greedy=True), gamma=0.99, enable_dueling_network=True)
            a.compile(Adam(lr=1e-4))
            return a
        dqn = agent(LinearAnnealedPolicy(EpsGreedyQPolicy(masked_greedy=False), attr="eps", value_max=1.0, value_min=0.02, value_test=0.0,
                                         nb_steps=200))
        log = FileLogger(filepath=str(tmp_path / "training_history.json"), interval=10)
        hist = dqn.fit(env, nb_steps=300, action_repetition=1, callbacks=[log], verbose=0, visualize=False, nb_max_start_steps=0,
                       start_step_policy=None, log_interval=10, nb_max_episode_steps=None, episode_averaging_length=10,
                       success_threshold=10000, stopping_patience=1000, min_nb_steps=200, single_cycle=False)
        assert "episode_lifetimes_rolling_avg" in hist.history
        pickle.dump(dqn.memory, open(tmp_path / "memory.p", "wb"))
        wfile = str(tmp_path / "final_dqn_weights.h5f")
        dqn.save_weights(wfile, overwrite=True)
        assert open(wfile, "rb").read(8) == b"\x89HDF\r\n\x1a\n"
        dqn2 = agent(GreedyQPolicy(masked_greedy=True))
        dqn2.model.load_weights(wfile)
        assert all(np.array_equal(a, b) for a, b in zip(dqn.model.get_weights(), dqn2.model.get_weights()))
        env.p_phys = 0.002
        env.p_meas = 0.002
        th = dqn2.test(env, nb_episodes=5, visualize=False, verbose=0, interval=10, single_cycle=False)
        assert len(th.history["episode_lifetimes_rolling_avg"]) >= 1
        # the continue-training driver: unpickled memory + initial weights, then fit again
        mem = pickle.load(open(tmp_path / "memory.p", "rb"))
        entries = mem.nb_entries
        assert entries >= 300
        dqn3 = DQNAgent(model=network(C_LAYERS, FF_LAYERS, env.observation_space.shape, env.num_actions), nb_actions=env.num_actions,
                        memory=mem, nb_steps_warmup=50, target_model_update=100, policy=EpsGreedyQPolicy(masked_greedy=False),
                        test_policy=GreedyQPolicy(masked_greedy=True), gamma=0.99, enable_dueling_network=True)
        dqn3.compile(Adam(lr=1e-4))
        dqn3.model.load_weights(wfile)
        dqn3.fit(env, nb_steps=120, action_repetition=1, callbacks=[], verbose=0, visualize=False, nb_max_start_steps=0,
                 start_step_policy=None, log_interval=10, nb_max_episode_steps=None, episode_averaging_length=10,
                 success_threshold=10000, stopping_patience=1000, min_nb_steps=50, single_cycle=False)
        assert dqn3.memory.nb_entries >= entries + 100
    finally:
        sys.path.pop(0)


@pytest.mark.parametrize("name", ["c3", "c5", "c2", "c3-ragged", "per-layer", "mixed"])
def test_fused_step_equals_separate_calls_at_baseline_size(dq, torch_mod, name):
    """BASELINE.json sizes (c3 / c2: 4096 lattices and a 4096-sample minibatch; c5: d = 7, 1024 per GPU): DQNCore.step_and_update (four forwards in one pair of launches with
    32-row dense workgroups, next minibatch drawn on the environment launch, TD step inside the backward, Adam on its reduction) leaves
    exactly the state that act_and_step() + update() leave -- parameters, moments, replay ring, episode counters -- bit for bit."""
    torch = torch_mod
    N, cfg = {"c3": (4096, dict(d=5, error_model="DP", use_Y=False, volume_depth=5, p_phys=0.011, p_meas=0.011)),
              "c5": (1024, dict(d=7, error_model="DP", use_Y=False, volume_depth=7, p_phys=0.005, p_meas=0.005)),
              "c2": (4096, dict(d=5, error_model="X", use_Y=False, volume_depth=5, p_phys=0.007, p_meas=0.007)),
              "c3-ragged": (1003, dict(d=5, error_model="DP", use_Y=False, volume_depth=5, p_phys=0.011, p_meas=0.011)),
              # 18 input planes: outside what the fused chains cover -> the per-layer GEMM path behind the same calls
              "per-layer": (96, dict(d=7, error_model="DP", use_Y=False, volume_depth=16, p_phys=0.004, p_meas=0.004)),
              # 10 input planes on the d = 7 image: 2250-byte observations -- the fused chains cover the forward, not the backward: the acting, target and online forwards
              # fused, the training forward and the backward per layer, no environment step riding on the backward
              "mixed": (96, dict(d=7, error_model="DP", use_Y=False, volume_depth=8, p_phys=0.004, p_meas=0.004))}[name]
    B = 777 if name == "c3-ragged" else N                           # neither a multiple of the 8 / 16 / 32 samples a workgroup takes
    cores = []
    for _ in range(2):
        env = dq.VectorEnv(n_envs=N, **cfg)
        net = dq.QNetwork(env.obs_shape, C_LAYERS, FF_LAYERS, env.num_actions, max_batch=N)
        assert net.fused_supported == (name != "per-layer")
        assert net.fused_backward_supported == (name not in ("per-layer", "mixed"))
        core = dq.DQNCore(env, net, batch_size=B, memory_limit=N * 12, gamma=0.99, lr=1e-3)
        assert core._fused_update() == net.fused_backward_supported and (name != "mixed" or not core.compact)
        core.reset_env()
        for _ in range(4):
            core.act_and_step(0.2)
        cores.append(core)
    a, b = cores
    for t in range(8):
        a.step_and_update(0.2, presample_next=(t % 3 != 2))
        b.act_and_step(0.2, presample=(t % 2 == 0))
        b.update()
        if t == 4:
            a.update_target_hard(); b.update_target_hard()
        assert torch.equal(a.params, b.params) and torch.equal(a.m, b.m) and torch.equal(a.v, b.v), t
        assert torch.equal(a.index, b.index) and torch.equal(a.q_act, b.q_act), t
    for x, y in ((a.obs_ring[:], b.obs_ring[:]), (a.action_ring, b.action_ring), (a.reward_ring, b.reward_ring), (a.terminal_ring, b.terminal_ring)):
        assert torch.equal(x, y)                # (obs_ring[:]: the tensor, or the compact ring's words decoded -- core.ObsRingView)
    assert a.read_stats() == b.read_stats() and a.read_stats()[3] == 0
    assert not torch.equal(a.params, a.target)


def test_the_loop_runs_where_only_the_forward_is_fused(dq, torch_mod):
    """d = 7 with X noise at volume_depth 9: 10 input planes again (9 syndrome planes + 1 action plane), the other configuration whose forward is fused and
    whose backward is not.  Three steps of the loop with two extra updates each (the paired-target form must not be taken either): finite parameters that moved,
    a loss, and the range word clear."""
    torch = torch_mod
    env = dq.VectorEnv(n_envs=64, d=7, error_model="X", use_Y=False, volume_depth=9, p_phys=0.005, p_meas=0.005)
    assert tuple(env.obs_shape) == (10, 15, 15)
    net = dq.QNetwork(env.obs_shape, C_LAYERS, FF_LAYERS, env.num_actions, max_batch=64)
    assert net.fused_supported and not net.fused_backward_supported
    core = dq.DQNCore(env, net, batch_size=48, memory_limit=64 * 12, gamma=0.99, lr=1e-3)
    assert not core.compact and not core._fused_update()
    core.reset_env()
    for _ in range(4):
        core.act_and_step(0.3)
    p0 = core.params.clone()
    for _ in range(3):
        core.step_and_update(0.3, extra_updates=2)
    loss, mean_q = core.read_metrics()
    assert core.updates == 9 and core.vector_steps == 7
    assert torch.isfinite(core.params).all() and not torch.equal(core.params, p0) and np.isfinite(loss) and np.isfinite(mean_q)


@pytest.mark.parametrize("name,cfg,n,R", [("c4", C3, 4096, 8), ("c5", C5, 1024, 8), ("c3-ragged", C3, 1003, 3)])
def test_one_large_batch_equals_the_concatenation_of_rank_shards(dq, torch_mod, name, cfg, n, R):
    """BASELINE.json configs[3] / [4] at GLOBAL size on one GPU: c4 = 32 768 d=5 DP lattices, c5 = 8 192 d=7 lattices, against the same
    job cut into R rank shards the way bench.py / DQNCore do it (rank r: lattice ids [r n, (r+1) n), sample ids [r B, (r+1) B), loss
    gradient scaled by 1 / (B R)).  (1) Acting + environment: every ring row of the big run equals the owning shard's row, bit for
    bit, over several eps-greedy vector steps.  (2) The update: the SUM of the R shard gradients -- what the RCCL all-reduce
    produces -- equals the big run's gradient on the concatenated minibatch within f32 summation round-off.  Together with the
    2-rank gloo tests this is the multi-GPU evidence available without an 8-GPU node."""
    torch = torch_mod
    N, steps = n * R, 6
    seed = (0x5EED, 0xD0DEC0DE)

    def make(n_envs, base, rank, world, batch):
        env = dq.VectorEnv(n_envs=n_envs, env_id_base=base, seed=seed, **cfg)
        net = dq.QNetwork(env.obs_shape, C_LAYERS, FF_LAYERS, env.num_actions, max_batch=max(n_envs, batch))
        core = dq.DQNCore(env, net, batch_size=batch, memory_limit=n_envs * 7, gamma=0.99, lr=1e-3, seed=seed, rank=rank, world_size=world)
        core.reset_env()
        for _ in range(steps):
            core.act_and_step(0.3)
        return core
    big = make(N, 0, 0, 1, N)
    T = big.T
    rows_big = []
    g_sum = torch.zeros_like(big.grads, dtype=torch.float64)
    for r in range(R):
        sh = make(n, r * n, r, R, n)
        assert sh.T == T and sh.cur == big.cur and torch.equal(sh.params, big.params)
        sl = slice(r * n, (r + 1) * n)
        assert torch.equal(big.obs_ring[:, sl], sh.obs_ring[:]) and torch.equal(big.action_ring[:, sl], sh.action_ring)
        assert torch.equal(big.reward_ring[:, sl], sh.reward_ring) and torch.equal(big.terminal_ring[:, sl], sh.terminal_ring)
        assert torch.equal(big.env.export_state()[sl], sh.env.export_state())
        g_sum += sh.local_gradient().double()
        idx = sh.index.long()                                   # shard row slot * n + e  ->  big row slot * N + r n + e
        rows_big.append((idx // n) * N + r * n + idx % n)
        del sh
    g_big = big.local_gradient(index=torch.cat(rows_big).to(torch.int32)).double()
    scale = float(g_big.abs().max())
    assert scale > 0
    diff = (g_sum - g_big).abs()
    assert float(diff.max()) < 2e-5 * scale, (float(diff.max()), scale)
    assert float(diff.mean()) < 1e-6 * scale


def test_config_dict_driven_grid_on_one_gpu(dq, torch_mod, tmp_path):
    """the reference's pickled fixed_config.p / variable_config_N.p drive the run (runner.train_single_point == the
    call sequence of Single_Point_Training_Script.py, then the Continue script from the first point's weights + memory), and
    runner.run_grid places the grid's points on the node's GPUs one at a time each (here: the one GPU, two points in turn)."""
    import pickle
    runner = dq.runner
    fixed = {"d": 3, "use_Y": False, "train_freq": 1, "batch_size": 32, "print_freq": 50, "rolling_average_length": 50,
             "stopping_patience": 100000, "error_model": "X", "c_layers": C_LAYERS, "ff_layers": FF_LAYERS, "max_timesteps": 64 * 60,
             "volume_depth": 3, "testing_length": 64, "buffer_size": 64 * 40, "dueling": True, "masked_greedy": False, "static_decoder": True}
    fam = str(tmp_path / "d3_x")
    dirs = runner.write_grid(fam, fixed, 0.001, 100000, grid=dict(learning_rate=[1e-4, 5e-5], exploration_fraction=[64 * 30],
                                                                  target_network_update_freq=[640], final_eps=[0.02], learning_starts=[256]))
    assert len(dirs) == 2
    codes = runner.run_grid(os.path.join(fam, "0.001"), gpus=[0], n_envs=64, extra_args=["--quiet", "--sync-interval", "4"])
    assert codes == {1: 0, 2: 0}, open(os.path.join(fam, "0.001", "output_files", "err_0.001_1.err")).read()[-2000:]
    for cdir in dirs:
        files = set(os.listdir(cdir))
        assert {"started_at.p", "training_history.json", "memory.p", "final_dqn_weights.h5f", "results.p", "all_results.p"} <= files
        allr = pickle.load(open(os.path.join(cdir, "all_results.p"), "rb"))
        assert list(allr)[0] == "0.001" and all(v > 0 for v in allr.values())
        assert len(json.load(open(os.path.join(cdir, "training_history.json")))["episode"]) > 0
    res = runner.collect_results(os.path.join(fam, "0.001"))
    assert set(res) == {"1", "2"} and all(isinstance(v, float) for v in res.values())
    # the Controller pass: best point -> next error rate's grid, continuing from its weights and memory (in this process)
    new = runner.spawn_next(fam, fixed, 0.001, 0.003, thresholds={"0.001": 0.0},
                            grid=dict(learning_rate=[1e-4], exploration_fraction=[64 * 20], max_eps=[0.5], target_network_update_freq=[640],
                                      final_eps=[0.02], learning_starts=[128]))
    assert len(new) == 1 and os.path.exists(os.path.join(new[0], "initial_dqn_weights.h5f"))
    mem_before = pickle.load(open(os.path.join(new[0], "memory.p"), "rb")).nb_entries
    allr = runner.train_single_point(new[0], n_envs=64, verbose=0, sync_interval=4)
    assert "0.001" in allr and pickle.load(open(os.path.join(new[0], "memory.p"), "rb")).nb_entries >= mem_before


def test_agent_loop_with_a_device_evaluated_network_referee(dq, torch_mod):
    """c5's lattice (d = 7) with the reference's kind of referee -- a feed-forward network called every step (ENV:53,144; here a Dense
    stack evaluated on the device, dq_env_set_referee_mlp) -- through DQNAgent.fit / test: the step of such an environment does not
    ride on the dense backward (policy kernel, referee pre-pass and step are separate launches), everything else is the same loop."""
    R = importlib.import_module("deepq-decoding_amd.referee")
    rng = np.random.RandomState(4)
    dims = [64, 80, 4]
    w = []
    for a, b in zip(dims, dims[1:]):
        w += [(rng.randn(a, b) / np.sqrt(a)).astype(np.float32), np.zeros(b, np.float32)]
    env = dq.VectorEnv(n_envs=64, referee=R.FeedForwardReferee(w), **dict(C5, volume_depth=3))
    assert env.mlp_referee
    agent = _make_agent(dq, env.obs_shape, env.num_actions, batch_size=32, warmup=64 * 4)
    hist = agent.fit(env, nb_steps=64 * 40, verbose=0, episode_averaging_length=50, success_threshold=None, stopping_patience=None,
                     min_nb_steps=0, single_cycle=False, sync_interval=8)
    assert agent._core.updates > 20 and len(hist.history["episode"]) > 0 and np.isfinite(hist.history["loss"][-1])
    th = agent.test(env, nb_episodes=64, visualize=False, verbose=0, single_cycle=False)
    assert len(th.history["episode_lifetime"]) == 64


def test_reference_training_run_replayed_against_its_own_record(dq, torch_mod):
    """The training half against a REFERENCE-HELD record (the keras-rl fork is not in the tree, so the update rule and the fit
    loop have no source-level pin): the reference's from-scratch run trained_models/d5_x/0.001 (training_history.json + its two config
    dicts, committed as data: tests/golden/training_history_d5_x_0.001.npz) replayed through runner.train_single_point -> DQNAgent.fit
    with the same recipe -- one lattice, batch 32, Adam 1e-5, epsilon 1 -> 0.02 over 200 000 steps, target copy every 5000, warm-up 1000 --
    for its first 120 000 steps (the whole 998 377-step run: tools/replay_reference_training.py, record in profiles/).  Random numbers
    and referee differ by construction, so the comparison is statistical: mean_eps exact; mean_q within x1.25, loss within x2 and the
    rolling lifetime within x1.5 of the reference's curve at 10 000 / 25 000 / 50 000 / 100 000 steps (measured: within 10 %, the loss within
    x1.7; round 4 asserted x2 / x4 / x3).  The shortened run's greedy lifetime is printed, not judged (the record is the finished agent's)."""
    import sys
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
    sys.path.insert(0, tools)
    try:
        import replay_reference_training as R
    finally:
        sys.path.pop(0)
    res = R.run("d5_x", "0.001", max_steps=120000, sweep_rates=[0.005])
    rows, ok = R.compare(res)
    for at, key, a, b, good in rows:
        print(f"{str(at):>8} {key:<60} ours {a:12.5g} reference {b:12.5g} {'ok' if good else 'OUTSIDE'}")
    assert ok, [r for r in rows if not r[4]]
    assert int(res["ours"]["nb_steps"][-1]) >= 119000 and len(rows) >= 13
    # keys and their order are the reference file's
    assert list(res["ours"]) == [str(k) for k in res["record"]["key_order"]]
