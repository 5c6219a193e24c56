"""The learner on the wide lattices (d = 9 .. 15): the Q-network DQNAgent.fit creates there -- the reference's stack on (volume_depth + action layers,
2d + 1, 2d + 1) observations and up to 676 actions, all on the per-layer kernels (csrc/qnet.hip, csrc/gemm.h, the TD kernels of csrc/dqn.hip) -- inside the
device loop, against the loop assembled from the CPU oracles: the wide C environment oracle (oracle/env_oracle_wide.c, pinned by tests/test_oracle_wide_c.py),
dqn_oracle.select_action on its legal words, the float64 network oracle; and a guided fit() on a wide core that takes optimizer steps.  The network alone, at
the same shapes: tests/test_arch_gpu.py on the wide entries of tests/architectures.py."""
import numpy as np
import pytest

import architectures as AR
from oracle import c_oracle, dqn_oracle as O, memory_oracle as M, philox
from test_env_wide_gpu import CONFIGS, SEED

pytestmark = pytest.mark.gpu

C_LAYERS, FF_LAYERS = AR.REF_CONV, AR.REF_FF

# architecture entry -> the environment configuration whose observations and actions it carries, and that configuration's legal words
WIDE_ENTRIES = {"wide_d11_dpy": ("d11dpy", 6), "wide_d13_dp": ("d13dp", 6), "wide_d15_x": ("d15x", 4), "wide_d15_dpy": ("d15dpy", 11)}


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return torch


@pytest.mark.parametrize("name", sorted(WIDE_ENTRIES))
def test_the_architecture_entries_have_the_environments_shapes(dq, torch_mod, name):
    """The wide entries of tests/architectures.py are the networks of these environments: observation shape, action count, and the legal words the
    policy reads beside the Q-values."""
    cfg_name, words = WIDE_ENTRIES[name]
    shape, _, _, A, dueling, _ = AR.ARCHITECTURES[name]
    env = dq.VectorEnv(n_envs=4, seed=SEED, **CONFIGS[cfg_name])
    try:
        assert env.wide
        assert tuple(env.obs_shape) == tuple(shape) and env.num_actions == A and dueling
        assert env.legal_words == -(-A // 64) == words
    finally:
        env.close()


# name -> (configuration, (observation shape, actions, legal words), episodes that must end inside the 9 steps).  d9dp is the configuration of
# tests/test_agent_gpu.py's d = 9 loop, where no episode ends; the others run at p = 0.02, where episodes end and lattices are reset inside the ring, so that
# terminal rows reach the sampler and the TD targets (at the rates of tests/test_env_wide_gpu.py, 0.006 and 0.003, nothing ends in 54 lattice-steps)
HOT = dict(p_phys=0.02, p_meas=0.02)
LOOPS = {
    "d9dp": (dict(d=9, error_model="DP", use_Y=False, volume_depth=3, p_phys=0.006, p_meas=0.006), ((5, 19, 19), 163, 3), 0),
    "d9dp-hot": (dict(d=9, error_model="DP", use_Y=False, volume_depth=3, **HOT), ((5, 19, 19), 163, 3), 1),
    "d11dpy": (dict(CONFIGS["d11dpy"], **HOT), ((7, 23, 23), 364, 6), 1),
    "d15dpy": (dict(CONFIGS["d15dpy"], **HOT), ((6, 31, 31), 676, 11), 1),
}


def _select(q, legal_words, eps, masked_greedy, t, seed, base=0):
    """dqn_oracle.select_action per lattice on the oracle's legal words (tests/test_env_wide_gpu.py _policy_oracle, under the loop's seed)."""
    out = np.zeros(q.shape[0], dtype=np.int32)
    for i in range(q.shape[0]):
        mask = sum(int(w) << (64 * k) for k, w in enumerate(legal_words[i]))
        words = philox.site_words(seed, (base + i) & 0xFFFFFFFF, t, 0, stream=philox.STREAM_POLICY)
        out[i] = O.select_action(q[i], mask, eps, masked_greedy, words)
    return out


@pytest.mark.parametrize("name", list(LOOPS))
def test_device_loop_on_wide_lattices_matches_oracle_loop(dq, torch_mod, name):
    """The schedule of test_agent_gpu.test_device_loop_at_distance_nine_matches_oracle_loop -- 6 lattices, minibatch 4, a ring of 7 slots that wraps, 9 vector
    steps, step_and_update and act_and_step + update alternating -- with the wide C oracle as the environment: the ring's actions, observations, rewards
    and terminals bit for bit at every step, the sampled rows those of the sampler's definition, loss and mean Q within 1e-5 and the gradient within
    1e-5 * max(1, max |g|) of the float64 oracle at every update (that test's bounds).  d = 9 runs here as well: the Python and the C environment oracle
    then judge the same device run."""
    cfg, (shape, A, words), min_done = LOOPS[name]
    N, B, steps, eps, gamma, lr = 6, 4, 9, 0.4, 0.99, 1e-3
    seed = SEED
    env = dq.VectorEnv(n_envs=N, seed=seed, **cfg)
    assert env.wide and env.legal_words == words and tuple(env.obs_shape) == shape and env.num_actions == A
    net = dq.QNetwork(env.obs_shape, C_LAYERS, FF_LAYERS, env.num_actions, max_batch=max(N, B))
    assert not net.fused_supported and not net.fused_backward_supported            # (A + 1 > 128: every forward and backward per layer)
    core = dq.DQNCore(env, net, batch_size=B, memory_limit=N * 6, gamma=gamma, lr=lr, seed=seed)
    spec = O.QNetSpec(env.obs_shape, C_LAYERS, FF_LAYERS, env.num_actions)
    p = core.params.cpu().numpy().astype(np.float64)
    assert np.array_equal(core.params.cpu().numpy(), O.glorot_init(spec, seed))
    p_t = p.copy()                                                   # (no target copy inside the 9 steps)
    ref = c_oracle.COracleWideEnv(n_envs=N, seed=seed, **cfg)
    T = core.T
    ring_obs = np.zeros((T, N) + tuple(env.obs_shape), np.uint8)
    ring_a, ring_r, ring_t = np.zeros((T, N), np.int32), np.zeros((T, N), np.float32), np.zeros((T, N), np.uint8)
    core.reset_env()
    ref.reset()
    cur, filled, n_updates = 0, 1, 0
    ring_obs[0] = ref.obs
    assert np.array_equal(core.obs_ring[0].cpu().numpy(), ref.obs)
    worst = dict(loss=0.0, mean_q=0.0, grad=0.0)
    seen = dict(done=0, reset=0, terminal_rows=0)
    for t in range(steps):
        will_update = min(T, filled + 1) >= 4
        fused = will_update and t % 2 == 0
        if fused:
            core.step_and_update(eps)
        else:
            core.act_and_step(eps, presample=True)
        q, _ = O.forward(spec, p, ring_obs[cur])
        acts = _select(q, ref.legal, eps, False, t, seed)
        assert np.array_equal(core.action_ring[cur].cpu().numpy(), acts), (name, "actions", t)
        ref.step(acts, auto_reset=True)
        nxt = (cur + 1) % T
        ring_a[cur], ring_r[cur], ring_t[cur], ring_obs[nxt] = acts, ref.reward, ref.done, ref.obs
        assert np.array_equal(core.obs_ring[nxt].cpu().numpy(), ref.obs), (name, "obs", t)
        assert np.array_equal(core.reward_ring[cur].cpu().numpy(), ref.reward), (name, "reward", t)
        assert np.array_equal(core.terminal_ring[cur].cpu().numpy(), ref.done), (name, "terminal", t)
        seen["done"] += int(ref.done.sum())
        seen["reset"] += int(ref.was_reset.sum())
        cur, filled = nxt, min(T, filled + 1)
        if not will_update:
            continue
        if not fused:
            core.update()
        n_updates += 1
        u = n_updates
        assert core.updates == u
        idx = core.index.cpu().numpy()
        assert np.array_equal(idx, M.device_replay_rows(ring_t, N, T, cur, filled, B, seed, u)), (name, "rows", t)
        rows = T * N
        flat_obs = ring_obs.reshape(rows, *env.obs_shape)
        s0, s1 = flat_obs[idx], flat_obs[(idx + N) % rows]
        seen["terminal_rows"] += int(ring_t.reshape(-1)[idx].sum())
        y = O.td_targets(O.forward(spec, p, s1)[0], O.forward(spec, p_t, s1)[0], ring_r.reshape(-1)[idx], ring_t.reshape(-1)[idx], gamma)
        keep = O.dropout_keep_mask(seed, u, np.arange(B), 512, 0.2)
        q0, cache = O.forward(spec, p, s0, training=True, keep_masks=[keep])
        loss, mean_q, dq_ = O.loss_and_grad(q0, ring_a.reshape(-1)[idx], y)
        g = O.backward(spec, p, cache, dq_)
        met = np.array(core.read_metrics())
        g_dev = core.grads.cpu().numpy()
        scale = float(np.abs(g).max())
        e_loss, e_q, e_g = abs(met[0] - loss), abs(met[1] - mean_q), float(np.abs(g_dev - g).max())
        worst = dict(loss=max(worst["loss"], e_loss), mean_q=max(worst["mean_q"], e_q), grad=max(worst["grad"], e_g / max(1.0, scale)))
        assert e_loss < 1e-5 and e_q < 1e-5, (name, t, met, loss, mean_q)
        assert scale > 0 and e_g < 1e-5 * max(1.0, scale), (name, t, e_g, scale)
        # the oracle's weights glued to the device's fp32 values, so that round-off cannot accumulate into an action flip
        p = core.params.cpu().numpy().astype(np.float64)
    print(f"WIDE LOOP {name}: {n_updates} updates, {spec.n_params} parameters; loss error {worst['loss']:.2e}, mean Q error {worst['mean_q']:.2e} (bounds 1e-5), "
          f"gradient error {worst['grad']:.2e} of max(1, max |g|) (bound 1e-5); {seen['done']} episodes ended, {seen['reset']} lattices reset, {seen['terminal_rows']} sampled rows terminal")
    assert n_updates >= 5 and seen["done"] >= min_done and seen["reset"] >= min_done
    assert len(set(ring_a.reshape(-1).tolist())) > N                 # (a run of one constant action would compare nothing)
    env.close()


def _guided_fit(dq, torch, cfg, n, steps, warmup_steps):
    env = dq.VectorEnv(n_envs=n, seed=SEED, **cfg)
    assert env.wide
    model = dq.build_convolutional_nn(C_LAYERS, FF_LAYERS, env.obs_shape, env.num_actions)
    policy = dq.EpsGreedyQPolicy(eps=0.5, masked_greedy=True, guide=dq.WideUnionFindAgent(), guide_share=0.5)
    agent = dq.DQNAgent(model=model, nb_actions=env.num_actions, memory=dq.SequentialMemory(limit=n * 40, window_length=1),
                        nb_steps_warmup=n * warmup_steps, target_model_update=512, policy=policy, test_policy=dq.GreedyQPolicy(masked_greedy=True),
                        gamma=0.99, enable_dueling_network=True, batch_size=32, seed=(1, 2))
    agent.compile(dq.Adam(lr=1e-4))
    agent._bind(env)
    initial = agent._core.params.clone()
    agent.fit(env, nb_steps=n * steps, verbose=0, episode_averaging_length=50, success_threshold=None, stopping_patience=None, min_nb_steps=0,
              single_cycle=False)
    return env, agent, initial


def test_guided_fit_on_a_wide_core_takes_optimizer_steps(dq, torch_mod):
    """d = 11 DP, volume_depth 3, 32 lattices, eps 0.5 with half of the exploring lattices following WideUnionFindAgent, a warm-up of 4 of the 16 vector
    steps: the updates happen (steps 5 .. 16), none is discarded, some but not all lattice-steps followed the teacher, the parameters moved and are
    finite -- and a second run from the same seeds leaves the same parameters, moments and ring, bit for bit."""
    torch = torch_mod
    cfg = dict(d=11, error_model="DP", use_Y=False, volume_depth=3, p_phys=0.006, p_meas=0.006)
    n, steps = 32, 16
    runs = []
    for _ in range(2):
        env, agent, initial = _guided_fit(dq, torch, cfg, n, steps, warmup_steps=4)
        core = agent._core
        assert core._wide and not core.net.fused_supported and tuple(env.obs_shape) == (5, 23, 23) and env.num_actions == 243
        assert core.vector_steps == steps and agent.step == n * steps
        assert core.updates >= 10, core.updates
        loss, mean_q = core.read_metrics()                           # (the synchronisation that counts discarded updates)
        assert core.discarded_updates == 0 and np.isfinite(loss) and np.isfinite(mean_q)
        assert 0 < agent.last_guided_steps < n * steps, agent.last_guided_steps
        assert bool(torch.isfinite(core.params).all()) and not torch.equal(core.params, initial)
        assert bool(torch.isfinite(core.m).all()) and bool(torch.isfinite(core.v).all()) and bool((core.v > 0).any())
        runs.append([x.clone() for x in (core.params, core.m, core.v, core.obs_ring[:], core.action_ring, core.reward_ring, core.terminal_ring)]
                    + [core.updates, agent.last_guided_steps, loss, mean_q])
        print(f"WIDE GUIDED FIT: {core.updates} updates, {agent.last_guided_steps} of {n * steps} lattice-steps guided, loss {loss:.6f}, mean Q {mean_q:.6f}")
        env.close()
    for a, b in zip(runs[0][:7], runs[1][:7]):
        assert torch.equal(a, b)
    assert runs[0][7:] == runs[1][7:]
