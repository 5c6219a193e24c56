"""Per-lattice error rates on the GPU (VectorEnv.set_rates with sequences, dq_env_set_rates_per_lattice / dq_envb_set_rates_per_lattice):
a lattice at rate p draws exactly what a uniform-rate environment at p draws for the same global id and seed, in every step body -- one
lattice per wave (d = 7), two per wave with the halves at different rates (d <= 5), the multi-step act_steps launch, the step riding on
the dense backward, the wide environment (d = 9) -- and DQNAgent.test_error_rates equals one test() per rate."""
import numpy as np
import pytest

from oracle import c_oracle

pytestmark = pytest.mark.gpu

SEED = (0x5EED, 0xD0DEC0DE)
C_LAYERS, FF_LAYERS = [[64, 3, 2], [32, 2, 1], [32, 2, 1]], [[512, 0.2]]
RATES = [0.003, 0.012, 0.045]                           # a 15x span: the groups' lifetimes and event counts differ by far more than noise

CFGS = {
    "d3x": dict(d=3, error_model="X", use_Y=False, volume_depth=3),
    "d5dp": dict(d=5, error_model="DP", use_Y=False, volume_depth=5),
    "d5iidxz": dict(d=5, error_model="IIDXZ", use_Y=False, volume_depth=4),
    "d7dp": dict(d=7, error_model="DP", use_Y=False, volume_depth=7),
    "d9dp": dict(d=9, error_model="DP", use_Y=False, volume_depth=5),
}


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return torch


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _groups(n, K, layout):
    """lattice indices of each rate group: contiguous blocks (the last absorbs the remainder) or interleaved i mod K (splits every pair)."""
    if layout == "interleaved":
        return [np.arange(g, n, K) for g in range(K)]
    m = n // K
    return [np.arange(g * m, n if g == K - 1 else (g + 1) * m) for g in range(K)]


def _group_env(dq, cfg, n, base, idx, layout, p, **kw):
    """(env, rows): a uniform-rate environment that holds group `idx`'s lattices under the same global ids, and the rows where they sit.
    Contiguous groups get an environment of their own lattices (env_id_base = the group's first id); interleaved ones the whole id range."""
    if layout == "interleaved":
        return dq.VectorEnv(n_envs=n, seed=SEED, env_id_base=base, p_phys=p, p_meas=p, **cfg, **kw), idx
    return dq.VectorEnv(n_envs=len(idx), seed=SEED, env_id_base=base + int(idx[0]), p_phys=p, p_meas=p, **cfg, **kw), np.arange(len(idx))


def _oracle(cfg, n, base, idx, layout, p):
    cls = c_oracle.COracleWideEnv if cfg["d"] > 7 else c_oracle.COracleEnv
    if layout == "interleaved":
        return cls(n_envs=n, seed=SEED, env_id_base=base, p_phys=p, p_meas=p, **cfg), idx
    return cls(n_envs=len(idx), seed=SEED, env_id_base=base + int(idx[0]), p_phys=p, p_meas=p, **cfg), np.arange(len(idx))


@pytest.mark.parametrize("layout", ["contiguous", "interleaved"])
@pytest.mark.parametrize("name,n,steps,base", [("d3x", 515, 64, 7), ("d5dp", 515, 64, 4096), ("d5iidxz", 387, 64, 2 ** 31 - 1000),
                                               ("d7dp", 259, 64, 0), ("d9dp", 131, 40, 33)])
def test_mixed_rates_equal_homogeneous_runs(dq, torch_mod, name, n, steps, base, layout):
    torch = torch_mod
    cfg = CFGS[name]
    wide = cfg["d"] > 7
    K = len(RATES)
    groups = _groups(n, K, layout)
    rate_of = np.empty(n)
    for g, idx in enumerate(groups):
        rate_of[idx] = RATES[g]
    meas_of = rate_of * 0.5                                              # p_meas != p_phys: the two thresholds are not swapped
    env = dq.VectorEnv(n_envs=n, seed=SEED, env_id_base=base, p_phys=0.02, p_meas=0.02, **cfg)
    env.set_rates(rate_of, meas_of)
    assert isinstance(env.p_phys, np.ndarray) and np.array_equal(env.p_phys, rate_of) and np.array_equal(env.rates[1], meas_of)
    homo, orc = [], []
    for g, idx in enumerate(groups):
        e, rows = _group_env(dq, cfg, n, base, idx, layout, RATES[g])
        e.set_rates(RATES[g], RATES[g] * 0.5)
        o, orows = _oracle(cfg, n, base, idx, layout, RATES[g])
        o.set_rates(RATES[g], RATES[g] * 0.5)
        homo.append((e, rows))
        orc.append((o, orows))
    patch = not wide and env.patch_supported
    pw = torch.zeros((n, env.patch_stride), dtype=torch.int32, device="cuda") if patch else None
    env.reset(out_patch=pw)
    for (e, _), (o, _) in zip(homo, orc):
        e.reset(out_patch=torch.zeros((e.n_envs, e.patch_stride), dtype=torch.int32, device="cuda") if patch else None)
        o.reset()
    ev = np.zeros((K, 3), dtype=np.int64)                                # dones, auto-resets, summed lifetime at the ends of episodes
    for t in range(steps):
        a = env.select_actions(t)
        hp = []
        for g, ((e, rows), (o, orows)) in enumerate(zip(homo, orc)):
            ae = e.select_actions(t)
            assert torch.equal(ae[torch.as_tensor(rows, device="cuda")], a[torch.as_tensor(groups[g], device="cuda")]), (name, layout, g, t)
            hpw = torch.zeros((e.n_envs, e.patch_stride), dtype=torch.int32, device="cuda") if patch else None
            e.step(ae, auto_reset=True, out_patch=hpw)
            o.step(o.policy_uniform_legal(t), auto_reset=True)
            hp.append(hpw)
        env.step(a, auto_reset=True, out_patch=pw)
        obs, rew, done, life = env.obs.cpu().numpy(), env.reward.cpu().numpy(), env.done.cpu().numpy(), env.lifetime.cpu().numpy()
        legal, wr = _u64(env.legal), env.was_reset.cpu().numpy()
        for g, ((e, rows), (o, orows), hpw) in enumerate(zip(homo, orc, hp)):
            idx = groups[g]
            assert np.array_equal(obs[idx], e.obs.cpu().numpy()[rows]), (name, layout, g, t, "obs")
            assert np.array_equal(rew[idx], e.reward.cpu().numpy()[rows]), (name, layout, g, t, "reward")
            assert np.array_equal(done[idx], e.done.cpu().numpy()[rows]), (name, layout, g, t, "done")
            assert np.array_equal(life[idx], e.lifetime.cpu().numpy()[rows]), (name, layout, g, t, "lifetime")
            assert np.array_equal(legal[idx], _u64(e.legal)[rows]), (name, layout, g, t, "legal")
            if patch:
                assert torch.equal(pw[torch.as_tensor(idx, device="cuda")], hpw[torch.as_tensor(rows, device="cuda")]), (name, layout, g, t, "patch")
            assert np.array_equal(obs[idx], o.obs[orows]) and np.array_equal(rew[idx], o.reward[orows]), (name, layout, g, t, "oracle")
            assert np.array_equal(done[idx], o.done[orows]) and np.array_equal(life[idx].view(np.uint32), o.lifetime[orows]), (name, g, t)
            assert np.array_equal(legal[idx][:, :o.legal.shape[1]], o.legal[orows][:, :legal.shape[1]]), (name, layout, g, t, "oracle legal")
            ev[g] += (int(done[idx].sum()), int(wr[idx].sum()), int(life[idx][done[idx] != 0].astype(np.int64).sum()))
    st = _u64(env.export_state())
    for g, (e, rows) in enumerate(homo):
        assert np.array_equal(st[groups[g]], _u64(e.export_state())[rows]), (name, layout, g, "export_state")
    print(name, layout, ev.tolist())
    assert (ev[:, 0] > 0).all() and (ev[:, 1] > 0).all(), ev            # dones and auto-resets in every group
    assert len(set(ev[:, 2].tolist())) == K and len(set(ev[:, 1].tolist())) > 1, ev     # the rates are not ignored


@pytest.mark.parametrize("name,n", [("d3x", 513), ("d5dp", 517)])
def test_act_steps_with_per_lattice_rates(dq, torch_mod, name, n):
    """The multi-step launch (env_block2<EPB, true>) equals the per-step act_step loop at the same rates and the homogeneous groups."""
    torch = torch_mod
    cfg, T, K = CFGS[name], 48, len(RATES)
    rate_of = np.array([RATES[i % K] for i in range(n)])
    a_env = dq.VectorEnv(n_envs=n, seed=SEED, env_id_base=11, **cfg)
    b_env = dq.VectorEnv(n_envs=n, seed=SEED, env_id_base=11, **cfg)
    for e in (a_env, b_env):
        e.set_rates(rate_of)
        e.reset()
    C, H, W = a_env.obs_shape
    act = torch.zeros((T, n), dtype=torch.int32, device="cuda")
    rew = torch.zeros((T, n), dtype=torch.float32, device="cuda")
    don = torch.zeros((T, n), dtype=torch.uint8, device="cuda")
    obs = torch.zeros((T, n, C, H, W), dtype=torch.uint8, device="cuda")
    a_env.act_steps(T - 1, 5, act, rew, don, obs, slot0=0)
    for s in range(T - 1):
        b = b_env.act_step(5 + s, q=None, eps=1.0)
        assert torch.equal(b, act[s]) and torch.equal(b_env.reward, rew[s]) and torch.equal(b_env.done, don[s]), (name, s)
        assert torch.equal(b_env.obs, obs[s + 1]), (name, s)
    assert torch.equal(a_env.legal, b_env.legal) and torch.equal(a_env.lifetime, b_env.lifetime)
    assert torch.equal(a_env.export_state(), b_env.export_state())
    for g in range(K):                                                   # and the homogeneous group over the same ids
        h = dq.VectorEnv(n_envs=n, seed=SEED, env_id_base=11, p_phys=RATES[g], p_meas=RATES[g], **cfg)
        h.reset()
        for s in range(T - 1):
            h.act_step(5 + s, q=None, eps=1.0)
        rows = torch.arange(g, n, K, device="cuda")
        assert torch.equal(h.export_state()[rows], a_env.export_state()[rows]), (name, g)
    assert int(don.sum()) > 0


def _core(dq, env, N):
    net = dq.QNetwork(env.obs_shape, C_LAYERS, FF_LAYERS, env.num_actions, max_batch=N)
    return dq.DQNCore(env, net, batch_size=N, memory_limit=N * 12, gamma=0.99, lr=1e-3, seed=SEED)


def test_riding_environment_step_honours_the_rates(dq, torch_mod):
    """DQNCore.step_and_update with the environment step riding on the dense backward (ride_env) leaves the rings and parameters the
    separate launches leave (ride_env off, as DQ_RIDE_ENV=0), at mixed rates; with eps = 1 its transitions are the homogeneous groups'."""
    torch = torch_mod
    N, K, cfg = 1024, len(RATES), CFGS["d5dp"]
    rate_of = np.array([RATES[(i // 5) % K] for i in range(N)])         # runs of 5: mixed pairs and mixed blocks
    cores = []
    for ride in (True, False):
        env = dq.VectorEnv(n_envs=N, seed=SEED, **cfg)
        env.set_rates(rate_of)
        core = _core(dq, env, N)
        core.ride_env = ride
        core.reset_env()
        for _ in range(4):
            core.act_and_step(1.0)
        cores.append(core)
    a, b = cores
    for t in range(8):
        a.step_and_update(1.0)
        b.step_and_update(1.0)
        assert torch.equal(a.params, b.params) and torch.equal(a.m, b.m) and torch.equal(a.v, b.v), t
    for ring in ("action_ring", "reward_ring", "terminal_ring"):
        assert torch.equal(getattr(a, ring), getattr(b, ring)), ring
    assert torch.equal(a.obs_ring[:], b.obs_ring[:])
    assert torch.equal(a.env.export_state(), b.env.export_state())
    # the transitions are those of the groups at their own rates (eps = 1: the actions do not depend on the network)
    for g in range(K):
        env = dq.VectorEnv(n_envs=N, seed=SEED, p_phys=RATES[g], p_meas=RATES[g], **cfg)
        h = _core(dq, env, N)
        h.reset_env()
        for _ in range(4):
            h.act_and_step(1.0)
        for _ in range(8):
            h.act_and_step(1.0)
        rows = torch.as_tensor(np.flatnonzero(rate_of == RATES[g]), device="cuda")
        for ring in ("action_ring", "reward_ring", "terminal_ring"):
            assert torch.equal(getattr(h, ring)[:, rows], getattr(a, ring)[:, rows]), (g, ring)
        assert torch.equal(h.obs_ring[:][:, rows], a.obs_ring[:][:, rows]), g
        assert torch.equal(h.env.export_state()[rows], a.env.export_state()[rows]), g


def _agent(dq, env, batch_size=64, warmup=256):
    model = dq.build_convolutional_nn(C_LAYERS, FF_LAYERS, env.obs_shape, env.num_actions)
    policy = dq.LinearAnnealedPolicy(dq.EpsGreedyQPolicy(masked_greedy=False), attr="eps", value_max=1.0, value_min=0.02,
                                     value_test=0.0, nb_steps=2000)
    agent = dq.DQNAgent(model=model, nb_actions=env.num_actions, memory=dq.SequentialMemory(limit=env.n_envs * 40, window_length=1),
                        nb_steps_warmup=warmup, target_model_update=2048, policy=policy,
                        test_policy=dq.GreedyQPolicy(masked_greedy=True), gamma=0.99, enable_dueling_network=True,
                        batch_size=batch_size, seed=(1, 2))
    agent.compile(dq.Adam(lr=1e-4))
    return agent


def test_fit_at_mixed_rates(dq, torch_mod):
    torch = torch_mod
    env = dq.VectorEnv(n_envs=128, seed=SEED, **CFGS["d5dp"])
    env.set_rates(np.linspace(0.002, 0.03, 128))
    agent = _agent(dq, env)
    hist = agent.fit(env, nb_steps=128 * 30, verbose=0, episode_averaging_length=100, success_threshold=None, stopping_patience=None,
                     min_nb_steps=0, single_cycle=False, sync_interval=8)
    assert agent._core.updates >= 20 and len(hist.history["episode"]) >= 1
    assert torch.isfinite(agent._core.params).all()
    loss, mean_q = agent._core.read_metrics()
    assert np.isfinite(loss) and np.isfinite(mean_q)


@pytest.mark.parametrize("name", ["d5dp", "d7dp", "d9dp"])
def test_uniform_arrays_and_scalar_reset_keep_the_scalar_bits(dq, torch_mod, name):
    """An all-equal array gives the scalar path's bits; a scalar after per-lattice rates gives those of an environment that never had them."""
    torch = torch_mod
    cfg, n = CFGS[name], 133
    envs = [dq.VectorEnv(n_envs=n, seed=SEED, env_id_base=3, p_phys=0.01, p_meas=0.01, **cfg) for _ in range(3)]
    envs[1].set_rates(np.full(n, 0.01), [0.01] * n)
    assert envs[1].p_phys == 0.01 and isinstance(envs[1].p_phys, float)
    envs[2].set_rates(np.linspace(0.0, 0.2, n), 0.3)
    envs[2].p_phys = 0.01                                              # back to the scalar pair, one setter at a time
    assert isinstance(envs[2].p_phys, float) and envs[2].p_meas == 0.3
    envs[2].p_meas = 0.01
    assert envs[2].p_phys == 0.01 and envs[2].p_meas == 0.01 and envs[2].rates[0].shape == (n,)
    for e in envs:
        e.reset()
    for t in range(48):
        acts = [e.select_actions(t) for e in envs]
        for e, a in zip(envs, acts):
            e.step(a, auto_reset=True)
        for e, a in zip(envs[1:], acts[1:]):
            assert torch.equal(acts[0], a) and torch.equal(envs[0].obs, e.obs) and torch.equal(envs[0].reward, e.reward), t
            assert torch.equal(envs[0].done, e.done) and torch.equal(envs[0].legal, e.legal), t
            assert torch.equal(envs[0].lifetime, e.lifetime), t
    for e in envs[1:]:
        assert torch.equal(envs[0].export_state(), e.export_state())


@pytest.mark.parametrize("N,K,nb", [(300, 3, 101), (64, 5, 40)])
def test_error_rate_sweep_equals_separate_test_runs(dq, torch_mod, N, K, nb):
    """test_error_rates: each rate's History equals test() on a VectorEnv of that block's lattices alone, entry for entry."""
    cfg = CFGS["d5dp"]
    rates = [0.004, 0.008, 0.016, 0.03, 0.05][:K]
    env = dq.VectorEnv(n_envs=N, seed=SEED, env_id_base=40, p_phys=0.02, p_meas=0.02, **cfg)
    agent = _agent(dq, env)
    agent._bind(env)
    rng = np.random.default_rng(3)
    agent.model.set_weights([x + 0.05 * rng.standard_normal(x.shape).astype(np.float32) for x in agent.model.get_weights()])
    weights = agent.model.get_weights()
    res = agent.test_error_rates(env, rates, nb_episodes=nb, verbose=0)
    assert list(res) == rates and env.p_phys == 0.02 and env.p_meas == 0.02      # previous rates restored
    m = N // K
    for k, p in enumerate(rates):
        sub = dq.VectorEnv(n_envs=m, seed=SEED, env_id_base=40 + k * m, p_phys=p, p_meas=p, **cfg)
        tester = _agent(dq, sub)
        tester.model.set_weights(weights)
        h = tester.test(sub, nb_episodes=nb, visualize=False, verbose=0, single_cycle=False)
        assert h.history == res[p].history, (k, p)
        assert len(h.history["episode_lifetime"]) == nb
    means = [np.mean(res[p].history["episode_lifetime"]) for p in rates]
    assert means[0] > means[-1], means
