"""keras-rl's finite delta_clip (the Huber TD loss) on the GPU, on every update path: the per-layer TD kernels (dq_td_loss_grad_clip,
dq_td_step), the TD step inside the fused dense backward (dq_qnet_td_backward_* with dq_td_job.delta_clip), the gradient scale it
implies, the riding environment step, the whole device loop, rank shards and the agent.  oracle/dqn_oracle.py has no Huber form: the
reference here is float64 c() / h() applied to the oracle's TD targets, and the oracle's backward fed the clipped dq."""
import importlib

import numpy as np
import pytest

import shipped
from oracle import c_oracle, dqn_oracle as O, philox
from relu_choices import device_relu_choices

pytestmark = pytest.mark.gpu

C_LAYERS, FF_LAYERS = [[64, 3, 2], [32, 2, 1], [32, 2, 1]], [[512, 0.2]]
C1 = dict(d=3, error_model="X", use_Y=False, volume_depth=3, p_phys=0.005, p_meas=0.005)
C3 = dict(d=5, error_model="DP", use_Y=False, volume_depth=5, p_phys=0.011, p_meas=0.011)
C5 = dict(d=7, error_model="DP", use_Y=False, volume_depth=7, p_phys=0.005, p_meas=0.005)
SEED = (0x5EED, 0xD0DEC0DE)


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def huber_c(x, delta):
    x = np.asarray(x, np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(np.abs(x) > delta, np.copysign(delta, x), x)


def huber_h(x, delta):
    x = np.asarray(x, np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(np.abs(x) > delta, delta * (np.abs(x) - 0.5 * delta), 0.5 * x * x)


def huber_c32(x, delta):
    """c() in float32, the kernels' arithmetic: x and delta as float32, a compare and a copysign (exact)."""
    x, d = np.asarray(x, np.float32), np.float32(delta)
    return np.where(np.abs(x) > d, np.copysign(d, x), x).astype(np.float32)


def _Q():
    return importlib.import_module("deepq-decoding_amd.qnet")


# ---- 1. the per-layer TD kernels ----------------------------------------------------------------------------------------------------
def test_per_layer_td_kernels_apply_the_huber_clamp_and_loss(dq, torch_mod):
    torch, Q = torch_mod, _Q()
    rng = np.random.RandomState(41)
    B, A, gamma, gs = 1000, 51, 0.99, 1.0 / 1000
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    q1o, q1t = cu(rng.randn(B, A).astype(np.float32) * 3), cu(rng.randn(B, A).astype(np.float32) * 3)
    rows = 3 * B
    reward, terminal = cu(rng.choice([-1.0, 0.0, 1.0], size=rows).astype(np.float32)), cu((rng.rand(rows) < 0.1).astype(np.uint8))
    action, index = cu(rng.randint(0, A, size=rows).astype(np.int32)), cu(rng.permutation(rows)[:B].astype(np.int32))
    q0_np = rng.randn(B, A).astype(np.float32) * 3
    y_inf = torch.empty(B, device="cuda")
    Q.td_update(q1o, q1t, cu(q0_np), reward, terminal, action, gamma, grad_scale=gs, index=index, y=y_inf)
    # TD errors log-uniform over [1e-3, 1e3] (both signs): the clamp at 0.05 / 1 / 10 catches 72 / 50 / 33 per cent of the samples
    y_np, a_b = y_inf.cpu().numpy(), action.cpu().numpy()[index.cpu().numpy()]
    td = (10.0 ** rng.uniform(-3, 3, size=B)) * rng.choice([-1.0, 1.0], size=B)
    q0_np[np.arange(B), a_b] = (y_np + td).astype(np.float32)
    q0 = cu(q0_np)
    diff32 = q0_np[np.arange(B), a_b] - y_np                                        # float32 subtraction, as the kernels do it
    for delta in (0.05, 1.0, 10.0):
        clipped = np.abs(diff32) > np.float32(delta)
        assert 0.1 < clipped.mean() < 0.9, clipped.mean()
        dq_ref = np.zeros((B, A), np.float32)
        dq_ref[np.arange(B), a_b] = huber_c32(diff32, delta) * np.float32(gs)
        loss_ref = float(np.mean(huber_h(diff32.astype(np.float64), delta)))
        # dq_td_step (td_update with a finite delta), with and without the riding episode bookkeeping
        for with_stats in (False, True):
            y, met = torch.empty(B, device="cuda"), torch.zeros(Q.TD_METRICS_FLOATS, device="cuda")
            st = None
            if with_stats:
                n = 64
                st = (cu(np.ones(n, np.uint8)), cu(np.zeros(n, np.uint8)), cu(np.arange(n, dtype=np.uint32)), cu(np.ones(n, np.float32)), n,
                      torch.zeros(4, dtype=torch.int64, device="cuda"))
            dq_ = Q.td_update(q1o, q1t, q0, reward, terminal, action, gamma, grad_scale=gs, index=index, y=y, metrics=met, step_stats=st,
                              delta_clip=delta)
            Q.td_metrics(met, B)
            assert torch.equal(y, y_inf)                                            # the target does not change
            assert np.array_equal(dq_.cpu().numpy(), dq_ref)
            assert abs(float(met[0]) - loss_ref) <= 1e-6 * loss_ref
            if with_stats:
                assert st[5].cpu().tolist() == [64, sum(range(64)), 64, 64]
        # dq_td_loss_grad_clip on the same target
        dq2, met2 = Q.td_loss_grad(q0, action, y_inf, grad_scale=gs, index=index, delta_clip=delta)
        assert np.array_equal(dq2.cpu().numpy(), dq_ref)
        assert abs(float(met2[0]) - loss_ref) <= 1e-6 * loss_ref
    # delta = inf through the new keyword is the old call, bit for bit
    dq_a, met_a = Q.td_loss_grad(q0, action, y_inf, grad_scale=gs, index=index)
    dq_b, met_b = Q.td_loss_grad(q0, action, y_inf, grad_scale=gs, index=index, delta_clip=np.inf)
    assert torch.equal(dq_a, dq_b) and torch.equal(met_a[:2], met_b[:2])
    # NaN in Q_target(s1) propagates into dq (the clamp is a compare), an infinite one becomes +-delta
    q1n = q1t.clone()
    q1n[3] = float("nan")
    q1n[5] = float("inf")
    dq_n = Q.td_update(q1o, q1n, q0, reward, terminal, action, gamma, grad_scale=gs, index=index, delta_clip=1.0).cpu().numpy()
    t_rows = terminal.cpu().numpy()[index.cpu().numpy()]
    if not t_rows[3]:
        assert np.isnan(dq_n[3, a_b[3]])
    if not t_rows[5]:
        assert dq_n[5, a_b[5]] == np.float32(-gs)
    with pytest.raises(ValueError):
        Q.td_update(q1o, q1t, q0, reward, terminal, action, gamma, delta_clip=0.0)


# ---- 2. fused chains vs per-layer f32 path vs the float64 oracle ----------------------------------------------------------------
def _td_setup(torch, Q, net, params, obs_t, B, A, rng, td_sd=2.0):
    """A TD job whose TD errors are ~N(0, td_sd): Q_target(s1) = Q_online(s1) = (Q(s0)[a_b] + td - r) / gamma in every column (computed
    from a training forward with the update's dropout draw).  Fragile samples (O.fragile_samples) get TD error 0 (terminal, reward = Q(s0)[a_b])."""
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    action = rng.randint(0, A, size=B).astype(np.int32)
    reward = rng.choice([-1.0, 0.0, 1.0], size=B).astype(np.float32)
    q0 = net.forward(params, obs_t, training=True, seed=(1, 2), t=7).cpu().numpy()
    qa = q0[np.arange(B), action].astype(np.float64)
    td = rng.randn(B) * td_sd
    q1 = np.repeat(((qa + td - reward) / 0.99).astype(np.float32)[:, None], A, axis=1)
    return dict(action=action, reward=reward, q1=q1, qa=qa)


def _fused_f32_oracle(dq, torch, spec, flat, obs, A, delta, fragile_rel=1e-6, dueling=True):
    Q = _Q()
    B = obs.shape[0]
    net = dq.QNetwork(obs.shape[1:], C_LAYERS, FF_LAYERS, A, dueling=dueling, max_batch=B)
    assert net.fused_supported
    params = torch.from_numpy(flat).cuda()
    obs_t = torch.from_numpy(obs).cuda()
    keep = O.dropout_keep_mask((1, 2), 7, np.arange(B), 512, 0.2)
    q_ref, cache = O.forward(spec, flat, obs, training=True, keep_masks=[keep])
    fragile = O.fragile_samples(cache, rel=fragile_rel)
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    net.set_fused(True)
    s = _td_setup(torch, Q, net, params, obs_t, B, A, np.random.RandomState(B))     # (the same TD job for both paths, from the fused forward)
    terminal, reward = np.zeros(B, np.uint8), s["reward"].copy()
    terminal[fragile], reward[fragile] = 1, s["qa"][fragile].astype(np.float32)     # y = Q(s0)[a_b]: TD error 0 on the fused path
    out = {}
    for fused in (True, False):
        net.set_fused(fused)
        q0 = net.forward(params, obs_t, training=True, seed=(1, 2), t=7)
        q0n = q0.cpu().numpy()
        p_, m_, v_, g_ = params.clone(), torch.zeros_like(params), torch.zeros_like(params), torch.empty_like(params)
        td = dict(q_online_s1=cu(s["q1"]), q_target_s1=cu(s["q1"]), q_s0=q0, reward=cu(reward), terminal=cu(terminal), action=cu(s["action"]),
                  gamma=0.99, grad_scale=1.0 / B, index=None, y=torch.empty(B, device="cuda"), dq=torch.zeros((B, A), device="cuda"),
                  metrics=torch.zeros(Q.TD_METRICS_FLOATS, device="cuda"), delta_clip=delta)
        net.td_backward_adam(p_, td, g_, m_, v_, 1, 1e-4)
        net.check_range()
        out[fused] = dict(y=td["y"].cpu().numpy(), dq=td["dq"].cpu().numpy(), g=g_.cpu().numpy(), q0=q0n, p=p_)
    # the TD step: identical y; dq equal wherever Q(s0)[a_b] is (the two forwards agree to fp32 round-off, not bit for bit) -- checked as c() of
    # each path's own Q(s0)[a_b] - y, bit for bit
    fu, pl = out[True], out[False]
    assert np.array_equal(fu["y"], pl["y"])
    for o in (fu, pl):
        diff32 = o["q0"][np.arange(B), s["action"]] - o["y"]
        ref = np.zeros((B, A), np.float32)
        ref[np.arange(B), s["action"]] = huber_c32(diff32, delta) * np.float32(1.0 / B)
        assert np.array_equal(o["dq"], ref)
        assert np.all(np.abs(o["dq"]) <= np.float32(delta) * np.float32(1.0 / B))
        assert not torch.equal(o["p"], params)
    clipped = np.abs(fu["q0"][np.arange(B), s["action"]] - fu["y"]) > delta
    assert 0.1 < clipped.mean() < 0.95
    # gradients against the float64 oracle's backward of the clipped dq
    g_ref = O.backward(spec, flat, cache, fu["dq"].astype(np.float64))
    scale = max(1.0, float(np.abs(g_ref).max()))
    for o in (fu, pl):
        err = np.abs(o["g"] - g_ref).max()
        assert err < 1e-5 * scale, (err, scale)
    return out


@pytest.mark.parametrize("B", [4096, 32])
def test_fused_and_per_layer_td_backward_match_the_oracle_on_shipped_weights(dq, torch_mod, B):
    """c3 (d = 5 DP, the shipped d5_dp/0.011 agent) at the reference's schedule (B = 32) and the benchmark's (B = 4096), delta = 1."""
    _, flat = shipped.shipped_weights("d5_dp", "0.011")
    spec = O.QNetSpec((7, 11, 11), shipped.C_LAYERS, shipped.FF_LAYERS, 51)
    obs = shipped.real_observations("d5_dp", 0.011, B)
    _fused_f32_oracle(dq, torch_mod, spec, flat, obs, 51, 1.0)


@pytest.mark.parametrize("name", ["d7", "no-dueling"])
def test_fused_and_per_layer_td_backward_match_the_oracle_other_heads(dq, torch_mod, name):
    """d = 7 (99 actions: the NT2 = 7 form of the dense backward) and a network without the dueling head (the non-SHORT TD prologue)."""
    cfg, dueling = (C5, True) if name == "d7" else (C3, False)
    env = c_oracle.COracleEnv(n_envs=64, seed=SEED, **cfg)
    env.reset()
    obs = []
    for t in range(4):
        obs.append(env.obs.copy())
        env.step(env.policy_uniform_legal(t), auto_reset=True)
    obs = np.concatenate(obs)
    A = {"d7": 99, "no-dueling": 51}[name]
    spec = O.QNetSpec(obs.shape[1:], C_LAYERS, FF_LAYERS, A, dueling=dueling)
    flat = O.glorot_init(spec, (11, 22)).astype(np.float32)
    flat += (np.random.RandomState(5).randn(flat.size) * 0.02).astype(np.float32)
    _fused_f32_oracle(dq, torch_mod, spec, flat, obs, A, 0.5, fragile_rel=None, dueling=dueling)


# ---- 3. range: a finite delta bounds the gradient, the host-known scale never overflows ---------------------------------------------
def test_finite_delta_carries_any_td_error_with_the_host_known_scale(dq, torch_mod):
    torch, Q = torch_mod, _Q()
    _, flat = shipped.shipped_weights("d5_dp", "0.011")
    shape, A, B = (7, 11, 11), 51, 256
    spec = O.QNetSpec(shape, shipped.C_LAYERS, shipped.FF_LAYERS, A)
    obs = shipped.real_observations("d5_dp", 0.011, B)
    net = dq.QNetwork(shape, shipped.C_LAYERS, shipped.FF_LAYERS, A, dueling=True, max_batch=B)
    params = torch.from_numpy(flat).cuda()
    cu = lambda a: torch.from_numpy(a).cuda()
    obs_t = cu(obs)
    rng = np.random.RandomState(3)
    action, idx = cu(rng.randint(0, A, size=B).astype(np.int32)), cu(np.arange(B, dtype=np.int32))
    reward, terminal = cu(np.zeros(B, np.float32)), cu(np.zeros(B, np.uint8))
    seed, t = (1, 2), 7
    keep = O.dropout_keep_mask(seed, t, np.arange(B), 512, 0.2)
    _, cache = O.forward(spec, flat, obs, training=True, keep_masks=[keep])
    # dq is formed inside the launch, so no sample can be given dq = 0: the oracle takes the fused path's own side of every ReLU whose pre-activation is
    # within fp32 round-off of 0 instead (tests/relu_choices.py), read back once from the training forward every launch below repeats
    assert O.fragile_samples(cache, rel=1e-6).any()
    choices = device_relu_choices(net, params, spec, flat, obs, keep, lambda: net.forward(params, obs_t, training=True, seed=seed, t=t), rel=1e-6,
                                  cache=cache, label="d5_dp/0.011 B=256 fused")

    def run(td_size, q1=None):
        """td_backward_adam with Q_target(s1) = -td_size / gamma everywhere (a TD error of Q(s0)[a] + td_size), delta = 1, auto_scale = 0."""
        p_, m_, v_, g_ = params.clone(), torch.zeros_like(params), torch.zeros_like(params), torch.empty_like(params)
        if q1 is None:
            q1 = torch.full((B, A), -td_size / 0.99, dtype=torch.float32, device="cuda")
        q0 = net.forward(p_, obs_t, training=True, seed=seed, t=t)
        td = dict(q_online_s1=q1, q_target_s1=q1, q_s0=q0, reward=reward, terminal=terminal, action=action, gamma=0.99, grad_scale=1.0 / B,
                  index=idx, y=torch.empty(B, device="cuda"), dq=torch.empty((B, A), device="cuda"),
                  metrics=torch.zeros(Q.TD_METRICS_FLOATS, device="cuda"), auto_scale=False, delta_clip=1.0)
        net.td_backward_adam(p_, td, g_, m_, v_, 1, 1e-4)
        return p_, g_, td["dq"]

    for td_size in (1e-3, 1.0, 1e3, 1e4, 1e6):
        p_, g_, dq_ = run(td_size)
        net.check_range()                                                           # never DQ_ERR_RANGE
        assert net.range_discarded() == 0
        assert torch.isfinite(g_).all() and torch.isfinite(p_).all() and not torch.equal(p_, params)
        dq_np = dq_.cpu().numpy().astype(np.float64)
        assert np.abs(dq_np).max() <= 1.0 / B
        g_ref = O.backward(spec, flat, cache, dq_np, relu_on=choices)
        err = np.abs(g_.cpu().numpy() - g_ref).max()
        print(f"TD error ~{td_size:g}, delta 1, host-known scale: max |g| {np.abs(g_ref).max():.3e}, max abs error {err:.2e}")
        assert err < 1e-5 * np.abs(g_ref).max(), (td_size, err)
    # a NaN TD error is still the guard's: the whole update discarded and reported
    q1 = torch.zeros((B, A), dtype=torch.float32, device="cuda")
    q1[17] = float("nan")
    p_, g_, _ = run(0.0, q1=q1)
    with pytest.raises(dq.DeepQError):
        net.check_range()
    assert net.range_discarded() == 1
    assert torch.equal(p_, params)
    net.check_range()


# ---- 4. delta at or above every TD error of the minibatch (and <= 8): the bits of delta = inf ---------------------------------------
def test_delta_above_every_td_error_gives_the_bits_of_the_unclipped_update(dq, torch_mod):
    torch, Q = torch_mod, _Q()
    _, flat = shipped.shipped_weights("d5_dp", "0.011")
    shape, A, B = (7, 11, 11), 51, 4096
    obs_t = torch.from_numpy(shipped.real_observations("d5_dp", 0.011, B)).cuda()
    net = dq.QNetwork(shape, shipped.C_LAYERS, shipped.FF_LAYERS, A, dueling=True, max_batch=B)
    params = torch.from_numpy(flat).cuda()
    s = _td_setup(torch, Q, net, params, obs_t, B, A, np.random.RandomState(9), td_sd=1.0)
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    results = {}
    for delta in (np.inf, None, 8.0):
        p_, m_, v_, g_ = params.clone(), torch.zeros_like(params), torch.zeros_like(params), torch.empty_like(params)
        q0 = net.forward(p_, obs_t, training=True, seed=(1, 2), t=7)
        y = torch.empty(B, device="cuda")
        td = dict(q_online_s1=cu(s["q1"]), q_target_s1=cu(s["q1"]), q_s0=q0, reward=cu(s["reward"]), terminal=cu(np.zeros(B, np.uint8)),
                  action=cu(s["action"]), gamma=0.99, grad_scale=1.0 / B, index=None, y=y, metrics=torch.zeros(Q.TD_METRICS_FLOATS, device="cuda"))
        if delta is None:                                                   # the smallest delta >= max |TD error| (float32)
            diff = q0.cpu().numpy()[np.arange(B), s["action"]] - y_inf
            delta = float(np.abs(diff).max())
            assert delta <= 8.0
        td["delta_clip"] = delta
        net.td_backward_adam(p_, td, g_, m_, v_, 1, 1e-4)
        net.check_range()
        if np.isinf(delta):
            y_inf = y.cpu().numpy()
        results[delta] = (g_.clone(), p_, m_, v_, td["metrics"][2:].clone())
    g0, p0, m0, v0, met0 = results[np.inf]
    for delta, (g, p, m, v, met) in results.items():
        assert torch.equal(g, g0) and torch.equal(p, p0) and torch.equal(m, m0) and torch.equal(v, v0), delta
        assert torch.equal(met, met0), delta                                # the loss / mean_q partials too: h(x) = 0.5 x^2 for every sample


# ---- 5. the riding environment step -------------------------------------------------------------------------------------------------
def test_riding_environment_step_with_delta_equals_separate_calls(dq, torch_mod):
    """DQNCore.step_and_update (environment step riding on the dense backward) leaves exactly the state act_and_step() + update() leave,
    with delta_clip = 1."""
    torch = torch_mod
    N = 1024
    cores = []
    for _ in range(2):
        env = dq.VectorEnv(n_envs=N, **C3)
        net = dq.QNetwork(env.obs_shape, C_LAYERS, FF_LAYERS, env.num_actions, max_batch=N)
        core = dq.DQNCore(env, net, batch_size=N, memory_limit=N * 12, gamma=0.99, lr=1e-3, delta_clip=1.0)
        core.reset_env()
        for _ in range(4):
            core.act_and_step(0.2)
        cores.append(core)
    a, b = cores
    assert a.ride_env
    for t in range(6):
        a.step_and_update(0.2, presample_next=(t % 3 != 2))
        b.act_and_step(0.2, presample=(t % 2 == 0))
        b.update()
        assert torch.equal(a.params, b.params) and torch.equal(a.m, b.m) and torch.equal(a.v, b.v), t
        assert torch.equal(a.dq, b.dq) and torch.equal(a.y, b.y)
    assert a.read_metrics() == b.read_metrics()
    assert a.read_stats() == b.read_stats()
    assert a.discarded_updates == 0 and b.discarded_updates == 0


# ---- 6. the whole loop against the oracle loop with the Huber gradient --------------------------------------------------------------
@pytest.mark.parametrize("name,cfg,N,B,steps", [("c1", C1, 16, 8, 11), ("c3", C3, 64, 32, 10)])
def test_device_loop_with_delta_matches_oracle_loop(dq, torch_mod, name, cfg, N, B, steps):
    torch = torch_mod
    from oracle import memory_oracle as M
    eps, gamma, lr, delta = 0.3, 0.99, 1e-3, 0.1
    env = dq.VectorEnv(n_envs=N, seed=SEED, **cfg)
    net = dq.QNetwork(env.obs_shape, C_LAYERS, FF_LAYERS, env.num_actions, max_batch=max(N, B))
    core = dq.DQNCore(env, net, batch_size=B, memory_limit=N * 8, gamma=gamma, lr=lr, seed=SEED, delta_clip=delta)
    spec = O.QNetSpec(env.obs_shape, C_LAYERS, FF_LAYERS, env.num_actions)
    p = core.params.cpu().numpy().astype(np.float64)
    p_t = p.copy()
    m, v = np.zeros_like(p), np.zeros_like(p)
    ref = c_oracle.COracleEnv(n_envs=N, seed=SEED, **cfg)
    T = core.T
    ring_obs = np.zeros((T, N) + env.obs_shape, np.uint8)
    ring_a, ring_r, ring_t = np.zeros((T, N), np.int32), np.zeros((T, N), np.float32), np.zeros((T, N), np.uint8)
    core.reset_env()
    ref.reset()
    cur, filled, n_updates, n_clipped = 0, 1, 0, 0
    ring_obs[0] = ref.obs
    for t in range(steps):
        will_update = min(T, filled + 1) >= 4
        fused = will_update and t % 3 == 2
        if fused:
            core.step_and_update(eps, presample_next=(t % 2 == 0))
        else:
            core.act_and_step(eps, presample=(t % 2 == 0))
        q, _ = O.forward(spec, p, ring_obs[cur])
        acts = np.zeros(N, np.int32)
        for i in range(N):
            w = philox.philox4x32((t, 0, i, philox.STREAM_POLICY << 16), SEED)
            mask = int(ref.legal[i, 0]) | (int(ref.legal[i, 1]) << 64)
            acts[i] = O.select_action(q[i], mask, eps, False, w)
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
        assert np.array_equal(idx, M.device_replay_rows(ring_t, N, T, cur, filled, B, SEED, u))
        rows = T * N
        flat_obs = ring_obs.reshape(rows, *env.obs_shape)
        s0, s1 = flat_obs[idx], flat_obs[(idx + N) % rows]
        y = O.td_targets(O.forward(spec, p, s1)[0], O.forward(spec, p_t, s1)[0], ring_r.reshape(-1)[idx], ring_t.reshape(-1)[idx], gamma)
        keep = O.dropout_keep_mask(SEED, u, np.arange(B), 512, 0.2)
        q0, cache = O.forward(spec, p, s0, training=True, keep_masks=[keep])
        a_b = ring_a.reshape(-1)[idx]
        x = q0[np.arange(B), a_b] - y
        n_clipped += int((np.abs(x) > delta).sum())
        dq_ = np.zeros_like(q0)
        dq_[np.arange(B), a_b] = huber_c(x, delta) / B
        g = O.backward(spec, p, cache, dq_)
        p, m, v = O.adam_step(p, g, m, v, u, lr)
        loss, mean_q = core.read_metrics()
        assert abs(loss - float(np.mean(huber_h(x, delta)))) < 1e-5 and abs(mean_q - float(np.mean(q0.max(axis=1)))) < 1e-5
        assert np.abs(core.grads.cpu().numpy() - g).max() < 1e-5 * max(1.0, np.abs(g).max())
        big = np.abs(g) > 1e-6
        assert np.abs(core.params.cpu().numpy() - p)[big].max() < 5e-6
        if u % 3 == 0:
            core.update_target_hard()
        p = core.params.cpu().numpy().astype(np.float64)
        m, v = core.m.cpu().numpy().astype(np.float64), core.v.cpu().numpy().astype(np.float64)
        if u % 3 == 0:
            p_t = p.copy()
    assert n_clipped > 0 and core.discarded_updates == 0


# ---- 7. rank shards --------------------------------------------------------------------------------------------------------------
def test_rank_shard_gradients_with_delta_sum_to_the_large_batch_gradient(dq, torch_mod):
    torch = torch_mod
    n, R, steps, cfg = 4096, 8, 6, C3
    N = n * R

    def make(n_envs, base, rank, world, batch):
        env = dq.VectorEnv(n_envs=n_envs, env_id_base=base, seed=SEED, **cfg)
        net = dq.QNetwork(env.obs_shape, C_LAYERS, FF_LAYERS, env.num_actions, max_batch=max(n_envs, batch))
        core = dq.DQNCore(env, net, batch_size=batch, memory_limit=n_envs * 7, gamma=0.99, lr=1e-3, seed=SEED, rank=rank, world_size=world,
                          delta_clip=1.0)
        core.reset_env()
        for _ in range(steps):
            core.act_and_step(0.3)
        return core
    big = make(N, 0, 0, 1, N)
    rows_big = []
    g_sum = torch.zeros_like(big.grads, dtype=torch.float64)
    for r in range(R):
        sh = make(n, r * n, r, R, n)
        g_sum += sh.local_gradient().double()
        idx = sh.index.long()
        rows_big.append((idx // n) * N + r * n + idx % n)
        del sh
    g_big = big.local_gradient(index=torch.cat(rows_big).to(torch.int32)).double()
    scale = float(g_big.abs().max())
    assert scale > 0
    diff = (g_sum - g_big).abs()
    assert float(diff.max()) < 2e-5 * scale, (float(diff.max()), scale)
    assert float(diff.mean()) < 1e-6 * scale


# ---- 8. the agent -------------------------------------------------------------------------------------------------------------------
def test_agent_fit_with_delta_clip(dq, torch_mod):
    """DQNAgent(delta_clip=1.0).fit at c1 (the single-lattice facade) for a few thousand steps runs to the end without a discarded update, and
    the loss it logs is the Huber metric: the last update's loss equals mean h() of that update's own TD errors (Q(s0)[a_b] - y on the device)."""
    env = dq.Surface_Code_Environment_Multi_Decoding_Cycles(static_decoder=None, **C1)
    model = dq.build_convolutional_nn(C_LAYERS, FF_LAYERS, env.observation_space.shape, env.num_actions)
    agent = dq.DQNAgent(model=model, nb_actions=env.num_actions, memory=dq.SequentialMemory(limit=5000, window_length=1), nb_steps_warmup=100,
                        target_model_update=200, policy=dq.EpsGreedyQPolicy(masked_greedy=False), test_policy=dq.GreedyQPolicy(masked_greedy=True),
                        gamma=0.99, enable_dueling_network=True, delta_clip=1.0)
    agent.compile(dq.Adam(lr=1e-3))
    hist = agent.fit(env, nb_steps=3000, verbose=0, single_cycle=False)
    core = agent._core
    assert agent.step >= 3000 and core.delta_clip == 1.0 and core.discarded_updates == 0 and core.updates > 2000
    h = hist.history["loss"]
    assert any(x == x for x in h) and all(x >= 0.0 for x in h if x == x)
    loss, _ = core.read_metrics()
    B = core.batch_size
    idx = core.index.cpu().numpy()
    a_b = core.action_ring.cpu().numpy().reshape(-1)[idx]
    x = core.q0.cpu().numpy()[np.arange(B), a_b].astype(np.float64) - core.y.cpu().numpy()
    assert abs(loss - float(np.mean(huber_h(x, 1.0)))) <= 1e-5 * max(1.0, loss)
    dq_ = core.dq.cpu().numpy()[np.arange(B), a_b] * B
    assert np.allclose(dq_, huber_c(x, 1.0), rtol=1e-5, atol=1e-6)
