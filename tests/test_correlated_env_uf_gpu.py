"""The correlated union-find decoder as a policy and a teacher of the wide environment on the device (csrc/env_wide_uf.hip: env_wide_uf_kernel<true, true>,
env_wide_guided_uf_kernel<true, true>; VectorEnv.uf_select_wide / guided_select_wide(correlated=); decoder_wide.WideUnionFindAgent(correlated=);
DQNCore.guided_act_and_step_wide(correlated=)).  The reference is correlated_env_uf_ref.replay: the C oracle environment played by
tests/correlated_uf_ref.decode -- three passes per volume, grown in unit steps where the device jumps -- + decoder.frame_to_actions, computed once per
configuration; the device environment runs in lockstep with it, and on every record of a run the other triples are launched too: a select writes nothing, so
they cost nothing in trajectory.  Actions are compared bit for bit."""
import ctypes

import numpy as np
import pytest

import correlated_env_uf_ref as R
from test_wide_env_uf_cpu import SEED

pytestmark = pytest.mark.gpu

C_LAYERS, FF_LAYERS = [[64, 3, 2], [32, 2, 1], [32, 2, 1]], [[512, 0.2]]


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return torch


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _wide_env(dq, name, n=None, base=0):
    kw, n_all, _, _ = R.CONFIGS[name]
    return dq.VectorEnv(n_envs=n_all if n is None else n, seed=SEED, env_id_base=base, backend="wide", **kw)


def _evaluator(dq, env):
    return dq.WideEvaluator(env.d, env.error_model, window=env.volume_depth, chunk=env.n_envs, device=env.device)


def _dev(torch, env, a):
    return torch.from_numpy(np.array(a, dtype=np.int32)).to(env.device)       # (a copy: the replay's arrays are read-only)


def _done_bits(env, state):
    return (state[:, 5 * ((env.d ** 2 + 63) // 64) + 1 + 2 * env.legal_words] >> np.uint64(32)) & np.uint64(1)


def _select(env, ev, triple, **kw):
    return env.uf_select_wide(ev, weights=tuple(triple[:2]), correlated=int(triple[2]), **kw)


@pytest.mark.parametrize("name", list(R.CONFIGS))
def test_correlated_select_is_the_rule_in_lockstep_with_the_oracle(dq, torch_mod, name):
    """Every record of every run under the run's own triple and under the other ones; with w_corr = w_space, and under the X model with any w_corr, the
    actions are dq_envb_uf_select_weighted's; in every DP run some action differs from that launch's.  d15deep asks for the kernel's LDS maximum (d = 15,
    volume_depth 16: 31.9 KB and 1 KB of masks), d15dpy and d5dpy have three action layers."""
    torch = torch_mod
    r = R.replay(name)
    _, n, steps, _ = R.CONFIGS[name]
    triple = R.run_triple(dq, name)
    env = _wide_env(dq, name)
    ev = _evaluator(dq, env)
    try:
        assert env.wide and env.identity_index == r["identity"] and r["triple"] == triple
        assert set(r["other"]) == set(R.others(dq, name)) >= set(R.OTHER_TRIPLES + (R.LIMIT_TRIPLES if env.d == 5 else ()))
        env.reset(write_obs=False)
        assert np.array_equal(_u64(env.legal), r["legal0"])
        out = torch.empty(n, dtype=torch.int32, device=env.device)
        done_seen = differs = 0
        for t in range(steps):
            before = env.export_state()
            assert np.array_equal(_u64(before), r["state"][t]), (name, "state", t)
            for p, want in r["other"].items():                                          # the other triples on the same record
                out.fill_(7)
                got = _select(env, ev, p, out=out).cpu().numpy()
                assert np.array_equal(got, want[t]), (name, p, t, np.flatnonzero(got != want[t])[:8])
                if env.error_model == "X" or p[2] == p[0]:                              # no mask, or a mask that changes no weight: the weighted launch
                    assert np.array_equal(got, env.uf_select_wide(ev, weights=p[:2]).cpu().numpy()), (name, p, t)
            weighted = env.uf_select_wide(ev, weights=triple[:2]).cpu().numpy()
            assert np.array_equal(weighted, r["weighted"][t]), (name, "weighted", t)
            assert np.array_equal(_select(env, ev, triple[:2] + (triple[0],)).cpu().numpy(), weighted), (name, "w_corr = w_space", t)
            out.fill_(7)
            a = _select(env, ev, triple, out=out)
            assert a is out
            got = a.cpu().numpy()
            assert np.array_equal(got, r["action"][t]), (name, "action", t, np.flatnonzero(got != r["action"][t])[:8])
            differs += int((got != weighted).sum())
            done = _done_bits(env, r["state"][t])
            done_seen += int((done != 0).sum())
            assert (got[done != 0] == env.identity_index).all()                         # a done lattice gets the identity
            assert torch.equal(before, env.export_state()), (name, "a call wrote to the record", t)
            env.step(a, auto_reset=True, write_obs=False)
            assert np.array_equal(env.reward.cpu().numpy(), r["reward"][t]), (name, "reward", t)
            assert np.array_equal(env.done.cpu().numpy(), r["done"][t]), (name, "done", t)
            assert np.array_equal(_u64(env.legal), r["legal"][t]), (name, "legal", t)
        assert np.array_equal(_u64(env.export_state()), r["state"][steps])
        R.assert_minimums(name, r["events"])
        assert done_seen == r["events"]["done_visits"] and differs == r["events"]["differ"]
        if name in R.DIFFERING:
            assert differs >= 1, name
        if env.error_model == "X":
            assert differs == 0 and done_seen >= 20                                     # the run that covers done lattices
    finally:
        ev.close()
        env.close()


@pytest.mark.parametrize("n", [1, 7, 40])
def test_a_per_lattice_array_gives_every_lattice_its_own_triple(dq, torch_mod, n):
    """d = 9, DP, depth 5, 0.004 / 0.04 on sub-batches of 1, 7 and 40 lattices of one batch (ids base .. base + n): a permuted array of four triples equals the
    four uniform launches lattice by lattice -- as a uint8 device tensor [n, 3] used in place, and as per-lattice pairs with one w_corr."""
    torch = torch_mod
    kw = R.CONFIGS["d9dp"][0]
    base = {1: 33, 7: 8, 40: 0}[n]
    env = dq.VectorEnv(n_envs=n, seed=SEED, env_id_base=base, backend="wide", **kw)
    ev = _evaluator(dq, env)
    triples = [(7, 4, 1), (7, 4, 7), (4, 4, 2), (15, 2, 3)]
    which = np.random.default_rng(5).permutation(np.arange(40) % 4)[base:base + n] if n < 40 else np.random.default_rng(5).permutation(np.arange(40) % 4)
    each = np.array([triples[k] for k in which], dtype=np.uint8)
    each_dev = torch.from_numpy(each).to(env.device)
    pairs = np.array([(7, 4), (4, 4), (15, 2), (7, 7)], dtype=np.int64)[np.arange(n) % 4]
    try:
        env.reset(write_obs=False)
        mixed = 0
        for t in range(10):
            uniform = np.stack([_select(env, ev, p).cpu().numpy() for p in triples])
            want = uniform[which, np.arange(n)]
            assert np.array_equal(env.uf_select_wide(ev, weights=each_dev).cpu().numpy(), want), t
            by_pair = {tuple(p): _select(env, ev, tuple(p) + (2,)).cpu().numpy() for p in np.unique(pairs, axis=0).tolist()}
            want2 = np.array([by_pair[tuple(p)][i] for i, p in enumerate(pairs)])
            for form in (pairs, pairs.tolist(), torch.from_numpy(pairs.astype(np.uint8)).to(env.device)):
                assert np.array_equal(env.uf_select_wide(ev, weights=form, correlated=2).cpu().numpy(), want2), t
            mixed += int((uniform[0] != uniform[1]).sum() + (uniform[0] != uniform[2]).sum())
            env.step(_dev(torch, env, uniform[0]), auto_reset=True, write_obs=False)
        if n == 40:
            assert mixed >= n // 2                                                      # (the launches are not copies of one another)
            with pytest.raises(ValueError):
                env.uf_select_wide(ev, weights=each_dev[:32])
            with pytest.raises(ValueError):
                env.uf_select_wide(ev, weights=each_dev.to(torch.int32))
            with pytest.raises(ValueError):
                env.uf_select_wide(ev, weights=each_dev, correlated=1)                  # triples take no w_corr beside them
            with pytest.raises(ValueError):
                env.uf_select_wide(ev, weights=pairs, correlated=5)                     # above the smallest w_space (4)
    finally:
        ev.close()
        env.close()


def test_the_kernel_clamps_a_raw_array_and_the_abi_refuses_a_bad_uniform_triple(dq, torch_mod):
    """Bytes sent through the C ABI directly: the pair is clamped to 1 .. 15 and w_corr to 1 .. w_space; with an array the uniform triple is not read;
    without one a bad uniform triple is DQ_ERR_INVALID before any device work."""
    torch = torch_mod
    L = dq._lib
    env = _wide_env(dq, "d5dp")
    ev = _evaluator(dq, env)
    n = env.n_envs
    raw = torch.tensor([[0, 200, 0], [200, 0, 200], [7, 4, 9], [255, 16, 1]] * (n // 4), dtype=torch.uint8, device=env.device)
    clamped = torch.tensor([[1, 15, 1], [15, 1, 15], [7, 4, 7], [15, 15, 1]] * (n // 4), dtype=torch.uint8, device=env.device)
    out = torch.empty(n, dtype=torch.int32, device=env.device)
    seed = (ctypes.c_uint32 * 2)(*env.seed)
    try:
        env.reset(write_obs=False)
        for t in range(8):
            L.check(env.L.dq_envb_uf_select_correlated(env._h, ev._h, 1, 1, 1, L.ptr(raw), L.ptr(out), env._stream()))
            got = out.cpu().numpy().copy()
            want = env.uf_select_wide(ev, weights=clamped).cpu().numpy()
            assert np.array_equal(got, want), t
            L.check(env.L.dq_envb_uf_select_correlated(env._h, ev._h, 0, 99, 50, L.ptr(raw), L.ptr(out), env._stream()))
            assert np.array_equal(out.cpu().numpy(), want)
            env.step(_dev(torch, env, want), auto_reset=True, write_obs=False)
        for ws, wt, wc in ((0, 1, 1), (1, 16, 1), (4, 2, 0), (4, 2, 5)):
            assert env.L.dq_envb_uf_select_correlated(env._h, ev._h, ws, wt, wc, None, L.ptr(out), env._stream()) == L.DQ_ERR_INVALID
            assert env.L.dq_envb_guided_select_uf_correlated(env._h, ev._h, None, 1.0, 1.0, 0, seed, 0, ws, wt, wc, None, L.ptr(out), None,
                                                             env._stream()) == L.DQ_ERR_INVALID
    finally:
        ev.close()
        env.close()


def test_rates_follow_set_rates_in_a_cache_of_their_own(dq, torch_mod):
    """correlated="rates" after set_rates with per-lattice rates equals the array built by rate_weights_correlated; the weighted cache lives beside it."""
    kw = R.CONFIGS["d9dp"][0]
    n = 48
    env = dq.VectorEnv(n_envs=n, seed=SEED, env_id_base=0, backend="wide", **kw)
    ev = _evaluator(dq, env)
    DW = dq.decoder_wide
    try:
        env.reset(write_obs=False)
        for _ in range(6):                                                              # mid-episode records
            env.step(env.uf_select_wide(ev, correlated="rates"), auto_reset=True, write_obs=False)
        assert env._uf_rate_triples.cpu().tolist() == [[7, 4, 1]] * n and env._uf_rate_weights is None
        env.set_rates(np.repeat([0.004, 0.01, 0.02], 16), np.repeat([0.04, 0.01, 0.004], 16))
        assert env._uf_rate_triples is None
        each = DW.rate_weights_correlated(*env.rates, env.error_model, n)
        assert each.shape == (n, 3) and len({tuple(x) for x in each.tolist()}) >= 2
        got = env.uf_select_wide(ev, correlated="rates").cpu().numpy()
        import torch
        assert np.array_equal(got, env.uf_select_wide(ev, weights=torch.from_numpy(each).to(env.device)).cpu().numpy())
        cached = env._uf_rate_triples
        assert np.array_equal(cached.cpu().numpy(), each)
        weighted = env.uf_select_wide(ev, weights="rates").cpu().numpy()
        assert env._uf_rate_triples is cached and np.array_equal(env._uf_rate_weights.cpu().numpy(), DW.rate_weights(*env.rates, env.error_model, n))
        assert np.array_equal(env.uf_select_wide(ev, weights="rates", correlated="rates").cpu().numpy(), got) and env._uf_rate_triples is cached
        assert (got != weighted).any()
    finally:
        ev.close()
        env.close()


def test_guided_select_with_the_correlated_teacher(dq, torch_mod):
    """Along the d = 9 run: against guided_actions_wide fed the correlated teacher at eps in {0.3, 1}, guide_share in {0, 0.5, 1}, with and without q."""
    torch = torch_mod
    name = "d9dp"
    r = R.replay(name)
    _, n, steps, _ = R.CONFIGS[name]
    triple = r["triple"]
    ckw = dict(weights=triple[:2], correlated=triple[2])
    env = _wide_env(dq, name)
    ev = _evaluator(dq, env)
    gen = torch.Generator(device="cuda").manual_seed(29)
    seen = dict(guided=0, uniform=0, greedy=0, teacher_differs=0)
    out = torch.empty(n, dtype=torch.int32, device=env.device)
    flag = torch.empty(n, dtype=torch.uint8, device=env.device)

    def guided(t, q, eps, share, masked, **kw):
        out.fill_(7)
        flag.fill_(7)
        assert env.guided_select_wide(ev, t, q=q, eps=eps, guide_share=share, masked_greedy=masked, out=out, out_guided=flag, **kw) is out
        return out.cpu().numpy().copy(), flag.cpu().numpy().copy()

    try:
        env.reset(write_obs=False)
        for t in range(steps):
            teacher = r["action"][t]
            q = torch.randn((n, env.num_actions), device="cuda", generator=gen)
            q[:, 5] = q[:, 2]                                                           # ties
            legal = env.legal.cpu().numpy()
            before = env.export_state()
            for qq in (q, None):
                for eps in (0.3, 1.0):
                    for share in (0.0, 0.5, 1.0):
                        masked = share == 0.5
                        a, g = guided(t, qq, eps, share, masked, **ckw)
                        wa, wg = dq.guided_actions_wide(None if qq is None else qq.cpu().numpy(), legal, teacher, eps, share, masked, SEED, 0, t)
                        assert np.array_equal(a, wa) and np.array_equal(g, wg), (t, qq is None, eps, share)
                        if share == 0.0:                                                # select_actions' bits, nobody guided
                            sa = env.select_actions(t, q=qq, eps=eps, masked_greedy=masked) if qq is not None else env.select_actions(t)
                            assert np.array_equal(a, sa.cpu().numpy()) and not g.any(), (t, eps)
                        if share == 1.0 and (eps == 1.0 or qq is None):                  # the correlated select's bits, everybody guided
                            assert np.array_equal(a, teacher) and (g == 1).all(), (t, eps)
                        if qq is not None and eps == 0.3 and share == 0.5:
                            _, explore = dq.guided_actions_wide(qq.cpu().numpy(), legal, teacher, eps, 1.0, masked, SEED, 0, t)
                            seen["guided"] += int(wg.sum())
                            seen["uniform"] += int((explore & ~wg.astype(bool)).sum())
                            seen["greedy"] += int((explore == 0).sum())
                            # the weighted teacher's flags are the same, its actions those of the weighted rule
                            ua, ug = guided(t, qq, eps, 1.0, masked, weights=triple[:2])
                            ca, _ = guided(t, qq, eps, 1.0, masked, **ckw)
                            assert np.array_equal(ua[ug == 1], r["weighted"][t][ug == 1])
                            seen["teacher_differs"] += int((ua != ca).sum())
            assert np.array_equal(guided(t, q, 1.0, 1.0, False, correlated="rates")[0], teacher)       # the handle's rates give this run's triple
            assert torch.equal(before, env.export_state())
            env.step(_dev(torch, env, teacher), auto_reset=True, write_obs=False)
        assert min(seen["guided"], seen["uniform"], seen["greedy"]) >= n and seen["teacher_differs"] >= 5, seen
    finally:
        ev.close()
        env.close()


D5 = dict(d=5, error_model="DP", use_Y=False, volume_depth=5)


def test_the_error_rate_sweep_of_the_correlated_agent_equals_one_test_per_rate(dq, torch_mod):
    """d = 5 wide, DP, depth 5, two blocks of 16 lattices at (0.012, 0.012) and (0.02, 0.06), whose triples differ: the sweep's histories are those of one
    test() per rate on an environment of the block's ids at the block's rates."""
    rates, meas, m, nb = [0.012, 0.02], [0.012, 0.06], 16, 24
    triples = [dq.uf_weights_correlated(p, q, "DP") for p, q in zip(rates, meas)]
    assert triples[0] != triples[1] and all(t[2] == 1 < t[0] for t in triples)
    env = dq.VectorEnv(n_envs=2 * m, seed=SEED, env_id_base=40, backend="wide", p_phys=0.01, p_meas=0.01, **D5)
    agent = dq.WideUnionFindAgent(correlated="rates")
    try:
        res = agent.test_error_rates(env, rates, nb_episodes=nb, p_meas=meas, verbose=0, nb_max_episode_steps=100000)
        assert list(res) == rates and env.p_phys == 0.01 and env.p_meas == 0.01          # previous rates restored
        assert agent.last_weights == sorted(triples) and agent.last_inexact_steps == 0
        for k, (p, q) in enumerate(zip(rates, meas)):
            sub = dq.VectorEnv(n_envs=m, seed=SEED, env_id_base=40 + k * m, backend="wide", p_phys=p, p_meas=q, **D5)
            try:
                one = dq.WideUnionFindAgent(correlated="rates")
                h = one.test(sub, nb_episodes=nb, verbose=0, nb_max_episode_steps=100000)
                assert one.last_weights == triples[k]
                assert h.history == res[p].history, (k, p)
                assert len(h.history["episode_lifetime"]) == nb
            finally:
                sub.close()
    finally:
        env.close()


def _agent(dq, env, policy, warmup, limit):
    model = dq.build_convolutional_nn(C_LAYERS, FF_LAYERS, env.obs_shape, env.num_actions)
    agent = dq.DQNAgent(model=model, nb_actions=env.num_actions, memory=dq.SequentialMemory(limit=limit, window_length=1), nb_steps_warmup=warmup,
                        target_model_update=512, policy=policy, test_policy=dq.GreedyQPolicy(masked_greedy=True), gamma=0.99,
                        enable_dueling_network=True, batch_size=32, seed=(1, 2))
    agent.compile(dq.Adam(lr=1e-4))
    return agent


def test_fit_and_the_guided_step_with_the_correlated_guide(dq, torch_mod):
    """A wide d = 5 core, DP, depth 5, 0.004 / 0.04, 32 lattices, eps 1, guide_share 0.5, warm-up 64 steps, 8 vector steps of fit: last_guided_steps > 0 and
    the ring's actions, rewards and done flags are those of a twin environment driven by guided_select_wide(correlated="rates") + step.  Then three direct
    guided_act_and_step_wide(weights=(7, 4), correlated=2) steps on the same core against the twin's guided_select_wide followed by step."""
    torch = torch_mod
    cfg = dict(D5, p_phys=0.004, p_meas=0.04)
    n, steps = 32, 8
    env = dq.VectorEnv(n_envs=n, seed=SEED, backend="wide", **cfg)
    assert env.wide
    guide = dq.WideUnionFindAgent(correlated="rates")
    agent = _agent(dq, env, dq.EpsGreedyQPolicy(eps=1.0, masked_greedy=True, guide=guide, guide_share=0.5), warmup=64, limit=n * 40)
    agent.fit(env, nb_steps=n * steps, verbose=0, episode_averaging_length=50, success_threshold=None, stopping_patience=None, min_nb_steps=0,
              single_cycle=False)
    core = agent._core
    assert core._wide and core.vector_steps == steps and agent.step == n * steps
    assert 0 < agent.last_guided_steps < n * steps
    twin = dq.VectorEnv(n_envs=n, seed=SEED, backend="wide", **cfg)
    ev = _evaluator(dq, twin)
    flag = torch.empty(n, dtype=torch.uint8, device=twin.device)
    try:
        twin.reset()
        guided = differs = 0
        for t in range(steps):
            a = twin.guided_select_wide(ev, t, eps=1.0, guide_share=0.5, out_guided=flag, correlated="rates")
            assert torch.equal(core.ring.action[t], a), t
            guided += int(flag.sum())
            differs += int((twin.uf_select_wide(ev, correlated="rates") != twin.uf_select_wide(ev, weights="rates")).sum())
            twin.step(a, auto_reset=True)
            assert torch.equal(core.ring.reward[t], twin.reward) and torch.equal(core.ring.terminal[t], twin.done), t
        assert guided == agent.last_guided_steps
        for t in range(steps, steps + 3):
            cur = core.ring.cur
            assert core.vector_steps == t
            core.guided_act_and_step_wide(ev, 1.0, 0.5, weights=(7, 4), correlated=2)
            a = twin.guided_select_wide(ev, t, eps=1.0, guide_share=0.5, weights=(7, 4), correlated=2)
            differs += int((twin.uf_select_wide(ev, weights=(7, 4), correlated=2) != twin.uf_select_wide(ev, weights=(7, 4))).sum())
            twin.step(a, auto_reset=True)
            assert torch.equal(core.ring.action[cur], a), t
            assert torch.equal(core.ring.reward[cur], twin.reward) and torch.equal(core.ring.terminal[cur], twin.done), t
        assert differs >= 1                                                             # (the correlated teacher is not the weighted one on this run)
    finally:
        ev.close()
        twin.close()
        env.close()


def test_correlated_environment_launches_leave_the_other_launches_alone(dq, torch_mod):
    """One decoder handle: the unweighted and weighted selects, and the unweighted, weighted and correlated stream decodes, give the same bits before and
    after correlated environment launches (whose LDS tail the other kernels do not have)."""
    torch = torch_mod
    name = "d9dp"
    env = _wide_env(dq, name)
    n, d, depth = 64, env.d, env.volume_depth
    ev = dq.WideEvaluator(d, env.error_model, window=depth, chunk=n, device=env.device)     # (its chunk does not bound n_envs)
    # 64 DP volumes at 0.02 / 0.02 from the handle's own sampler (lattice ids 100 ..): the three stream decodes differ on most of them
    syn = torch.empty((n, depth, d + 1, d + 1), dtype=torch.uint8, device=env.device)
    hid, triv = torch.empty((n, d * d), dtype=torch.uint8, device=env.device), torch.empty(n, dtype=torch.uint8, device=env.device)
    ev.run_into(n, depth, depth, 100, (5, 6), 0.02, 0.02, hid, triv, torch.empty((n, d, d), dtype=torch.uint8, device=env.device), syndromes=syn)

    def streams():
        out = []
        for w in (None, (7, 4), (7, 4, 1)):
            frame = torch.full((n, d, d), 7, dtype=torch.uint8, device=env.device)
            ev.decode_into(syn, n, depth, depth, frame, **({} if w is None else dict(weights=w)))
            out.append(frame)
        return out

    try:
        env.reset(write_obs=False)
        for _ in range(5):
            env.step(env.uf_select_wide(ev), auto_reset=True, write_obs=False)
        before = [env.uf_select_wide(ev).clone(), env.uf_select_wide(ev, weights=(7, 4)).clone()] + streams()
        assert len({tuple(x.flatten().tolist()) for x in before[2:]}) == 3               # (the three stream decodes are not copies of one another)
        for p in ((7, 4, 1), (15, 15, 1), (4, 4, 4)):
            _select(env, ev, p)
            env.guided_select_wide(ev, 0, weights=p[:2], correlated=p[2])
        after = [env.uf_select_wide(ev), env.uf_select_wide(ev, weights=(7, 4))] + streams()
        assert all(torch.equal(x, y) for x, y in zip(before, after))
    finally:
        ev.close()
        env.close()
