"""The weighted union-find decoder as a policy and a teacher of the wide environment on the device (csrc/env_wide_uf.hip: env_wide_uf_kernel<true>,
env_wide_guided_uf_kernel<true>; VectorEnv.uf_select_wide / guided_select_wide(weights=); decoder_wide.WideUnionFindAgent(weights=);
DQNCore.guided_act_and_step_wide(weights=); DQNAgent.decode_benchmark_wide(weights=)).  The reference is weighted_env_uf_ref.replay: the
C oracle environment played by tests/weighted_uf_ref.decode -- which grows in unit steps where the device jumps -- + decoder.frame_to_actions, computed once per
configuration; the device environment runs in lockstep with it, and on every record of a run the other weight pairs are launched too: a select writes
nothing, so they cost nothing in trajectory.  Actions are compared bit for bit."""
import ctypes

import numpy as np
import pytest

import weighted_env_uf_ref as R
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
    kw, n_all, _ = R.CONFIGS[name]
    return dq.VectorEnv(n_envs=n_all if n is None else n, seed=SEED, env_id_base=base, backend="wide", **kw)


def _evaluator(dq, env):
    return dq.WideEvaluator(env.d, env.error_model, window=env.volume_depth, chunk=env.n_envs, device=env.device)


def _dev(torch, env, a):
    return torch.from_numpy(np.array(a, dtype=np.int32)).to(env.device)       # (a copy: the replay's arrays are read-only)


def _done_bits(env, state):
    return (state[:, 5 * ((env.d ** 2 + 63) // 64) + 1 + 2 * env.legal_words] >> np.uint64(32)) & np.uint64(1)


@pytest.mark.parametrize("name", list(R.CONFIGS))
def test_weighted_select_is_the_rule_in_lockstep_with_the_oracle(dq, torch_mod, name):
    """d15deep asks for the kernel's LDS maximum (d = 15, volume_depth 16: 31.9 KB), d15dpy has three action layers (676 actions)."""
    torch = torch_mod
    r = R.replay(name)
    _, n, steps = R.CONFIGS[name]
    pair = R.rate_pair(dq, name)
    env = _wide_env(dq, name)
    ev = _evaluator(dq, env)
    try:
        assert env.wide and env.identity_index == r["identity"] and r["pair"] == pair
        assert set(r["other"]) == set(R.OTHER_PAIRS + (R.LIMIT_PAIRS if env.d == 5 else ()))
        env.reset(write_obs=False)
        assert np.array_equal(_u64(env.legal), r["legal0"])
        out = torch.empty(n, dtype=torch.int32, device=env.device)
        done_seen = 0
        for t in range(steps):
            before = env.export_state()
            assert np.array_equal(_u64(before), r["state"][t]), (name, "state", t)
            for p, want in r["other"].items():                                          # the other pairs on the same record
                out.fill_(7)
                got = env.uf_select_wide(ev, out=out, weights=p).cpu().numpy()
                assert np.array_equal(got, want[t]), (name, p, t, np.flatnonzero(got != want[t])[:8])
            out.fill_(7)
            a = env.uf_select_wide(ev, out=out, weights=pair)
            assert a is out
            got = a.cpu().numpy()
            assert np.array_equal(got, r["action"][t]), (name, "action", t, np.flatnonzero(got != r["action"][t])[:8])
            done = _done_bits(env, r["state"][t])
            done_seen += int((done != 0).sum())
            assert (got[done != 0] == env.identity_index).all()                         # a done lattice gets the identity under weights
            assert torch.equal(before, env.export_state()), (name, "a call wrote to the record", t)
            env.step(a, auto_reset=True, write_obs=False)
            assert np.array_equal(env.reward.cpu().numpy(), r["reward"][t]), (name, "reward", t)
            assert np.array_equal(env.done.cpu().numpy(), r["done"][t]), (name, "done", t)
            assert np.array_equal(_u64(env.legal), r["legal"][t]), (name, "legal", t)
        assert np.array_equal(_u64(env.export_state()), r["state"][steps])
        R.assert_minimums(name, r["events"])
        assert done_seen == r["events"]["done_visits"]
        if name == "d5x":
            assert done_seen >= 20                                                      # the run that covers done lattices
    finally:
        ev.close()
        env.close()


@pytest.mark.parametrize("name", ["d9dp", "d15dpy"])
def test_unit_weights_are_the_unweighted_launch_and_leave_it_alone(dq, torch_mod, name):
    """Along the weighted run: the weighted entry at (1, 1) equals dq_envb_uf_select on every record, and the unweighted results before and after weighted
    calls on the same handle are the same bits."""
    torch = torch_mod
    r = R.replay(name)
    _, n, steps = R.CONFIGS[name]
    env = _wide_env(dq, name)
    ev = _evaluator(dq, env)
    try:
        env.reset(write_obs=False)
        flips = 0
        for t in range(steps):
            plain = env.uf_select_wide(ev).cpu().numpy()
            unit = env.uf_select_wide(ev, weights=(1, 1)).cpu().numpy()
            assert np.array_equal(unit, plain) and np.array_equal(plain, r["other"][(1, 1)][t]), (name, t)
            for p in ((7, 4), (1, 15), (15, 15)):
                env.uf_select_wide(ev, weights=p)
            assert np.array_equal(env.uf_select_wide(ev).cpu().numpy(), plain), (name, t)
            flips += int((plain != env.identity_index).sum())
            env.step(_dev(torch, env, r["action"][t]), auto_reset=True, write_obs=False)
        assert flips >= n * steps // 4
    finally:
        ev.close()
        env.close()


def test_a_per_lattice_array_gives_every_lattice_its_own_pair(dq, torch_mod):
    """d = 9, DP, depth 5, 0.004 / 0.04 on 40 lattices (no multiple of 64): a permuted array of three pairs equals the three uniform launches lattice by
    lattice, as a numpy array, as nested lists and as a uint8 device tensor used in place."""
    torch = torch_mod
    kw = R.CONFIGS["d9dp"][0]
    n, steps = 40, 10
    env = dq.VectorEnv(n_envs=n, seed=SEED, env_id_base=0, backend="wide", **kw)
    ev = _evaluator(dq, env)
    pairs = [(7, 4), (1, 1), (2, 3)]
    which = np.random.default_rng(5).permutation(np.arange(n) % 3)
    each = np.array([pairs[k] for k in which], dtype=np.int64)
    each_dev = torch.from_numpy(each.astype(np.uint8)).to(env.device)
    try:
        env.reset(write_obs=False)
        mixed = 0
        for t in range(steps):
            uniform = np.stack([env.uf_select_wide(ev, weights=p).cpu().numpy() for p in pairs])
            want = uniform[which, np.arange(n)]
            for form in (each, each.tolist(), each_dev):
                assert np.array_equal(env.uf_select_wide(ev, weights=form).cpu().numpy(), want), t
            mixed += int((uniform[0] != uniform[1]).sum() + (uniform[1] != uniform[2]).sum())
            env.step(_dev(torch, env, uniform[0]), auto_reset=True, write_obs=False)
        assert mixed >= n                                                               # (the three launches are not copies of one another)
        with pytest.raises(ValueError):
            env.uf_select_wide(ev, weights=each[:32])
        with pytest.raises(ValueError):
            env.uf_select_wide(ev, weights=each_dev[:32])
        with pytest.raises(ValueError):
            env.uf_select_wide(ev, weights=each_dev.to(torch.int32))
    finally:
        ev.close()
        env.close()


def test_rates_follow_set_rates(dq, torch_mod):
    """weights="rates" after set_rates with per-lattice rates equals the array built by rate_weights, and follows a second set_rates."""
    torch = torch_mod
    kw = R.CONFIGS["d9dp"][0]
    n = 48
    env = dq.VectorEnv(n_envs=n, seed=SEED, env_id_base=0, backend="wide", **kw)
    ev = _evaluator(dq, env)
    DW = dq.decoder_wide
    try:
        env.reset(write_obs=False)
        for _ in range(6):                                                              # mid-episode records
            env.step(env.uf_select_wide(ev, weights="rates"), auto_reset=True, write_obs=False)
        assert env._uf_rate_weights.cpu().tolist() == [list(DW.uf_weights(0.004, 0.04, "DP"))] * n
        seen = []
        for ph, pm in ((np.repeat([0.004, 0.01, 0.02], 16), np.repeat([0.04, 0.01, 0.004], 16)), (np.repeat([0.02, 0.004], 24), 0.03)):
            env.set_rates(ph, pm)
            assert env._uf_rate_weights is None
            each = DW.rate_weights(*env.rates, env.error_model, n)
            assert each.shape == (n, 2) and len({tuple(x) for x in each.tolist()}) >= 2
            got = env.uf_select_wide(ev, weights="rates").cpu().numpy()
            assert np.array_equal(got, env.uf_select_wide(ev, weights=each).cpu().numpy())
            assert np.array_equal(env._uf_rate_weights.cpu().numpy(), each)
            cached = env._uf_rate_weights
            env.uf_select_wide(ev, weights="rates")
            assert env._uf_rate_weights is cached                                       # uploaded once per set_rates
            seen.append(each)
        assert not np.array_equal(seen[0], seen[1])
    finally:
        ev.close()
        env.close()


def test_the_kernel_clamps_a_raw_array(dq, torch_mod):
    """Bytes 0 and 200, sent through the C ABI directly, decode as 1 and 15."""
    torch = torch_mod
    L = dq._lib
    env = _wide_env(dq, "d5x")
    ev = _evaluator(dq, env)
    n = env.n_envs
    raw = torch.tensor([[0, 200], [200, 0], [0, 0], [255, 16]] * (n // 4), dtype=torch.uint8, device=env.device)
    clamped = [[1, 15], [15, 1], [1, 1], [15, 15]] * (n // 4)
    out = torch.empty(n, dtype=torch.int32, device=env.device)
    try:
        env.reset(write_obs=False)
        differ = 0
        for t in range(12):
            L.check(env.L.dq_envb_uf_select_weighted(env._h, ev._h, 1, 1, L.ptr(raw), L.ptr(out), env._stream()))
            got = out.cpu().numpy().copy()
            want = env.uf_select_wide(ev, weights=clamped).cpu().numpy()
            assert np.array_equal(got, want), t
            differ += int((want != env.uf_select_wide(ev).cpu().numpy()).sum())
            # with an array the uniform pair is not read; without one it is refused before any device work
            L.check(env.L.dq_envb_uf_select_weighted(env._h, ev._h, 0, 99, L.ptr(raw), L.ptr(out), env._stream()))
            assert np.array_equal(out.cpu().numpy(), want)
            env.step(_dev(torch, env, want), auto_reset=True, write_obs=False)
        assert differ >= 10                                                             # (the clamped pairs matter on these records)
        for ws, wt in ((0, 1), (1, 16)):
            assert env.L.dq_envb_uf_select_weighted(env._h, ev._h, ws, wt, None, L.ptr(out), env._stream()) == L.DQ_ERR_INVALID
            seed = (ctypes.c_uint32 * 2)(*env.seed)
            assert env.L.dq_envb_guided_select_uf_weighted(env._h, ev._h, None, 1.0, 1.0, 0, seed, 0, ws, wt, None, L.ptr(out), None,
                                                           env._stream()) == L.DQ_ERR_INVALID
    finally:
        ev.close()
        env.close()


def test_guided_select_with_the_weighted_teacher(dq, torch_mod):
    """Along the d = 9 run: against guided_actions_wide fed the weighted teacher at eps in {0.3, 1}, guide_share in {0, 0.5, 1}, with and without q."""
    torch = torch_mod
    name = "d9dp"
    r = R.replay(name)
    _, n, steps = R.CONFIGS[name]
    pair = r["pair"]
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
            assert np.array_equal(env.uf_select_wide(ev, weights=pair).cpu().numpy(), teacher)
            for qq in (q, None):
                for eps in (0.3, 1.0):
                    for share in (0.0, 0.5, 1.0):
                        masked = share == 0.5
                        a, g = guided(t, qq, eps, share, masked, weights=pair)
                        wa, wg = dq.guided_actions_wide(None if qq is None else qq.cpu().numpy(), legal, teacher, eps, share, masked, SEED, 0, t)
                        assert np.array_equal(a, wa) and np.array_equal(g, wg), (t, qq is None, eps, share)
                        if share == 0.0:                                                # select_actions' bits, nobody guided
                            sa = env.select_actions(t, q=qq, eps=eps, masked_greedy=masked) if qq is not None else env.select_actions(t)
                            assert np.array_equal(a, sa.cpu().numpy()) and not g.any(), (t, eps)
                        if share == 1.0 and (eps == 1.0 or qq is None):                  # weighted uf_select_wide's bits, everybody guided
                            assert np.array_equal(a, teacher) and (g == 1).all(), (t, eps)
                        if qq is not None and eps == 0.3 and share == 0.5:
                            _, explore = dq.guided_actions_wide(qq.cpu().numpy(), legal, teacher, eps, 1.0, masked, SEED, 0, t)
                            seen["guided"] += int(wg.sum())
                            seen["uniform"] += int((explore & ~wg.astype(bool)).sum())
                            seen["greedy"] += int((explore == 0).sum())
                            # the unweighted teacher's flags are the same, its actions those of the unit rule
                            ua, ug = guided(t, qq, eps, share, masked)
                            assert np.array_equal(ug, g)
                            seen["teacher_differs"] += int((ua != a).sum())
            assert np.array_equal(guided(t, q, 1.0, 1.0, False, weights="rates")[0], teacher)      # the handle's rates give this run's pair
            assert torch.equal(before, env.export_state())
            env.step(_dev(torch, env, teacher), auto_reset=True, write_obs=False)
        assert min(seen["guided"], seen["uniform"], seen["greedy"]) >= n and seen["teacher_differs"] >= 10, seen
    finally:
        ev.close()
        env.close()


def _agent(dq, env, policy, warmup, limit):
    model = dq.build_convolutional_nn(C_LAYERS, FF_LAYERS, env.obs_shape, env.num_actions)
    agent = dq.DQNAgent(model=model, nb_actions=env.num_actions, memory=dq.SequentialMemory(limit=limit, window_length=1), nb_steps_warmup=warmup,
                        target_model_update=512, policy=policy, test_policy=dq.GreedyQPolicy(masked_greedy=True), gamma=0.99,
                        enable_dueling_network=True, batch_size=32, seed=(1, 2))
    agent.compile(dq.Adam(lr=1e-4))
    return agent


def test_the_weighted_agent_returns_what_the_unweighted_agent_returns(dq, torch_mod):
    """d = 9: under the X model with p_meas = p_phys "rates" is (1, 1), so the whole history -- keys, record order, values -- is the unweighted agent's; at
    0.004 / 0.04 under DP the keys and the episode count are, and the pair used is reported."""
    cfg = dict(d=9, error_model="X", use_Y=False, volume_depth=5, p_phys=0.012, p_meas=0.012)
    env, twin = (dq.VectorEnv(n_envs=8, seed=SEED, **cfg) for _ in range(2))              # (a second test() on one handle plays other episodes)
    noisy = dq.VectorEnv(n_envs=8, seed=SEED, **R.CONFIGS["d9dp"][0])
    try:
        plain, weighted = dq.WideUnionFindAgent(), dq.WideUnionFindAgent(weights="rates")
        h0 = plain.test(env, nb_episodes=8, verbose=0, nb_max_episode_steps=100000)
        h1 = weighted.test(twin, nb_episodes=8, verbose=0, nb_max_episode_steps=100000)
        assert weighted.last_weights == (1, 1) and plain.last_weights is None
        assert list(h1.history) == list(h0.history) and all(list(h1.history[k]) == list(h0.history[k]) for k in h0.history)
        assert len(h0.history["episode_lifetime"]) == 8 and weighted.last_vector_steps == plain.last_vector_steps
        h2 = weighted.test(noisy, nb_episodes=8, verbose=0, nb_max_episode_steps=100000)
        assert list(h2.history) == list(h0.history) and len(h2.history["episode_lifetime"]) == 8
        assert weighted.last_weights == dq.uf_weights(0.004, 0.04, "DP") == (7, 4) and weighted.last_inexact_steps == 0
        out = weighted.test_error_rates(noisy, [0.004, 0.012], nb_episodes=2, p_meas=0.04, verbose=0, nb_max_episode_steps=100000)
        assert list(out) == [0.004, 0.012] and all(len(h.history["episode_lifetime"]) == 2 for h in out.values())
        assert weighted.last_weights == sorted({dq.uf_weights(0.004, 0.04, "DP"), dq.uf_weights(0.012, 0.04, "DP")})
        assert noisy.p_phys == 0.004 and noisy.p_meas == 0.04                           # the previous rates are restored
    finally:
        env.close()
        twin.close()
        noisy.close()


def _records_of(env, state):
    """COracleWideEnv.export()'s fields of VectorEnv.export_state() rows: done, the completed set as a mask, the volume as one integer per round."""
    W_, LW, depth = (env.d ** 2 + 63) // 64, env.legal_words, env.volume_depth
    o_comp = 5 * W_ + 1
    o_meta = o_comp + 2 * LW
    out = []
    for row in state:
        words = [int(x) for x in row]
        out.append(dict(done=(words[o_meta] >> 32) & 1, completed=sum(words[o_comp + k] << (64 * k) for k in range(LW)),
                        volume=[sum(words[o_meta + 1 + t * W_ + k] << (64 * k) for k in range(W_)) for t in range(depth)]))
    return out


def test_fit_with_the_weighted_guide_records_the_weighted_teachers_actions(dq, torch_mod):
    """d = 9, DP, depth 5, 0.004 / 0.04, 32 lattices, eps 1, share 1, warm-up 64 steps, 256 steps (8 vector steps): the ring's actions are those of a twin
    environment driven by uf_select_wide(weights="rates"), and on the twin's exported state they are the weighted rule's."""
    torch = torch_mod
    cfg = R.CONFIGS["d9dp"][0]
    n, steps = 32, 8
    env = dq.VectorEnv(n_envs=n, seed=SEED, **cfg)
    assert env.wide
    guide = dq.WideUnionFindAgent(weights="rates")
    agent = _agent(dq, env, dq.EpsGreedyQPolicy(eps=1.0, masked_greedy=True, guide=guide, guide_share=1.0), warmup=64, limit=n * 40)
    agent.fit(env, nb_steps=n * steps, verbose=0, episode_averaging_length=50, success_threshold=None, stopping_patience=None, min_nb_steps=0,
              single_cycle=False)
    core = agent._core
    assert core.vector_steps == steps and agent.step == n * steps
    assert agent.last_guided_steps == n * steps > 0
    twin = dq.VectorEnv(n_envs=n, seed=SEED, **cfg)
    ev = _evaluator(dq, twin)
    pair = dq.uf_weights(cfg["p_phys"], cfg["p_meas"], cfg["error_model"])
    try:
        twin.reset()
        differs = 0
        for t in range(steps):
            a = twin.uf_select_wide(ev, weights="rates")
            assert torch.equal(core.ring.action[t], a), t
            differs += int((a != twin.uf_select_wide(ev)).sum())
            if t == steps - 2:                                                          # mid-run: the rule in numpy on the exported state
                recs = _records_of(twin, _u64(twin.export_state()))
                want = np.array([R.rule_action(dq, cfg, rec, pair) for rec in recs], dtype=np.int32)
                assert np.array_equal(a.cpu().numpy(), want) and (want != twin.identity_index).any()
            twin.step(a, auto_reset=True)
            assert torch.equal(core.ring.reward[t], twin.reward) and torch.equal(core.ring.terminal[t], twin.done), t
        assert differs >= 1                                                             # (the weighted teacher is not the unit one on this run)
    finally:
        ev.close()
        twin.close()
        env.close()


def test_decode_benchmark_weights_the_union_find_row_only(dq, torch_mod):
    """d = 9, DP, depth 5, 256 volumes per block.  rates=[...] keys its blocks by distinct physical rates, so the two blocks of one call are (0.004, 0.04)
    and (0.005, 0.005); the cell (0.004, 0.004) is scored in a call of its own.  The union-find row equals
    memory_experiment_wide(rounds = window = commit = depth, weights="rates") on the same ids; the agent's row equals the call without weights."""
    cfg = dict(d=9, error_model="DP", use_Y=False, volume_depth=5)
    env = dq.VectorEnv(n_envs=2, p_phys=0.004, p_meas=0.04, seed=(5, 6), **cfg)
    agent = _agent(dq, env, dq.GreedyQPolicy(masked_greedy=True), warmup=100, limit=64)
    n, seed, base = 256, (0xC0DE, 0x5EED), 4096
    try:
        kw = dict(rates=[0.004, 0.005], p_meas=[0.04, 0.005], seed=seed, env_id_base=base, baseline="union_find")
        mine_w, uf_w = agent.decode_benchmark_wide(env, n, weights="rates", **kw)
        mine_0, uf_0 = agent.decode_benchmark_wide(env, n, **kw)
        want = dq.memory_experiment_wide((9, "DP"), n, rounds=5, window=5, commit=5, rates=[0.004, 0.005], p_meas=[0.04, 0.005], seed=seed, env_id_base=base,
                                         weights="rates")
        for rate, pm in ((0.004, 0.04), (0.005, 0.005)):
            assert uf_w[rate].counters == want[rate].counters and uf_w[rate].weights == want[rate].weights == dq.uf_weights(rate, pm, "DP"), rate
            assert mine_w[rate].counters == mine_0[rate].counters and uf_0[rate].weights is None, rate
        assert uf_w[0.004].weights == (7, 4) != uf_w[0.005].weights
        assert uf_w[0.004].counters != uf_0[0.004].counters                             # (the weights matter on these volumes)
        # the cell (0.004, 0.004), and a uniform pair
        one = dict(p_phys=0.004, p_meas=0.004, seed=seed, env_id_base=base, baseline="union_find")
        for w in ("rates", (3, 2)):
            m1, u1 = agent.decode_benchmark_wide(env, n, weights=w, **one)
            w1 = dq.memory_experiment_wide((9, "DP"), n, rounds=5, window=5, commit=5, p_phys=0.004, p_meas=0.004, seed=seed, env_id_base=base, weights=w)
            assert u1.counters == w1.counters and u1.weights == w1.weights == (dq.uf_weights(0.004, 0.004, "DP") if w == "rates" else w)
            assert m1.counters == agent.decode_benchmark_wide(env, n, **one)[0].counters
        with pytest.raises(ValueError):
            agent.decode_benchmark_wide(env, n, p_phys=0.004, p_meas=0.04, seed=seed, weights="rates")
    finally:
        for name in ("_wide_decoder", "_decoder"):
            dec = getattr(agent, name, None)
            if dec is not None:
                dec.close()
            setattr(agent, name, None)
        env.close()
