"""The union-find decoder as a policy and a teacher of the wide environment on the device (csrc/env_wide_uf.hip: env_wide_uf_kernel,
env_wide_guided_uf_kernel; VectorEnv.uf_select_wide / guided_select_wide; decoder_wide.WideUnionFindAgent; DQNCore.guided_act_and_step_wide; DESIGN.md
section 19).  The reference is test_wide_env_uf_cpu.replay: the C oracle environment played by tests/wide_uf_ref.decode + decoder.frame_to_actions, computed
once per configuration; the device environment runs in lockstep with it (its exported state equals the oracle's in front of every step, so the rule was
computed on the device's own state), and every configuration asserts the events it exists to exercise."""
import numpy as np
import pytest

from test_wide_env_uf_cpu import CONFIGS, SEED, assert_minimums, env_kwargs, replay

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
    kw, n_all, _ = env_kwargs(name)
    return dq.VectorEnv(n_envs=n_all if n is None else n, seed=SEED, env_id_base=base, backend="wide", **kw)


def _evaluator(dq, env, window=None):
    return dq.WideEvaluator(env.d, env.error_model, window=env.volume_depth if window is None else window, chunk=env.n_envs, device=env.device)


def _dev(torch, env, a):
    return torch.from_numpy(np.array(a, dtype=np.int32)).to(env.device)       # (a copy: the replay's arrays are read-only)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_select_is_the_rule_in_lockstep_with_the_oracle(dq, torch_mod, name):
    torch = torch_mod
    r = replay(name)
    _, n, steps = env_kwargs(name)
    env = _wide_env(dq, name)
    ev = _evaluator(dq, env)
    try:
        assert env.wide and env.identity_index == r["identity"]
        env.reset(write_obs=False)
        assert np.array_equal(_u64(env.legal), r["legal0"])
        out = torch.empty(n, dtype=torch.int32, device=env.device)
        for t in range(steps):
            before = env.export_state()
            assert np.array_equal(_u64(before), r["state"][t]), (name, "state", t)
            out.fill_(7)
            a = env.uf_select_wide(ev, out=out)
            assert a is out
            got = a.cpu().numpy()
            assert np.array_equal(got, r["action"][t]), (name, "action", t, np.flatnonzero(got != r["action"][t])[:8])
            done = (r["state"][t][:, 5 * ((env.d ** 2 + 63) // 64) + 1 + 2 * env.legal_words] >> np.uint64(32)) & np.uint64(1)
            assert (got[done != 0] == env.identity_index).all()
            assert torch.equal(before, env.export_state()), (name, "the call wrote to the record", t)
            env.step(a, auto_reset=True, write_obs=False)
            assert np.array_equal(env.reward.cpu().numpy(), r["reward"][t]), (name, "reward", t)
            assert np.array_equal(env.done.cpu().numpy(), r["done"][t]), (name, "done", t)
            assert np.array_equal(_u64(env.legal), r["legal"][t]), (name, "legal", t)
        assert np.array_equal(_u64(env.export_state()), r["state"][steps])
        assert_minimums(name, r["events"])
    finally:
        ev.close()
        env.close()


D3 = dict(d=3, error_model="DP", use_Y=False, volume_depth=3, p_phys=0.01, p_meas=0.01)


@pytest.mark.parametrize("name", ["d5wide", "d3dp"])
def test_the_narrow_union_find_policy_gives_the_same_actions(dq, torch_mod, name):
    """d <= 7: the narrow environment with the same seed, played by match_select(method="union_find"), takes the same action on every lattice at every step."""
    kw, n, steps = env_kwargs(name) if name in CONFIGS else (D3, 64, 40)
    wide = dq.VectorEnv(n_envs=n, seed=SEED, backend="wide", **kw)
    narrow = dq.VectorEnv(n_envs=n, seed=SEED, **kw)
    ev = _evaluator(dq, wide)
    nev = dq.decoder.Evaluator(kw["d"], kw["error_model"], kw["use_Y"], kw["volume_depth"], chunk=n, device=narrow.device)
    try:
        assert wide.wide and not narrow.wide
        wide.reset(write_obs=False)
        narrow.reset(write_obs=False)
        flips = dones = 0
        for t in range(steps):
            a = wide.uf_select_wide(ev)
            b = narrow.match_select(nev, method="union_find")
            assert np.array_equal(a.cpu().numpy(), b.cpu().numpy()), (name, t)
            if name in CONFIGS:
                assert np.array_equal(a.cpu().numpy(), replay(name)["action"][t])
            wide.step(a, auto_reset=True, write_obs=False)
            narrow.step(b, auto_reset=True, write_obs=False)
            assert np.array_equal(wide.done.cpu().numpy(), narrow.done.cpu().numpy()) and np.array_equal(wide.reward.cpu().numpy(), narrow.reward.cpu().numpy())
            flips += int((a != wide.identity_index).sum())
            dones += int(wide.done.sum())
        assert flips >= n * steps // 4 and dones >= 1
    finally:
        ev.close()
        nev.close()
        wide.close()
        narrow.close()


@pytest.mark.parametrize("name", ["d9dp", "d15dpy", "d5wide"])
def test_guided_select_along_the_select_run(dq, torch_mod, name):
    torch = torch_mod
    r = replay(name)
    kw, n, steps = env_kwargs(name)
    half = n // 2
    env = _wide_env(dq, name)
    parts = [_wide_env(dq, name, n=half, base=b) for b in (0, half)]
    narrow = dq.VectorEnv(n_envs=n, seed=SEED, **kw) if name == "d5wide" else None
    ev = _evaluator(dq, env)
    nev = dq.decoder.Evaluator(kw["d"], kw["error_model"], kw["use_Y"], kw["volume_depth"], chunk=n, device=env.device) if narrow is not None else None
    gen = torch.Generator(device="cuda").manual_seed(23)
    seen = dict(guided=0, uniform=0, greedy=0)
    try:
        for e in [env] + parts + ([narrow] if narrow is not None else []):
            e.reset(write_obs=False)
        out = torch.empty(n, dtype=torch.int32, device=env.device)
        flag = torch.empty(n, dtype=torch.uint8, device=env.device)

        def guided(t, q, eps, share, masked, e=env, o=None, f=None):
            o, f = (out, flag) if o is None else (o, f)
            o.fill_(7)
            f.fill_(7)
            assert e.guided_select_wide(ev, t, q=q, eps=eps, guide_share=share, masked_greedy=masked, out=o, out_guided=f) is o
            return o.cpu().numpy().copy(), f.cpu().numpy().copy()

        for t in range(steps):
            want = r["action"][t]
            q = torch.randn((n, env.num_actions), device="cuda", generator=gen)
            q[:, 5] = q[:, 2]                                                           # ties
            before = env.export_state()
            # share 0: select_actions, nobody guided
            a, g = guided(t, q, 0.3, 0.0, True)
            assert np.array_equal(a, env.select_actions(t, q=q, eps=0.3, masked_greedy=True).cpu().numpy()) and not g.any(), (name, t)
            # eps 1 / share 1, and no Q at all: the select actions, everybody guided
            for qq, eps in ((q, 1.0), (None, 0.0)):
                a, g = guided(t, qq, eps, 1.0, False)
                assert np.array_equal(a, want) and (g == 1).all(), (name, t)
            # the three branches
            a, g = guided(t, q, 0.5, 0.5, False)
            wa, wg = dq.guided_actions_wide(q.cpu().numpy(), env.legal.cpu().numpy(), want, 0.5, 0.5, False, SEED, 0, t)
            assert np.array_equal(a, wa) and np.array_equal(g, wg), (name, t)
            _, explore = dq.guided_actions_wide(q.cpu().numpy(), env.legal.cpu().numpy(), want, 0.5, 1.0, False, SEED, 0, t)
            seen["guided"] += int(wg.sum())
            seen["uniform"] += int((explore & ~wg.astype(bool)).sum())
            seen["greedy"] += int((explore == 0).sum())
            assert torch.equal(before, env.export_state())
            # two half batches at their own bases
            for p, b in zip(parts, (0, half)):
                pa, pg = guided(t, q[b:b + half].contiguous(), 0.5, 0.5, False, e=p, o=out[:half], f=flag[:half])
                assert np.array_equal(pa, a[b:b + half]) and np.array_equal(pg, g[b:b + half]), (name, t, b)
            if narrow is not None:
                na = narrow.guided_select(nev, t, q=q, eps=0.5, guide_share=0.5, masked_greedy=False, out_guided=flag, method="union_find")
                assert np.array_equal(na.cpu().numpy(), a) and np.array_equal(flag.cpu().numpy(), g), (name, t)
                narrow.step(_dev(torch, narrow, want), auto_reset=True, write_obs=False)
            env.step(_dev(torch, env, want), auto_reset=True, write_obs=False)
            for p, b in zip(parts, (0, half)):
                p.step(_dev(torch, p, want[b:b + half]), auto_reset=True, write_obs=False)
            assert np.array_equal(_u64(env.legal), r["legal"][t])
        assert min(seen.values()) >= n, seen
    finally:
        ev.close()
        if nev is not None:
            nev.close()
        for e in [env] + parts + ([narrow] if narrow is not None else []):
            e.close()


def test_handles(dq, torch_mod):
    """d9hot: blocks of the batch on handles of their own in another order, repeated calls, an evaluator of window 16 serving depth 4, the stream decode on the
    same handle before and after, and pre-filled outputs."""
    torch = torch_mod
    name = "d9hot"
    r = replay(name)
    kw, n, steps = env_kwargs(name)
    env = _wide_env(dq, name)
    bases = (48, 0, 32, 16)
    blocks = [_wide_env(dq, name, n=16, base=b) for b in bases]
    ev, ev16 = _evaluator(dq, env), _evaluator(dq, env, window=16)
    try:
        d = kw["d"]
        rng = np.random.default_rng(3)
        syn = torch.from_numpy((rng.random((n, 4, d + 1, d + 1)) < 0.05).astype(np.uint8)).to(env.device)
        frame0 = torch.empty((n, d, d), dtype=torch.uint8, device=env.device)
        frame1 = torch.full_like(frame0, 7)
        ev16.decode_into(syn, n, 4, 4, frame0)
        for e in [env] + blocks:
            e.reset(write_obs=False)
        out = torch.empty(n, dtype=torch.int32, device=env.device)
        for t in range(steps):
            want = r["action"][t]
            for fill, e_ in ((7, ev), (8, ev), (7, ev16)):
                out.fill_(fill)
                assert np.array_equal(env.uf_select_wide(e_, out=out).cpu().numpy(), want), (t, fill)
            for blk, b in zip(blocks, bases):
                assert np.array_equal(blk.uf_select_wide(ev16).cpu().numpy(), want[b:b + 16]), (t, b)
                blk.step(_dev(torch, blk, want[b:b + 16]), auto_reset=True, write_obs=False)
            env.step(out, auto_reset=True, write_obs=False)
        ev16.decode_into(syn, n, 4, 4, frame1)
        assert torch.equal(frame0, frame1) and int((frame0 != 0).sum()) > n
    finally:
        ev.close()
        ev16.close()
        for e in [env] + blocks:
            e.close()


def _agent(dq, env, policy, warmup, limit):
    model = dq.build_convolutional_nn(C_LAYERS, FF_LAYERS, env.obs_shape, env.num_actions)
    agent = dq.DQNAgent(model=model, nb_actions=env.num_actions, memory=dq.SequentialMemory(limit=limit, window_length=1), nb_steps_warmup=warmup,
                        target_model_update=512, policy=policy, test_policy=dq.GreedyQPolicy(masked_greedy=True), gamma=0.99,
                        enable_dueling_network=True, batch_size=32, seed=(1, 2))
    agent.compile(dq.Adam(lr=1e-4))
    return agent


def test_fit_with_the_wide_guide_records_the_teachers_episode(dq, torch_mod):
    """d = 9 X, volume_depth 5, 32 lattices, eps 1, share 1, warm-up beyond the run, 20 vector steps: the ring's actions, rewards and done flags are those of a
    twin environment (same seed and ids) driven by uf_select_wide + step(auto_reset=True)."""
    torch = torch_mod
    cfg = dict(d=9, error_model="X", use_Y=False, volume_depth=5, p_phys=0.006, p_meas=0.006)
    n, steps = 32, 20
    env = dq.VectorEnv(n_envs=n, seed=SEED, **cfg)
    assert env.wide
    guide = dq.WideUnionFindAgent()
    agent = _agent(dq, env, dq.EpsGreedyQPolicy(eps=1.0, masked_greedy=True, guide=guide, guide_share=1.0), warmup=10 ** 9, limit=n * 40)
    agent.fit(env, nb_steps=n * steps, verbose=0, episode_averaging_length=50, success_threshold=None, stopping_patience=None, min_nb_steps=0,
              single_cycle=False)
    core = agent._core
    assert core.vector_steps == steps and core.updates == 0 and agent.step == n * steps
    assert agent.last_guided_steps == 640
    twin = dq.VectorEnv(n_envs=n, seed=SEED, **cfg)
    ev = _evaluator(dq, twin)
    try:
        twin.reset()
        flips = 0
        for t in range(steps):
            a = twin.uf_select_wide(ev)
            twin.step(a, auto_reset=True)
            assert torch.equal(core.ring.action[t], a), t
            assert torch.equal(core.ring.reward[t], twin.reward), t
            assert torch.equal(core.ring.terminal[t], twin.done), t
            flips += int((a != twin.identity_index).sum())
        assert flips > n                                                           # (the teacher acted)
    finally:
        ev.close()
        twin.close()


def test_union_find_outlives_the_identity_at_distance_nine(dq, torch_mod):
    """An ordering, not a tolerance: d = 9 DP, volume_depth 5, p = 0.012, 64 lattices, 64 episodes each way on the same seed and ids.  (On the oracle
    environment the first episodes of 48 lattices lasted 306 measurements under the rule against 26 under the identity, the longest about 1500 agent
    steps: the cap is far beyond that.)"""
    cfg = dict(d=9, error_model="DP", use_Y=False, volume_depth=5, p_phys=0.012, p_meas=0.012)
    env = dq.VectorEnv(n_envs=64, seed=SEED, **cfg)
    try:
        uf = dq.WideUnionFindAgent()
        h_uf = uf.test(env, nb_episodes=64, verbose=0, nb_max_episode_steps=200000)
        ident = dq.WideUnionFindAgent(policy="identity")
        h_id = ident.test(env, nb_episodes=64, verbose=0, nb_max_episode_steps=200000)
        life_uf, life_id = (np.asarray(h.history["episode_lifetime"], dtype=np.float64) for h in (h_uf, h_id))
        assert len(life_uf) == 64 and len(life_id) == 64 and uf.last_inexact_steps == 0 and uf.last_vector_steps > ident.last_vector_steps
        print(f"mean lifetime: union-find {life_uf.mean():.1f}, identity {life_id.mean():.1f}")
        assert life_uf.mean() > life_id.mean()
    finally:
        env.close()
