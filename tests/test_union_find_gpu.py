"""The union-find decoder on the device (decoder.matching_decode / score_matching / MatchingAgent / VectorEnv.match_select / guided_select with
method="union_find"; csrc/uf_dev.h, uf_st.hip and the union-find forms of env_match.hip / env_guide.hip) against
tests/union_find_ref.py, bit for bit: the algorithm is fully specified (synchronous growth, lowest-edge-id parents), so frames, weights, defect
counts and growth rounds are compared as they are."""
import numpy as np
import pytest

import decode_eval_ref as V
import match_st_ref as M
import shipped
import union_find_ref as U
from oracle import lattice, referee

pytestmark = pytest.mark.gpu

SEED = (1234, 5678)
UF = "union_find"
CONFIGS = {                                                                   # test_match_policy_gpu.py's shapes: the smallest that reach every record layout
    "a_d3_x_2": (dict(d=3, error_model="X", use_Y=False, volume_depth=2), 0.02),
    "b_d5_dp_5_y": (dict(d=5, error_model="DP", use_Y=True, volume_depth=5), 0.011),
    "b_d5_dp_5": (dict(d=5, error_model="DP", use_Y=False, volume_depth=5), 0.011),
    "c_d5_dp_9": (dict(d=5, error_model="DP", use_Y=False, volume_depth=9), 0.011),      # the 32-word record
    "d_d7_x_7": (dict(d=7, error_model="X", use_Y=False, volume_depth=7), 0.011),
}
N, STEPS = 256, 40
C_LAYERS, FF_LAYERS = [[64, 3, 2], [32, 2, 1], [32, 2, 1]], [[512, 0.2]]
D5X = dict(d=5, error_model="X", use_Y=False, volume_depth=5, p_phys=0.007, p_meas=0.007)


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return torch


def _env1(dq, d, model, depth, p=0.01, ref=None):
    return dq.VectorEnv(n_envs=1, p_phys=p, p_meas=p, seed=SEED, referee=ref, d=d, error_model=model, use_Y=False, volume_depth=depth)


def _env(dq, cfg, p, n=N, base=0):
    return dq.VectorEnv(n_envs=n, p_phys=p, p_meas=p, seed=SEED, env_id_base=base, referee="lut", **cfg)


def _volume_from_defects(d, depth, rows0=None, rows1=None):
    """One volume uint8 [depth, d+1, d+1] whose components have the given defect rows int [depth, n] (S_t = XOR of D_0 .. D_t)."""
    vol = np.zeros((depth, d + 1, d + 1), dtype=np.uint8)
    for comp, rows in ((0, rows0), (1, rows1)):
        if rows is None:
            continue
        s = np.bitwise_xor.accumulate(np.asarray(rows, dtype=np.int64), axis=0)
        for j, (a, b) in enumerate(M.Component(d, comp).cells):
            vol[:, a, b] = s[:, j]
    return vol


def _assert_is_reference(d, depth, vol, res, tag):
    frame, weight, ndef, rounds = U.decode(d, vol, depth)
    for key, want in (("frame", frame), ("weight", weight), ("n_defects", ndef), ("rounds", rounds)):
        got = getattr(res, key)
        assert got.dtype == want.dtype and got.shape == want.shape, (tag, key, got.dtype, got.shape)
        bad = np.flatnonzero((got != want).reshape(len(vol), -1).any(axis=1))
        assert bad.size == 0, (tag, key, bad[:8], got[bad[:2]], want[bad[:2]])
    assert res.inexact.dtype == np.uint8 and res.inexact.shape == (len(vol),) and not res.inexact.any(), tag
    return frame, weight, ndef, rounds


# ---- 1. exhaustive -------------------------------------------------------------------------------------------------------------------------
def test_every_volume_of_d3_depth2_is_the_reference(dq, torch_mod):
    d, depth = 3, 2
    m = lattice.Masks(d)
    n = 1 << (depth * m.n_stab)
    idx = np.arange(n, dtype=np.int64)
    vol = np.zeros((n, depth, d + 1, d + 1), dtype=np.uint8)
    for t in range(depth):
        for s, (a, b) in enumerate(m.order):
            vol[:, t, a, b] = (idx >> (t * m.n_stab + s)) & 1
    res = dq.decoder.matching_decode(vol, _env1(dq, d, "DP", depth), chunk=20000, to_host=True, method=UF)
    frame, weight, _, rounds = _assert_is_reference(d, depth, vol, res, "d3")
    assert len(np.unique(frame.reshape(n, -1), axis=0)) > 50 and rounds.max() >= 2 and weight.max() >= 4      # (not vacuous)


# ---- 2. samples ------------------------------------------------------------------------------------------------------------------------------
SAMPLES = {"d5_5_p011": (5, 5, 512, 0.011), "d7_7_p007": (7, 7, 256, 0.007), "d7_16_p02": (7, 16, 64, 0.02), "d5_5_p06": (5, 5, 256, 0.06)}


@pytest.mark.parametrize("name", sorted(SAMPLES))
def test_sampled_volumes_are_the_reference(dq, torch_mod, name):
    d, depth, n, p = SAMPLES[name]
    env = _env1(dq, d, "DP", depth, p)
    vol, _, _ = dq.decoder.sample_volumes(env, n, seed=SEED, to_host=True)
    res = dq.decoder.matching_decode(vol, env, to_host=True, method=UF)
    _, weight, ndef, rounds = _assert_is_reference(d, depth, vol, res, name)
    print(name, dict(max_defects=int(ndef.max()), max_weight=int(weight.max()), max_rounds=int(rounds.max()), nonzero=int((ndef.sum(axis=1) > 0).sum())))
    assert (ndef.sum(axis=1) > 0).sum() > n // 4
    if name == "d5_5_p06":                                                    # the density at which matching takes its 14 / 32 fallback
        assert ndef.max() > 14 and dq.decoder.matching_decode(vol, env, to_host=True).inexact.sum() > 0


# ---- 3. hand cases ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,depth", [(5, 5), (7, 7), (7, 16)])
def test_hand_cases(dq, torch_mod, d, depth):
    cases = [c for c in U.hand_cases() if c[1] == d and c[3] == depth]
    vol = np.stack([_volume_from_defects(d, depth, rows if comp == 0 else None, rows if comp == 1 else None) for _, _, comp, _, rows, _ in cases])
    res = dq.decoder.matching_decode(vol, _env1(dq, d, "DP", depth), to_host=True, method=UF)
    _assert_is_reference(d, depth, vol, res, f"hand d{d} depth {depth}")
    q = np.arange(d * d)
    for i, (name, _, comp, _, rows, want) in enumerate(cases):
        plane = M.Component(d, comp).plane(res.frame[i:i + 1])[0]
        got = dict(M=int((plane << q).sum()), W=int(res.weight[i, comp]), rounds=int(res.rounds[i, comp]))
        for key, v in want.items():
            assert got[key] == v, (name, key, got, want)
        assert res.n_defects[i, comp] == rows.sum() and res.weight[i, 1 - comp] == 0 and res.rounds[i, 1 - comp] == 0, name
    assert any(name.endswith("central") and want["rounds"] == 6 for name, _, _, _, _, want in cases) == (d == 7)


# ---- 4. / 5. invariance; the two decoders share a handle ------------------------------------------------------------------------------------------
def test_results_depend_on_the_volume_alone_and_matching_is_untouched(dq, torch_mod):
    D = dq.decoder
    d, depth, n = 5, 5, 300
    env = _env1(dq, d, "DP", depth, 0.03)
    vol, _, _ = D.sample_volumes(env, n, seed=SEED, env_id_base=77, to_host=True)
    keys = ("frame", "weight", "n_defects", "inexact", "rounds")
    same = lambda a, b, ks=keys: all(np.array_equal(getattr(a, k), getattr(b, k)) for k in ks)
    ev = D.Evaluator(d, "DP", False, depth, chunk=n, device=env.device)
    try:
        before = D.matching_decode(vol, env, to_host=True, evaluator=ev)                # matching first: its tables and the union-find ones coexist
        assert before.rounds is None
        base = D.matching_decode(vol, env, to_host=True, evaluator=ev, method=UF)
        after = D.matching_decode(vol, env, to_host=True, evaluator=ev)
        assert same(before, after, keys[:4]) and same(before, D.matching_decode(vol, env, to_host=True), keys[:4])
        assert same(base, D.matching_decode(vol, env, to_host=True, evaluator=ev, method=UF))          # a repeated call
    finally:
        ev.close()
    for chunk in (1, 7, n):
        assert same(base, D.matching_decode(vol, env, chunk=chunk, to_host=True, method=UF)), chunk
    perm = np.random.default_rng(3).permutation(n)
    shuffled = D.matching_decode(vol[perm], env, chunk=64, to_host=True, method=UF)
    assert all(np.array_equal(getattr(shuffled, k), getattr(base, k)[perm]) for k in keys)
    assert (base.weight >= before.weight)[before.inexact == 0].all()                   # where matching is exact it is the minimum


# ---- 6. the policy ------------------------------------------------------------------------------------------------------------------------------
def _state(dq, env):
    """(volumes uint8 [N, depth, d+1, d+1], completed sets, done flags) of the lattices as they stand."""
    st = env.export_state().cpu().numpy().view(np.uint64)
    d, depth = env.d, env.volume_depth
    vol = np.zeros((len(st), depth, d + 1, d + 1), dtype=np.uint8)
    for s, (a, b) in enumerate(lattice.Masks(d).order):
        vol[:, :, a, b] = ((st[:, 11:11 + depth] >> np.uint64(s)) & np.uint64(1)).astype(np.uint8)
    completed = [dq.decoder.completed_from_words(w0, w1) for w0, w1 in st[:, 6:8]]
    return vol, completed, ((st[:, 10] >> np.uint64(32)) & np.uint64(1)).astype(bool)


_teacher_runs = {}


def _teacher_run(dq, torch, name):
    """40 agent steps of match_select(method="union_find") + step(auto_reset) on the configuration, checked against the rule on every live lattice;
    cached: the per-step actions the guided tests compare with."""
    if name in _teacher_runs:
        return _teacher_runs[name]
    cfg, p = CONFIGS[name]
    D = dq.decoder
    d, model, use_Y, depth = cfg["d"], cfg["error_model"], cfg["use_Y"], cfg["volume_depth"]
    env = _env(dq, cfg, p)
    ev = D.Evaluator(d, model, use_Y, depth, chunk=N, device=env.device)
    identity = env.identity_index
    flag = torch.full((N,), 7, dtype=torch.uint8, device=env.device)
    env.reset()
    actions = []
    dead = second = flips = 0
    try:
        for t in range(STEPS):
            before = env.export_state().clone()
            vol, completed, done = _state(dq, env)
            res = D.matching_decode(vol, env, to_host=True, evaluator=ev, method=UF)
            act = env.match_select(ev, out_inexact=flag, method=UF)
            assert torch.equal(before, env.export_state()), (name, t)
            got = act.cpu().numpy()
            assert not flag.cpu().numpy().any()
            for i in range(N):
                if done[i]:
                    assert got[i] == identity, (name, t, i)
                    dead += 1
                    continue
                wanted, a = D.frame_to_actions(res.frame[i], completed[i], d, model, use_Y)
                assert got[i] == a, (name, t, i, wanted, sorted(completed[i]), int(got[i]))
                flips += a != identity
                second += a != identity and len(completed[i]) > 0
            actions.append(got.copy())
            env.step(act, auto_reset=True)
    finally:
        ev.close()
        env.close()
    live = STEPS * N - dead
    print(name, dict(live=live, dead=dead, flips=int(flips), second_flips=int(second)))
    assert live > 30 * N and flips > N and second > 0
    _teacher_runs[name] = actions
    return actions


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_policy_action_is_the_rule_on_every_live_lattice(dq, torch_mod, name):
    _teacher_run(dq, torch_mod, name)


# ---- 7. guided selection ------------------------------------------------------------------------------------------------------------------------
class _Run:
    def __init__(self, dq, torch, name, n=N, base=0):
        cfg, p = CONFIGS[name]
        self.torch, self.env = torch, _env(dq, cfg, p, n=n, base=base)
        self.ev = dq.decoder.Evaluator(cfg["d"], cfg["error_model"], cfg["use_Y"], cfg["volume_depth"], chunk=n, device=self.env.device)
        self.gen = torch.Generator(device="cpu").manual_seed(len(name) * 1000 + cfg["d"])
        self.guided, self.inexact = (torch.zeros(n, dtype=torch.uint8, device=self.env.device) for _ in range(2))
        self.env.reset()

    def q(self):
        return self.torch.randn((self.env.n_envs, self.env.num_actions), generator=self.gen, dtype=self.torch.float32).to(self.env.device)

    def guided_select(self, t, q, eps, share, masked):
        self.guided.fill_(7)
        self.inexact.fill_(7)
        a = self.env.guided_select(self.ev, t, q=q, eps=eps, guide_share=share, masked_greedy=masked, out_guided=self.guided, out_inexact=self.inexact,
                                   method=UF)
        assert not self.inexact.cpu().numpy().any()                               # zero-filled: the union-find teacher has no fallback
        return a.cpu().numpy(), self.guided.cpu().numpy()

    def step(self, a):
        self.env.step(self.torch.from_numpy(np.ascontiguousarray(a)).to(self.env.device), auto_reset=True)

    def close(self):
        self.ev.close()
        self.env.close()


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_guided_selection_with_the_union_find_teacher(dq, torch_mod, name):
    """Along the teacher's own 40 steps (the run of test 6, so its actions are the checked ones): share 0 is select_actions, eps 1 / share 1 and q = None
    are the teacher, eps 0.5 / share 0.5 is decoder.guided_actions fed with the teacher's actions, all three branches occurring."""
    teacher = _teacher_run(dq, torch_mod, name)
    r = _Run(dq, torch_mod, name)
    D = dq.decoder
    counts = dict(guided=0, uniform=0, greedy=0)
    try:
        for t in range(STEPS):
            q = r.q()
            want = r.env.select_actions(t, q=q, eps=0.3, masked_greedy=True).cpu().numpy()
            got, guided = r.guided_select(t, q, 0.3, 0.0, True)
            assert np.array_equal(got, want) and not guided.any(), (name, t)
            for q_arg, eps in ((q, 1.0), (None, 0.0)):
                got, guided = r.guided_select(t, q_arg, eps, 1.0, True)
                assert np.array_equal(got, teacher[t]) and (guided == 1).all(), (name, t, eps)
            legal = r.env.legal.cpu().numpy()
            want, want_guided = D.guided_actions(q.cpu().numpy(), legal, teacher[t], 0.5, 0.5, False, SEED, 0, t)
            got, guided = r.guided_select(t, q, 0.5, 0.5, False)
            assert np.array_equal(got, want) and np.array_equal(guided, want_guided), (name, t, np.flatnonzero(got != want)[:8])
            explore = D.guided_actions(q.cpu().numpy(), legal, teacher[t], 0.5, 1.0, False, SEED, 0, t)[1].astype(bool)
            g = want_guided.astype(bool)
            counts["guided"] += int(g.sum())
            counts["uniform"] += int((explore & ~g).sum())
            counts["greedy"] += int((~explore).sum())
            r.step(teacher[t])
    finally:
        r.close()
    assert min(counts.values()) > 0, counts


def test_guided_selection_depends_on_state_and_global_ids_only(dq, torch_mod):
    name = "b_d5_dp_5"
    whole = _Run(dq, torch_mod, name, n=64)
    parts = [_Run(dq, torch_mod, name, n=32, base=b) for b in (0, 32)]
    try:
        for t in range(STEPS):
            q = whole.q()
            a, g = whole.guided_select(t, q, 0.5, 0.5, True)
            got = [p.guided_select(t, q[b:b + 32].contiguous(), 0.5, 0.5, True) for p, b in zip(parts, (0, 32))]
            for k, want in enumerate((a, g)):
                assert np.array_equal(np.concatenate([got[0][k], got[1][k]]), want), (t, k)
            whole.step(a)
            for p, b in zip(parts, (0, 32)):
                p.step(a[b:b + 32])
    finally:
        for r in [whole] + parts:
            r.close()


# ---- 8. fit() with the union-find teacher -----------------------------------------------------------------------------------------------------------
def test_fit_with_the_union_find_guide_records_the_teachers_episode(dq, torch_mod):
    torch = torch_mod
    n, steps = 64, 30
    env = dq.VectorEnv(n_envs=n, seed=SEED, **D5X)
    model = dq.build_convolutional_nn(C_LAYERS, FF_LAYERS, env.obs_shape, env.num_actions)
    policy = dq.EpsGreedyQPolicy(eps=1.0, masked_greedy=True, guide=dq.decoder.MatchingAgent(method=UF), guide_share=1.0)
    agent = dq.DQNAgent(model=model, nb_actions=env.num_actions, memory=dq.SequentialMemory(limit=64 * 80, window_length=1), nb_steps_warmup=10 ** 9,
                        target_model_update=512, policy=policy, test_policy=dq.GreedyQPolicy(masked_greedy=True), gamma=0.99,
                        enable_dueling_network=True, batch_size=32, seed=(1, 2))
    agent.compile(dq.Adam(lr=1e-4))
    agent.fit(env, nb_steps=n * steps, verbose=0, episode_averaging_length=50, success_threshold=None, stopping_patience=None, min_nb_steps=0,
              single_cycle=False)
    core = agent._core
    assert core.vector_steps == steps and core.updates == 0 and agent.step == n * steps
    assert agent.last_guided_steps == steps * n and agent.last_inexact_steps == 0
    twin = dq.VectorEnv(n_envs=n, seed=SEED, **D5X)
    ev = dq.decoder.Evaluator(5, "X", False, 5, chunk=n, device=twin.device)
    try:
        twin.reset()
        flips = dones = differs = 0
        for t in range(steps):
            a = twin.match_select(ev, method=UF)
            differs += int((a != twin.match_select(ev)).sum())
            twin.step(a, auto_reset=True)
            assert torch.equal(core.ring.action[t], a), t
            assert torch.equal(core.ring.reward[t], twin.reward), t
            assert torch.equal(core.ring.terminal[t], twin.done), t
            flips += int((a != twin.identity_index).sum())
            dones += int(twin.done.sum())
        print("flips", flips, "dones", dones, "lattice-steps on which matching would act otherwise", differs)
        assert flips > n and dones > 0
    finally:
        ev.close()


# ---- 9. ordering: a condition, not a tolerance -------------------------------------------------------------------------------------------------------
def test_union_find_outlives_the_identity_policy(dq, torch_mod):
    cfg, p, n = shipped.CONFIGS["d5_dp"], 0.007, 256
    D = dq.decoder
    mean = lambda h: float(np.mean(h.history["episode_lifetime"]))
    agent = D.MatchingAgent(method=UF)
    uf = mean(agent.test(_env(dq, cfg, p, n=n), nb_episodes=n, verbose=0))
    assert agent.last_inexact_steps == 0 and agent.last_vector_steps > 0
    ident = mean(D.MatchingAgent(policy="identity").test(_env(dq, cfg, p, n=n), nb_episodes=n, verbose=0))
    print(f"d5_dp p = {p}, {n} episodes: mean lifetime union-find {uf:.2f}, identity only {ident:.2f}")
    assert uf > ident, (uf, ident)


# ---- 10. scoring ----------------------------------------------------------------------------------------------------------------------------------
def test_score_union_find_counts_and_the_three_rows(dq, torch_mod):
    from oracle import c_oracle
    D = dq.decoder
    n, first, p = 65536, 1024, 0.007
    env = dq.VectorEnv(n_envs=1, p_phys=p, p_meas=p, seed=SEED, referee="lut", **shipped.CONFIGS["d5_dp"])
    timings = {}
    got = D.score_matching(env, n, no_decoder=True, method=UF, timings=timings)
    assert got.counters["volumes"] == n and got.inexact == 0 and "match" in timings
    head = D.score_matching(env, first, method=UF)
    vol, hid, triv = D.sample_volumes(env, first, to_host=True)
    frame = U.decode(5, vol, 5)[0]
    lx, lz = c_oracle.luts(5)
    verd = V.verdict(5, hid, frame, V.classify_with(referee.LutReferee(5, "DP", lx, lz)))
    want = D.counters_from_arrays(verd, triv, np.full(first, D.STATUS_IDENTITY), (frame.reshape(first, -1) != 0).sum(axis=1))
    assert [head.counters[k] for k in D.COUNTER_NAMES] == want
    print(f"union-find failure rate {got.failure_rate:.5f} {got.failure_interval}, no decoder {got.no_decoder.failure_rate:.5f} {got.no_decoder.failure_interval}")
    assert got.failure_interval[1] < got.no_decoder.failure_interval[0]
    weights, _ = shipped.shipped_weights("d5_dp", "0.007")
    model = dq.build_convolutional_nn(shipped.C_LAYERS, shipped.FF_LAYERS, env.observation_space.shape, env.num_actions)
    agent = dq.DQNAgent(model=model, nb_actions=env.num_actions, memory=dq.SequentialMemory(limit=1000, window_length=1), nb_steps_warmup=100,
                        target_model_update=100, policy=dq.GreedyQPolicy(masked_greedy=True), test_policy=dq.GreedyQPolicy(masked_greedy=True),
                        gamma=0.99, enable_dueling_network=True)
    agent.compile(dq.Adam(lr=1e-4))
    agent._bind(env)
    agent.model.set_weights(weights)
    try:
        rows = agent.decode_benchmark(env, 8192, chunk=8192, baseline=("matching", UF))
        assert isinstance(rows, tuple) and len(rows) == 3
        assert len({(r.counters["volumes"], r.counters["trivial"]) for r in rows}) == 1 and rows[0].counters["volumes"] == 8192
        pair = agent.decode_benchmark(env, 8192, chunk=8192, baseline=UF)
        assert len(pair) == 2 and pair[1].counters == rows[2].counters and pair[0].counters == rows[0].counters
        assert rows[2].counters == D.score_matching(env, 8192, method=UF).counters and rows[2].inexact == 0
        print("failure rates on 8192 volumes: agent %.4f, matching %.4f, union-find %.4f" % tuple(r.failure_rate for r in rows))
    finally:
        agent._decoder = None
