"""Exploration guided by the matching decoder on the device (VectorEnv.guided_select, csrc/env_guide.hip; DQNAgent.fit with
EpsGreedyQPolicy(guide=...)).  The kernel's actions and flags must be the rule decoder.guided_actions states -- select_actions'
bits without a teacher's share, match_select's with nothing else -- on every lattice of 40 consecutive agent steps of every record layout; the
selection is a function of the lattices' state and global ids alone; fit() with a guide records the teacher's episode in the replay ring."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = (1234, 5678)
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


def _env(dq, cfg, p, n=N, base=0):
    return dq.VectorEnv(n_envs=n, p_phys=p, p_meas=p, seed=SEED, env_id_base=base, referee="lut", **cfg)


class _Run:
    """One environment of a configuration with its evaluator, random Q rows per step and the three selections side by side."""

    def __init__(self, dq, torch, name, n=N, base=0):
        cfg, p = CONFIGS[name]
        self.torch, self.env = torch, _env(dq, cfg, p, n=n, base=base)
        self.ev = dq.decoder.Evaluator(cfg["d"], cfg["error_model"], cfg["use_Y"], cfg["volume_depth"], chunk=n, device=self.env.device)
        self.gen = torch.Generator(device="cpu").manual_seed(len(name) * 1000 + cfg["d"])
        dev = self.env.device
        self.guided, self.inexact, self.t_inexact = (torch.zeros(n, dtype=torch.uint8, device=dev) for _ in range(3))
        self.env.reset()

    def q(self):
        """This step's random Q rows, float32 [n, num_actions] on the device."""
        return self.torch.randn((self.env.n_envs, self.env.num_actions), generator=self.gen, dtype=self.torch.float32).to(self.env.device)

    def legal_matrix(self):
        """The exported legal sets as a boolean matrix [n, num_actions]."""
        words = self.env.legal.cpu().numpy().view(np.uint64)
        a = np.arange(self.env.num_actions)
        return ((words[:, a >> 6] >> (a & 63).astype(np.uint64)) & np.uint64(1)).astype(bool)

    def guided_select(self, t, q, eps, share, masked):
        self.guided.fill_(7)
        self.inexact.fill_(7)
        a = self.env.guided_select(self.ev, t, q=q, eps=eps, guide_share=share, masked_greedy=masked, out_guided=self.guided, out_inexact=self.inexact)
        return a.cpu().numpy(), self.guided.cpu().numpy(), self.inexact.cpu().numpy()

    def teacher(self):
        a = self.env.match_select(self.ev, out_inexact=self.t_inexact)
        return a.cpu().numpy(), self.t_inexact.cpu().numpy()

    def close(self):
        self.ev.close()
        self.env.close()


@pytest.mark.parametrize("masked", [False, True], ids=["unmasked", "masked"])
@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_no_share_is_select_actions(dq, torch_mod, name, masked):
    r = _Run(dq, torch_mod, name)
    explored = greedy = 0
    try:
        for t in range(STEPS):
            q = r.q()
            want = r.env.select_actions(t, q=q, eps=0.3, masked_greedy=masked).cpu().numpy()
            got, guided, inexact = r.guided_select(t, q, 0.3, 0.0, masked)
            assert np.array_equal(got, want), (name, t, np.flatnonzero(got != want)[:8])
            assert not guided.any() and not inexact.any()
            legal = r.legal_matrix()
            top = np.where(legal, q.cpu().numpy(), -np.inf).argmax(axis=1) if masked else q.argmax(dim=1).cpu().numpy()
            greedy += int((got == top).sum())
            explored += int((got != top).sum())                                 # (only an exploring lattice leaves the row's first maximum)
            r.env.step(r.torch.from_numpy(got).to(r.env.device), auto_reset=True)
    finally:
        r.close()
    assert explored > 0 and greedy > 0


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_full_share_is_match_select(dq, torch_mod, name):
    r = _Run(dq, torch_mod, name)
    flips = 0
    try:
        for t in range(STEPS):
            want, want_flag = r.teacher()
            q = r.q()
            for q_arg, eps in ((q, 1.0), (None, 0.0), (None, 1.0)):              # q = None: every lattice explores, whatever eps
                got, guided, inexact = r.guided_select(t, q_arg, eps, 1.0, True)
                assert np.array_equal(got, want), (name, t, eps)
                assert np.array_equal(inexact, want_flag) and (guided == 1).all()
            flips += int((want != r.env.identity_index).sum())
            r.env.step(r.torch.from_numpy(want).to(r.env.device), auto_reset=True)
    finally:
        r.close()
    assert flips > N                                                            # (the teacher had something to say)


@pytest.mark.parametrize("masked", [False, True], ids=["unmasked", "masked"])
@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_mixed_policy_is_the_numpy_rule(dq, torch_mod, name, masked):
    """eps = 0.5, guide_share = 0.5: actions and flags equal decoder.guided_actions fed with match_select's output, the exported legal sets and the same
    Q; every one of the three branches is taken (counted from the flags and the rule's own draw, per configuration)."""
    r = _Run(dq, torch_mod, name)
    D = dq.decoder
    counts = dict(guided=0, uniform=0, greedy=0, guided_not_legal=0, guided_on_done=0)
    try:
        for t in range(STEPS):
            q = r.q()
            teacher, t_flag = r.teacher()
            legal = r.env.legal.cpu().numpy()
            done = r.env.done.cpu().numpy().astype(bool)
            want, want_guided = D.guided_actions(q.cpu().numpy(), legal, teacher, 0.5, 0.5, masked, SEED, 0, t)
            got, guided, inexact = r.guided_select(t, q, 0.5, 0.5, masked)
            assert np.array_equal(got, want), (name, t, np.flatnonzero(got != want)[:8])
            assert np.array_equal(guided, want_guided)
            assert np.array_equal(inexact, np.where(want_guided == 1, t_flag, 0))
            # the branches: with guide_share = 1 the rule's flags are its explore draws
            explore = D.guided_actions(q.cpu().numpy(), legal, teacher, 0.5, 1.0, masked, SEED, 0, t)[1].astype(bool)
            g = want_guided.astype(bool)
            assert not (g & ~explore).any()
            counts["guided"] += int(g.sum())
            counts["uniform"] += int((explore & ~g).sum())
            counts["greedy"] += int((~explore).sum())
            counts["guided_not_legal"] += int((g & ~r.legal_matrix()[np.arange(N), got]).sum())
            counts["guided_on_done"] += int((g & done).sum())
            r.env.step(r.torch.from_numpy(got).to(r.env.device), auto_reset=True)
    finally:
        r.close()
    print(name, "masked" if masked else "unmasked", counts)
    assert counts["guided"] > 0 and counts["uniform"] > 0 and counts["greedy"] > 0, counts


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_q_none_explores_everywhere(dq, torch_mod, name):
    r = _Run(dq, torch_mod, name)
    try:
        for t in range(STEPS):
            q = r.q()
            a1, g1, i1 = r.guided_select(t, q, 1.0, 0.5, False)
            a0, g0, i0 = r.guided_select(t, None, 0.0, 0.5, False)
            assert np.array_equal(a0, a1) and np.array_equal(g0, g1) and np.array_equal(i0, i1), (name, t)
            assert 0 < g0.sum() < N
            r.env.step(r.torch.from_numpy(a0).to(r.env.device), auto_reset=True)
    finally:
        r.close()


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_selection_depends_on_state_and_global_ids_only(dq, torch_mod, name):
    """A 64-lattice call equals two 32-lattice calls at env_id_base 0 and 32; a repeated call gives the same bytes and leaves export_state() unchanged."""
    torch = torch_mod
    whole = _Run(dq, torch, name, n=64)
    parts = [_Run(dq, torch, name, n=32, base=b) for b in (0, 32)]
    try:
        for t in range(STEPS):
            q = whole.q()
            before = whole.env.export_state().clone()
            a, g, i = whole.guided_select(t, q, 0.5, 0.5, True)
            a2, g2, i2 = whole.guided_select(t, q, 0.5, 0.5, True)
            assert np.array_equal(a, a2) and np.array_equal(g, g2) and np.array_equal(i, i2)
            assert torch.equal(before, whole.env.export_state())
            got = [p.guided_select(t, q[b:b + 32].contiguous(), 0.5, 0.5, True) for p, b in zip(parts, (0, 32))]
            for k, want in enumerate((a, g, i)):
                assert np.array_equal(np.concatenate([got[0][k], got[1][k]]), want), (name, t, k)
            whole.env.step(torch.from_numpy(a).to(whole.env.device), auto_reset=True)
            for p, b in zip(parts, (0, 32)):
                p.env.step(torch.from_numpy(a[b:b + 32].copy()).to(p.env.device), auto_reset=True)
    finally:
        for r in [whole] + parts:
            r.close()


def _agent(dq, env, policy, warmup, limit=64 * 80):
    model = dq.build_convolutional_nn(C_LAYERS, FF_LAYERS, env.obs_shape, env.num_actions)
    agent = dq.DQNAgent(model=model, nb_actions=env.num_actions, memory=dq.SequentialMemory(limit=limit, window_length=1), nb_steps_warmup=warmup,
                        target_model_update=512, policy=policy, test_policy=dq.GreedyQPolicy(masked_greedy=True), gamma=0.99,
                        enable_dueling_network=True, batch_size=32, seed=(1, 2))
    agent.compile(dq.Adam(lr=1e-4))
    return agent


def test_fit_with_a_guide_records_the_teachers_episode(dq, torch_mod):
    """d = 5 X, 64 lattices, eps fixed at 1, share 1, warm-up longer than the run, 30 vector steps: the ring's actions, rewards and done flags are those of a
    twin environment (same seed and ids) driven by match_select + step(auto_reset=True)."""
    torch = torch_mod
    n, steps = 64, 30
    env = dq.VectorEnv(n_envs=n, seed=SEED, **D5X)
    agent = _agent(dq, env, dq.EpsGreedyQPolicy(eps=1.0, masked_greedy=True, guide=dq.decoder.MatchingAgent(), guide_share=1.0), warmup=10 ** 9)
    agent.fit(env, nb_steps=n * steps, verbose=0, episode_averaging_length=50, success_threshold=None, stopping_patience=None, min_nb_steps=0,
              single_cycle=False)
    core = agent._core
    assert core.vector_steps == steps and core.updates == 0 and agent.step == n * steps
    assert agent.last_guided_steps == steps * n
    twin = dq.VectorEnv(n_envs=n, seed=SEED, **D5X)
    ev = dq.decoder.Evaluator(5, "X", False, 5, chunk=n, device=twin.device)
    try:
        twin.reset()
        flips = dones = 0
        for t in range(steps):
            a = twin.match_select(ev)
            twin.step(a, auto_reset=True)
            assert torch.equal(core.ring.action[t], a), t
            assert torch.equal(core.ring.reward[t], twin.reward), t
            assert torch.equal(core.ring.terminal[t], twin.done), t
            flips += int((a != twin.identity_index).sum())
            dones += int(twin.done.sum())
        assert flips > n and dones > 0                                          # (the teacher acted; the comparison crosses an auto-reset)
    finally:
        ev.close()
    # test() ignores the guide: a greedy evaluation, nothing counted, the training ring untouched
    ring_actions = core.ring.action.clone()
    th = agent.test(env, nb_episodes=8, visualize=False, verbose=0)
    assert len(th.history["episode_lifetime"]) == 8 and torch.equal(core.ring.action, ring_actions)


def test_guided_training_runs_to_the_end(dq, torch_mod):
    """The same lattice, eps annealed 1 -> 0.1, share 0.5, 2 000 steps with updates: finite loss and parameters, some but not all steps guided."""
    torch = torch_mod
    n, nb = 64, 2000
    env = dq.VectorEnv(n_envs=n, seed=SEED, **D5X)
    inner = dq.EpsGreedyQPolicy(masked_greedy=True, guide=dq.decoder.MatchingAgent(), guide_share=0.5)
    policy = dq.LinearAnnealedPolicy(inner, attr="eps", value_max=1.0, value_min=0.1, value_test=0.0, nb_steps=nb)
    agent = _agent(dq, env, policy, warmup=256)
    hist = agent.fit(env, nb_steps=nb, verbose=0, episode_averaging_length=50, success_threshold=None, stopping_patience=None, min_nb_steps=0,
                     single_cycle=False, sync_interval=4)
    core = agent._core
    assert agent.step >= nb and core.updates > 0
    loss, mean_q = core.read_metrics()
    assert np.isfinite(loss) and np.isfinite(mean_q) and torch.isfinite(core.params).all()
    losses = [x for x in hist.history.get("loss", []) if x == x]
    assert losses and np.isfinite(losses).all()
    assert 0 < agent.last_guided_steps < agent.step
    assert 0 <= agent.last_inexact_steps <= agent.last_guided_steps
    # a second fit() without a guide takes the riding path again and counts nothing
    agent.policy = dq.EpsGreedyQPolicy(eps=0.1, masked_greedy=True)
    agent.policy._set_agent(agent)
    agent.fit(env, nb_steps=4 * n, verbose=0, episode_averaging_length=50, success_threshold=None, stopping_patience=None, min_nb_steps=0,
              single_cycle=False)
    assert agent.last_guided_steps == 0 and agent.last_inexact_steps == 0
