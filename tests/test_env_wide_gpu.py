"""The wide environment (csrc/env_big.hip: W-word bit-planes, the matching referee inside the step, policy_wide_kernel) against the wide C
oracle (oracle/env_oracle_wide.c, pinned by tests/test_oracle_wide_c.py) at full batch: every output of every step -- action, obs, reward,
done, lifetime, all legal words, was_reset, inexact -- and the whole exported state at the end, bit for bit.  Batches fill many workgroups
of BIG_EPB = 4 lattices (with ragged last ones), and each configuration asserts the events it exists to exercise (rewards, dones, auto-resets,
referee fallbacks), so that a retune cannot make it vacuous."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = (0x5EED, 0xD0DEC0DE)

CONFIGS = {
    "d9dp": dict(d=9, error_model="DP", use_Y=False, volume_depth=9, p_phys=0.008, p_meas=0.008),
    "d9x": dict(d=9, error_model="X", use_Y=False, volume_depth=9, p_phys=0.006, p_meas=0.006),
    "d9iidxz": dict(d=9, error_model="IIDXZ", use_Y=False, volume_depth=6, p_phys=0.006, p_meas=0.006),
    "d9deep": dict(d=9, error_model="DP", use_Y=False, volume_depth=16, p_phys=0.004, p_meas=0.004),
    # measurement-heavy: most volumes come from measurement flips on a clean lattice, where the identity earns reward = 1
    "d9meas": dict(d=9, error_model="X", use_Y=False, volume_depth=4, p_phys=0.0005, p_meas=0.01),
    "d11dp": dict(d=11, error_model="DP", use_Y=False, volume_depth=5, p_phys=0.006, p_meas=0.006),
    "d11dpy": dict(d=11, error_model="DP", use_Y=True, volume_depth=4, p_phys=0.006, p_meas=0.006),
    "d13x": dict(d=13, error_model="X", use_Y=False, volume_depth=5, p_phys=0.004, p_meas=0.004),
    "d13dp": dict(d=13, error_model="DP", use_Y=False, volume_depth=4, p_phys=0.004, p_meas=0.004),
    "d15dpy": dict(d=15, error_model="DP", use_Y=True, volume_depth=3, p_phys=0.003, p_meas=0.003),
    "d15x": dict(d=15, error_model="X", use_Y=False, volume_depth=3, p_phys=0.003, p_meas=0.003),
    "d15meas": dict(d=15, error_model="DP", use_Y=False, volume_depth=3, p_phys=0.0002, p_meas=0.006),
    # hot: clusters beyond MAX_DEFECTS and components beyond MAX_LIST defects in most steps (the referee's fallbacks, the scratch pool)
    "d15hot": dict(d=15, error_model="DP", use_Y=False, volume_depth=2, p_phys=0.06, p_meas=0.06),
    # the wide backend below d = 9 (the header promises dq_env_*'s bits there)
    "c3": dict(d=5, error_model="DP", use_Y=False, volume_depth=5, p_phys=0.011, p_meas=0.011),
    "c5": dict(d=7, error_model="DP", use_Y=False, volume_depth=7, p_phys=0.011, p_meas=0.011),
    "d3dp": dict(d=3, error_model="DP", use_Y=False, volume_depth=3, p_phys=0.01, p_meas=0.01),
}


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _policy_oracle(q, legal_words, eps, masked_greedy, t, base):
    """dqn_oracle.select_action per lattice on the oracle's legal sets (a Python-int mask of all LW words)."""
    from oracle import dqn_oracle, philox
    out = np.zeros(q.shape[0], dtype=np.int32)
    for i in range(q.shape[0]):
        mask = sum(int(w) << (64 * k) for k, w in enumerate(legal_words[i]))
        words = philox.site_words(SEED, (base + i) & 0xFFFFFFFF, t, 0, stream=philox.STREAM_POLICY)
        out[i] = dqn_oracle.select_action(q[i], mask, eps, masked_greedy, words)
    return out


def _run(dq, torch, name, n_envs, steps, base, mode="uniform"):
    """mode: "uniform" -- select_actions(t) (policy_wide_kernel, no Q) then step; "eps" / "greedy" -- the fused act_step with random Q at
    eps = 0.3 (unmasked greedy otherwise) / eps = 0 masked greedy.  Returns the event totals."""
    from oracle import c_oracle
    cfg = CONFIGS[name]
    env = dq.VectorEnv(n_envs=n_envs, seed=SEED, env_id_base=base, backend="wide", **cfg)
    ref = c_oracle.COracleWideEnv(n_envs=n_envs, seed=SEED, env_id_base=base, **cfg)
    assert env.wide and env.legal_words == ref.legal_words and env.state_words == ref.state_words
    lut = c_oracle.COracleEnv(n_envs=n_envs, seed=SEED, env_id_base=base, **cfg) if cfg["d"] <= 7 else None
    env.reset()
    ref.reset()
    assert np.array_equal(env.obs.cpu().numpy(), ref.obs) and np.array_equal(_u64(env.legal), ref.legal)
    if lut is not None:
        lut.reset()
    gen = torch.Generator(device="cuda").manual_seed(17)
    ev = dict(reward=0, done=0, reset=0, inexact=0)
    for t in range(steps):
        if mode == "uniform":
            a = env.select_actions(t)
            a_ref = ref.policy_uniform_legal(t)
            env.step(a, auto_reset=True)
        else:
            q = torch.randn((n_envs, env.num_actions), device="cuda", generator=gen)
            eps, masked = (0.3, False) if mode == "eps" else (0.0, True)
            a_ref = _policy_oracle(q.cpu().numpy(), ref.legal, eps, masked, t, base)
            a = env.act_step(t, q=q, eps=eps, masked_greedy=masked, auto_reset=True)
        assert np.array_equal(a.cpu().numpy(), a_ref), (name, "action", t)
        ref.step(a_ref, auto_reset=True)
        assert np.array_equal(env.reward.cpu().numpy(), ref.reward), (name, "reward", t)
        assert np.array_equal(env.done.cpu().numpy(), ref.done), (name, "done", t)
        assert np.array_equal(env.was_reset.cpu().numpy(), ref.was_reset), (name, "was_reset", t)
        assert np.array_equal(env.inexact.cpu().numpy(), ref.inexact), (name, "inexact", t)
        assert np.array_equal(env.lifetime.cpu().numpy().view(np.uint32), ref.lifetime), (name, "lifetime", t)
        assert np.array_equal(_u64(env.legal), ref.legal), (name, "legal", t)
        assert np.array_equal(env.obs.cpu().numpy(), ref.obs), (name, "obs", t)
        if lut is not None:
            lut.step(a_ref, auto_reset=True)
            assert np.array_equal(lut.reward, ref.reward) and np.array_equal(lut.done, ref.done) and np.array_equal(lut.obs, ref.obs)
            assert np.array_equal(lut.legal[:, :ref.legal_words], ref.legal) and not lut.legal[:, ref.legal_words:].any()
        ev["reward"] += int((ref.reward == 1.0).sum())
        ev["done"] += int(ref.done.sum())
        ev["reset"] += int(ref.was_reset.sum())
        ev["inexact"] += int(ref.inexact.sum())
    assert np.array_equal(_u64(env.export_state()), ref.export_state()), (name, "export_state")
    env.close()
    return ev


# (config, n_envs, steps, env_id_base, selection, minimum events {reward, done, reset, inexact})
CASES = [
    ("d9dp", 1027, 20, 4096 * 3, "uniform", dict(done=600, reset=500, inexact=15)),
    ("d9x", 1024, 20, 0, "uniform", dict(reward=8, done=700, reset=600, inexact=20)),
    ("d9iidxz", 1022, 20, 77, "uniform", dict(done=500, reset=400, inexact=10)),
    ("d9deep", 1024, 16, 2 ** 31 - 515, "uniform", dict(done=400, reset=350, inexact=1)),
    ("d9meas", 4097, 24, 5, "uniform", dict(reward=700, done=1500, reset=1400)),
    ("d9dp", 1024, 16, 9000, "eps", dict(done=400, reset=350, inexact=10)),
    ("d9x", 1023, 16, 9000, "greedy", dict(reward=4, done=500, reset=450, inexact=10)),
    ("d11dp", 1024, 16, 0, "uniform", dict(reward=1, done=120, reset=100, inexact=20)),
    ("d11dpy", 1021, 16, 2 ** 31 - 3, "uniform", dict(reward=4, done=150, reset=120, inexact=15)),
    ("d13x", 1024, 12, 0, "uniform", dict(reward=8, done=90, reset=70, inexact=70)),
    ("d13dp", 1026, 13, 31, "eps", dict(done=4, reset=2, inexact=30)),
    ("d15dpy", 1024, 16, 2 ** 31 - 600, "uniform", dict(reward=8, done=8, reset=5, inexact=20)),
    ("d15x", 1025, 16, 123, "greedy", dict(reward=25, done=40, reset=30, inexact=60)),
    ("d15meas", 2048, 20, 0, "uniform", dict(reward=60, done=4, reset=3)),
    ("d15hot", 258, 2, 0, "uniform", dict(done=70, reset=60, inexact=180)),      # (every fallback cluster walks 2^20 subsets on the device)
    ("c3", 4096, 30, 4096 * 3, "uniform", dict(reward=600, done=7000, reset=7000)),
    ("c5", 1024, 20, 0, "eps", dict(done=800, reset=800)),
    ("d3dp", 4096, 30, 1, "uniform", dict(reward=3000, done=12000, reset=12000)),
]


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return torch


@pytest.mark.parametrize("name,n_envs,steps,base,mode,minimum", CASES,
                         ids=[f"{c[0]}-{c[1]}-{c[4]}" for c in CASES])
def test_wide_environment_vs_wide_c_oracle(dq, torch_mod, name, n_envs, steps, base, mode, minimum):
    ev = _run(dq, torch_mod, name, n_envs, steps, base, mode)
    print(name, n_envs, steps, mode, ev)
    for k, v in minimum.items():
        assert ev[k] >= v, (name, k, ev)
