"""Scoring batched decoding on the device (DQNAgent.decode_benchmark, decoder.BatchDecoder.evaluate / sample_volumes / verdict,
csrc/decode_eval.hip) against the numpy restatement (tests/decode_eval_ref.py), the environment, and itself across
chunk sizes and call shapes.

Test 9 (the shipped d5_dp agent against no decoder at p = 0.007, 2^18 volumes): measured on the MI355X, masked greedy -- see DESIGN.md
section 12 for the figures with their Wilson intervals (agent 217 209 successes of 262 144, failure 0.1714 [0.1700, 0.1729]; no decoder 109 426, failure
0.5826 [0.5807, 0.5845]); the test asserts the ordering only."""
import importlib

import numpy as np
import pytest

import decode_eval_ref as V
import decode_ref as R
import shipped
from oracle import lattice, referee

pytestmark = pytest.mark.gpu

P = 0.007
SEED = (0xC0FFEE, 0x5EED)
DP5 = dict(d=5, error_model="DP", use_Y=False, volume_depth=5)


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _agent(dq, family="d5_dp", p=P, referee="lut", n_envs=1):
    weights, flat = shipped.shipped_weights(family, str(P))
    env = dq.VectorEnv(n_envs=n_envs, p_phys=p, p_meas=p, seed=SEED, referee=referee, **shipped.CONFIGS[family])
    model = dq.build_convolutional_nn(shipped.C_LAYERS, shipped.FF_LAYERS, env.observation_space.shape, env.num_actions)
    agent = dq.DQNAgent(model=model, nb_actions=env.num_actions, memory=dq.SequentialMemory(limit=1000, window_length=1), nb_steps_warmup=100,
                        target_model_update=100, policy=dq.GreedyQPolicy(masked_greedy=True), test_policy=dq.GreedyQPolicy(masked_greedy=True),
                        gamma=0.99, enable_dueling_network=True)
    agent.compile(dq.Adam(lr=1e-4))
    agent._bind(env)
    agent.model.set_weights(weights)
    return agent, env


@pytest.fixture(scope="module")
def dp_agent(dq, torch_mod):
    agent, env = _agent(dq)
    yield agent, env
    agent._decoder = None


# ---- 4. the sampler ---------------------------------------------------------------------------------------------------------------------
SAMPLE_CASES = [(3, "X", False, 3, 0.03), (3, "DP", True, 2, 0.03), (5, "DP", False, 5, 0.007), (5, "IIDXZ", False, 3, 0.006),
                (5, "X", False, 5, 0.007), (7, "DP", False, 3, 0.005), (7, "IIDXZ", False, 2, 0.004), (7, "X", False, 3, 0.005)]


@pytest.mark.parametrize("d,model,use_Y,depth,p", SAMPLE_CASES, ids=[f"d{c[0]}_{c[1]}{'Y' if c[2] else ''}" for c in SAMPLE_CASES])
def test_sampler_equals_the_restatement_and_the_environment(dq, torch_mod, d, model, use_Y, depth, p):
    D = dq.decoder
    base = (1 << 31) - 100                                       # lattice ids across 2^31
    cfg = dict(d=d, error_model=model, use_Y=use_Y, volume_depth=depth)
    for n in (1, 257, 4097):
        env = dq.VectorEnv(n_envs=n, p_phys=p, p_meas=1.5 * p, seed=SEED, env_id_base=base, referee=None, **cfg)
        want = V.sample_volumes(d, model, depth, n, p, 1.5 * p, SEED, base)
        got = D.sample_volumes(env, n, seed=SEED, env_id_base=base, chunk=1000, to_host=True)      # the environment's rates, chunked
        for g, w, name in zip(got, want, ("volumes", "hidden", "trivial")):
            assert g.dtype == np.uint8 and np.array_equal(g, w), (n, name)
        if n > 1:
            assert 0 < int(want[2].sum()) < n                    # all-zero volumes and others: neither branch is vacuous
        # per-volume rates: volume i draws what a scalar call at its rate draws for its lattice
        ph = np.where(np.arange(n) % 2 == 0, p, 3 * p)
        pm = np.where(np.arange(n) % 3 == 0, 0.0, 2 * p)
        want_each = V.sample_volumes(d, model, depth, n, ph, pm, SEED, base)
        got_each = D.sample_volumes(env, n, ph, pm, seed=SEED, env_id_base=base, to_host=True)
        for g, w, name in zip(got_each, want_each, ("volumes", "hidden", "trivial")):
            assert np.array_equal(g, w), (n, name, "per-volume rates")
        # the environment's own first volume, where it is not all zero (reset() redraws the others)
        env.reset()
        st = env.export_state().cpu().numpy().view(np.uint64)
        live = want[2] == 0
        assert np.array_equal(R.words_to_grids(d, st[:, 11:11 + depth])[live], got[0][live])
        x, z = V.codes_to_xz(got[1])
        bits = lambda planes: np.array([sum(int(b) << q for q, b in enumerate(row)) for row in planes], dtype=np.uint64)
        assert np.array_equal(st[live, 0], bits(x)[live]) and np.array_equal(st[live, 1], bits(z)[live])
        env.close()


# ---- 5. the verdict, every referee kind ------------------------------------------------------------------------------------------------------
class _TablePredict:
    """Component tables behind the reference's `.predict` protocol, vectorised (oracle/ conventions only)."""

    def __init__(self, d, model, lut_x, lut_z):
        m = lattice.Masks(d)
        self.model, self.lut = model, {3: np.asarray(lut_x), 1: np.asarray(lut_z)}
        self.cols = {t: [(a * (d + 1) + b, m.ref_bit[s]) for s, (a, b) in enumerate(m.order) if m.stab_type[s] == t] for t in (3, 1)}

    def predict(self, x, batch_size=None, verbose=0):
        x = np.asarray(x).astype(np.int64)
        idx = {t: sum(x[:, c] << bit for c, bit in self.cols[t]) for t in (3, 1)}
        cls = self.lut[3][idx[3]].astype(np.int64)
        if self.model != "X":
            cls = cls + 2 * self.lut[1][idx[1]]
        out = np.zeros((len(x), 2 if self.model == "X" else 4), dtype=np.float32)
        out[np.arange(len(x)), cls] = 1.0
        return out


def _random_stack(dq, rng, d, classes, hidden=(96, 40)):
    Rf = importlib.import_module("deepq-decoding_amd.referee")
    dims = [(d + 1) ** 2] + list(hidden) + [classes]
    w = []
    for a, b in zip(dims, dims[1:]):
        w += [(rng.randn(a, b) * (1.5 / np.sqrt(a))).astype(np.float32), (rng.randn(b) * 0.3).astype(np.float32)]
    return Rf.FeedForwardReferee(w)


def _referee_case(dq, kind, d, model):
    """(the `referee=` argument of VectorEnv, the restatement's classify(words)) for one referee kind."""
    from oracle import c_oracle
    n_tab = 1 << ((d * d - 1) // 2)
    rng = np.random.RandomState(100 * d + len(kind))
    if kind == "lut":
        lx, lz = c_oracle.luts(d)
        return "lut", V.classify_with(referee.LutReferee(d, model, lx, lz))
    if kind == "ml":
        q = 0.03
        return ("ml", q), V.classify_with(referee.LutReferee(d, model, referee.build_ml_lut(d, 3, q), referee.build_ml_lut(d, 1, q)))
    lx, lz = (rng.rand(n_tab) < 0.5).astype(np.uint8), (rng.rand(n_tab) < 0.5).astype(np.uint8)
    if kind == "pair":
        return (lx, lz), V.classify_with(referee.LutReferee(d, model, lx, lz))
    if kind == "joint":
        return _TablePredict(d, model, lx, lz), V.classify_with(referee.LutReferee(d, model, lx, lz))
    if kind == "mlp":
        ff = _random_stack(dq, rng, d, 2 if model == "X" else 4)
        ff.on_device = True                                      # evaluated on the device at d = 5 too (a table would fit there)
        return ff, V.classify_with_predict(d, ff.logits_exact)
    raise ValueError(kind)


def _pairs(d, n, rng):
    """Random (hidden, frame) code arrays whose residual is empty (30 %), of weight 1-2 (30 %) or heavy (40 %)."""
    hidden = rng.randint(0, 4, size=(n, d * d))
    res = np.zeros((n, d * d), dtype=np.int64)
    kind = rng.rand(n)
    for i in range(n):
        w = 0 if kind[i] < 0.3 else (rng.randint(1, 3) if kind[i] < 0.6 else rng.randint(d, 2 * d + 1))
        res[i, rng.choice(d * d, size=w, replace=False)] = rng.randint(1, 4, size=w)
    hx, hz = V.codes_to_xz(hidden)
    rx, rz = V.codes_to_xz(res)
    frame = V.xz_to_codes(d, hx ^ rx, hz ^ rz)
    return hidden.reshape(n, d, d).astype(np.uint8), frame


VERDICT_CASES = [("lut", 3, "X"), ("lut", 3, "DP"), ("lut", 5, "DP"), ("lut", 5, "IIDXZ"), ("lut", 7, "DP"), ("lut", 7, "X"),
                 ("ml", 3, "DP"), ("ml", 5, "X"), ("ml", 5, "DP"), ("pair", 3, "DP"), ("pair", 5, "DP"), ("pair", 7, "DP"),
                 ("joint", 3, "X"), ("joint", 3, "DP"), ("joint", 5, "DP"), ("mlp", 7, "DP"), ("mlp", 7, "X"), ("mlp", 5, "DP"), ("mlp", 3, "DP")]


@pytest.mark.parametrize("kind,d,model", VERDICT_CASES, ids=[f"{k}_d{d}_{m}" for k, d, m in VERDICT_CASES])
def test_verdict_equals_the_restatement_for_every_referee_kind(dq, torch_mod, kind, d, model):
    D = dq.decoder
    n = 4097
    arg, classify = _referee_case(dq, kind, d, model)
    if kind == "pair":                                          # caller tables (dq_env_set_referee)
        env = dq.VectorEnv(n_envs=4, d=d, error_model=model, use_Y=False, volume_depth=3, referee=None)
        env.set_referee(*arg)
    else:
        env = dq.VectorEnv(n_envs=4, d=d, error_model=model, use_Y=False, volume_depth=3, referee=arg)
    hidden, frame = _pairs(d, n, np.random.RandomState(7 * d + len(kind)))
    if model == "X":                                            # the bit-flip model's errors and corrections are X only
        hidden, frame = (hidden != 0).astype(np.uint8), (frame != 0).astype(np.uint8)
    want = V.verdict(d, hidden, frame, classify)
    got, res = D.verdict(hidden, frame, env, chunk=1500, to_host=True)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    s, a = V.flags(want)
    # the residual is empty for ~30 % (success), light for ~30 %, heavy for ~40 %: a referee of any quality names the class of a fair share of the
    # light and heavy ones (alive) and misses a fair share of the heavy ones (dead); a twentieth of the batch each is far inside that
    assert s.sum() >= n // 20 and (a & ~s).sum() >= n // 20 and (~a).sum() >= n // 20, (s.sum(), (a & ~s).sum(), (~a).sum())
    assert res.counters == dict(zip(D.COUNTER_NAMES, D.counters_from_arrays(want)))
    # no correction: the verdict on the error itself
    got0, _ = D.verdict(hidden, None, env, to_host=True)
    assert np.array_equal(got0, V.verdict(d, hidden, None, classify))
    # the frame equal to the error: a success whatever the referee
    got1, res1 = D.verdict(hidden, hidden, env, to_host=True)
    assert V.flags(got1)[0].all() and res1.n_success == n and res1.failure_rate == 0.0
    env.close()


# ---- 6. the verdict is the environment's, on volumes that stop with the identity --------------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True])
def test_verdict_equals_the_environment_on_the_stopping_step(dq, torch_mod, masked):
    torch = torch_mod
    D = dq.decoder
    cfg, p, n_env = DP5, 0.007, 512
    d, depth = cfg["d"], cfg["volume_depth"]
    A, layers = lattice.num_actions(d, cfg["error_model"], cfg["use_Y"])
    shape = (depth + layers, 2 * d + 1, 2 * d + 1)
    env = dq.VectorEnv(n_envs=n_env, p_phys=p, p_meas=p, seed=(77, 5), **cfg)
    net = dq.QNetwork(shape, shipped.C_LAYERS, shipped.FF_LAYERS, A, max_batch=n_env)
    params = torch.from_numpy(shipped.shipped_weights("d5_dp", str(P))[1]).cuda()
    dec = D.BatchDecoder(shape, shipped.C_LAYERS, shipped.FF_LAYERS, A, d, cfg["error_model"], cfg["use_Y"], depth, masked_greedy=masked,
                         obs_form="uint8", chunk=n_env)
    env.reset()
    st0 = env.export_state().cpu().numpy().view(np.uint64)
    grids = R.words_to_grids(d, st0[:, 11:11 + depth])
    hidden0 = np.stack([np.asarray(V.xz_to_codes(d, np.array([[(int(x) >> q) & 1 for q in range(d * d)]]),
                                                 np.array([[(int(z) >> q) & 1 for q in range(d * d)]]))[0]) for x, z in zip(st0[:, 0], st0[:, 1])])
    actions = [[] for _ in range(n_env)]
    stop = [None] * n_env                                       # (reward, done, done before the step) of the stopping step
    running = np.ones(n_env, bool)
    for t in range(A + 1):
        done_before = env.done.cpu().numpy().astype(bool)
        q = net.forward(params, env.obs)
        a = env.act_step(t, q=q, eps=0.0, masked_greedy=masked, auto_reset=False).cpu().numpy()
        reward, done = env.reward.cpu().numpy(), env.done.cpu().numpy().astype(bool)
        for i in np.nonzero(running)[0]:
            if a[i] == A - 1 or int(a[i]) in actions[i]:
                running[i] = False
                stop[i] = (float(reward[i]), bool(done[i]), bool(done_before[i]))
            else:
                actions[i].append(int(a[i]))
        if not running.any():
            break
    assert not running.any()
    res = dec.decode(params, grids)
    assert [list(map(int, res.corrections[i, :res.n_corrections[i]])) for i in range(n_env)] == actions
    verdict, _ = D.verdict(hidden0, res.frame, env, to_host=True)
    success, alive = V.flags(verdict)
    ident = np.nonzero(res.status == R.IDENTITY)[0]
    assert len(ident) >= n_env // 2, len(ident)
    for i in ident:
        reward, done, done_before = stop[i]
        # (the environment's `done` is sticky until a reset: a lattice the referee lost on an earlier correction stays done)
        assert (reward == 1.0) == bool(success[i]) and done == (done_before or not alive[i]), (i, stop[i], int(verdict[i]))
    assert sum(1 for i in ident if not stop[i][2]) >= n_env // 2
    dec.close()
    env.close()


# ---- 7. evaluate(): counters, chunking, the separate calls, the rate sweep ---------------------------------------------------------------------
def test_evaluate_counters_chunking_and_the_separate_calls(dq, torch_mod, dp_agent):
    agent, env = dp_agent
    D = dq.decoder
    n, base = 10000, 12345
    full = agent.decode_benchmark(env, n, chunk=n, env_id_base=base, return_volumes=True, no_decoder=True)
    host = lambda t: t.cpu().numpy()
    dec = full.decode
    assert list(full.counters.values()) == D.counters_from_arrays(host(full.verdict), host(full.trivial), host(dec.status), host(dec.n_corrections))
    assert full.n_volumes == n and 0 < full.n_trivial < n and 0 < full.n_success <= n
    assert full.n_identity + full.n_repeat + full.n_stopped == n
    # the separate calls
    vol, hid, triv = D.sample_volumes(env, n, env_id_base=base)
    assert all(torch_mod.equal(a, b) for a, b in ((vol, full.volumes), (hid, full.hidden), (triv, full.trivial)))
    res = agent.decode(vol, to_host=False, chunk=n)
    for f in ("corrections", "n_corrections", "frame", "status"):
        assert torch_mod.equal(getattr(res, f), getattr(dec, f)), f
    verd, vres = D.verdict(hid, res.frame, env)
    assert torch_mod.equal(verd, full.verdict)
    assert all(vres.counters[k] == full.counters[k] for k in ("volumes", "in_codespace", "success", "alive"))
    verd0, vres0 = D.verdict(hid, None, env)
    assert all(vres0.counters[k] == full.no_decoder.counters[k] for k in ("volumes", "in_codespace", "success", "alive"))
    assert full.no_decoder.n_trivial == full.n_trivial
    # against the restatement (the sampler and the verdict; the decode has its own tests)
    lx, lz = importlib.import_module("oracle.c_oracle").luts(5)
    want = V.verdict(5, host(hid), host(res.frame), V.classify_with(referee.LutReferee(5, "DP", lx, lz)))
    assert np.array_equal(host(verd), want)
    # chunk sizes
    for chunk in (1000, 4096):
        r = agent.decode_benchmark(env, n, chunk=chunk, env_id_base=base, return_volumes=True, no_decoder=True)
        assert r.counters == full.counters and r.no_decoder.counters == full.no_decoder.counters, chunk
        assert torch_mod.equal(r.verdict, full.verdict) and torch_mod.equal(r.volumes, full.volumes) and torch_mod.equal(r.decode.frame, dec.frame)
        lean = agent.decode_benchmark(env, n, chunk=chunk, env_id_base=base)
        assert lean.counters == full.counters and lean.volumes is None


def test_rate_sweep_equals_one_call_per_rate(dq, torch_mod, dp_agent):
    agent, env = dp_agent
    rates, m, base = [0.003, 0.007, 0.011], 3000, 500
    sweep = agent.decode_benchmark(env, m, rates=rates, env_id_base=base, chunk=4096)         # (chunks straddle the rates' blocks)
    assert list(sweep) == rates
    previous = env.p_phys
    for k, r in enumerate(rates):
        env.set_rates(r)
        one = agent.decode_benchmark(env, m, env_id_base=base + k * m, chunk=4096)
        assert one.counters == sweep[r].counters, r
        assert sweep[r].p_phys == r and sweep[r].n_volumes == m
    env.set_rates(previous)
    assert sweep[0.003].failure_rate < sweep[0.011].failure_rate
    mixed = agent.decode_benchmark(env, m, rates=[0.007], p_meas=0.0, env_id_base=base + m)
    assert mixed[0.007].n_volumes == m and mixed[0.007].counters != sweep[0.007].counters


# ---- 8. anchors that need no measured number ----------------------------------------------------------------------------------------------
def test_no_noise_is_always_a_success(dq, torch_mod, dp_agent):
    agent, env = dp_agent
    n = 5000
    r = agent.decode_benchmark(env, n, rates=[0.0], masked_greedy=True, no_decoder=True)[0.0]
    assert r.n_trivial == n and r.n_success == n and r.n_alive == n and r.n_corrections == 0 and r.n_identity == n
    assert r.no_decoder.n_success == n and r.failure_rate == 0.0 and r.failure_interval[0] == 0.0


# ---- 9. the shipped agent against no decoder ----------------------------------------------------------------------------------------------------
def test_the_shipped_agent_beats_no_decoder(dq, torch_mod, dp_agent):
    agent, env = dp_agent
    n = 1 << 18
    r = agent.decode_benchmark(env, n, rates=[P], masked_greedy=True, no_decoder=True, chunk=1 << 18)[P]
    print(f"\nd5_dp p={P} N={n}: agent success {r.n_success} failure {r.failure_rate:.6f} {r.failure_interval}; "
          f"no decoder success {r.no_decoder.n_success} failure {r.no_decoder.failure_rate:.6f} {r.no_decoder.failure_interval}; "
          f"trivial {r.n_trivial} status {r.status_histogram} mean corrections {r.mean_corrections:.4f}")
    assert r.n_success > r.no_decoder.n_success
