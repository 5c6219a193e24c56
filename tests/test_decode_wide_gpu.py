"""Batched agent decoding at d = 9 .. 15 on the device (DQNAgent.decode_wide / decode_benchmark_wide, decoder_wide.WideBatchDecoder,
csrc/decode_wide.hip): against the narrow decode where both exist, against the numpy restatement (tests/decode_ref.py) under supplied
Q rows and under a network whose choice depends on the action planes, against the wide environment stepped greedily, and the scorer against
memory_experiment_wide.

Exactness: the stepping tests feed Q rows of multiples of 1/8, so every comparison is exact.  The run tests compare with the per-call forward loop, a forward
of another batch shape: a differing volume is accepted only where the float64 oracle shows its first differing step to be a near-tie inside the forward's
bound max(1e-5, 2e-6 max |Q|), and at most one volume in 100 may differ."""
import functools

import numpy as np
import pytest

import decode_ref as R
import decode_wide_ref as WR
import shipped
from oracle import dqn_oracle as O
from oracle import lattice

pytestmark = pytest.mark.gpu

FIELDS = ("corrections", "n_corrections", "frame", "status")


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return torch


def env_volumes(dq, cfg, n, p, seed):
    """n volumes of the environment at rate p: each lattice's first volume after reset, read back from the observation's syndrome planes."""
    env = dq.VectorEnv(n_envs=n, p_phys=p, p_meas=p, seed=seed, **cfg)
    try:
        env.reset()
        return np.ascontiguousarray(env.obs.cpu().numpy()[:, :cfg["volume_depth"], ::2, ::2])
    finally:
        env.close()


def make_agent(dq, cfg, weights, masked=True, p=0.01):
    env = dq.VectorEnv(n_envs=2, p_phys=p, p_meas=p, seed=(5, 6), **cfg)
    model = dq.build_convolutional_nn(WR.C_LAYERS, WR.FF_LAYERS, env.obs_shape, env.num_actions)
    agent = dq.DQNAgent(model=model, nb_actions=env.num_actions, memory=dq.SequentialMemory(limit=64, window_length=1), nb_steps_warmup=100,
                        target_model_update=100, policy=dq.GreedyQPolicy(masked_greedy=masked), test_policy=dq.GreedyQPolicy(masked_greedy=masked),
                        gamma=0.99, enable_dueling_network=True)
    agent.compile(dq.Adam(lr=1e-4))
    agent._bind(env)
    agent.model.set_weights(weights)
    return agent, env


def release(agent):
    for name in ("_wide_decoder", "_decoder"):
        dec = getattr(agent, name, None)
        if dec is not None:
            dec.close()
        setattr(agent, name, None)
    agent._wide_decoder_key = agent._decoder_key = None


# ---- 1. wide equals narrow where both exist -------------------------------------------------------------------------------------------------
NARROW = {"d5_x": dict(shipped.CONFIGS["d5_x"]), "d5_dp": dict(shipped.CONFIGS["d5_dp"]),
          "d3_dp": dict(d=3, error_model="DP", use_Y=False, volume_depth=3), "d7_dp": dict(d=7, error_model="DP", use_Y=False, volume_depth=5)}


@pytest.mark.parametrize("name", sorted(NARROW))
def test_wide_equals_narrow_where_both_exist(dq, torch_mod, name):
    cfg = NARROW[name]
    grids = env_volumes(dq, cfg, 500, 0.02, (0xDEC0, 0xDE))
    if name in shipped.CONFIGS:
        weights = shipped.shipped_weights(name, "0.007")[0]
    else:
        spec, flat = WR.sensitive_network(cfg, grids[:100])
        weights = WR.weights_of(spec, flat)
    agent, env = make_agent(dq, cfg, weights)
    try:
        n_actions = 0
        for masked in (False, True):
            wide = agent.decode_wide(grids, masked_greedy=masked, chunk=512)
            narrow = agent.decode(grids, masked_greedy=masked, obs_form="uint8", chunk=512)
            for f in FIELDS:
                assert np.array_equal(getattr(wide, f), getattr(narrow, f)), (name, masked, f)
            assert wide.iterations == narrow.iterations
            n_actions += int(wide.n_corrections.sum())
        assert n_actions > 0
    finally:
        release(agent)
        env.close()


# ---- 2. stepping against the numpy restatement ----------------------------------------------------------------------------------------------
STEP_CFG = [dict(d=9, error_model="X", use_Y=False, volume_depth=3), dict(d=9, error_model="DP", use_Y=False, volume_depth=5),
            dict(d=13, error_model="DP", use_Y=False, volume_depth=3), dict(d=11, error_model="DP", use_Y=True, volume_depth=4),
            dict(d=15, error_model="DP", use_Y=True, volume_depth=16)]
STEP_ACTIONS = [82, 163, 339, 364, 676]
STEP_IDS = ["d9_x_depth3", "d9_dp_depth5", "d13_dp_depth3", "d11_dpy_depth4", "d15_dpy_depth16"]
STEP_N, STEP_MAX = 256, 12


def step_inputs(k, n=STEP_N):
    cfg = STEP_CFG[k]
    A, _ = lattice.num_actions(cfg["d"], cfg["error_model"], cfg["use_Y"])
    assert A == STEP_ACTIONS[k]
    return cfg, A, WR.sparse_grids(cfg, STEP_N, seed=100 + k)[:n]


@functools.lru_cache(maxsize=None)
def step_reference(k, masked):
    """The restatement's (lists, frames, statuses) of configuration k at max_actions = 12: computed once, shared, never changed."""
    cfg, A, grids = step_inputs(k)
    return WR.reference_decode(cfg, grids, WR.SuppliedQ(STEP_N, A, seed=7 + k), masked, STEP_MAX)


def drive(torch, dec, grids, supplied):
    """pack, then steps with the supplied rows of the volumes still active, uploaded per iteration.  Returns (host outputs, iterations)."""
    out = dec.pack(grids)
    n_active, it = len(grids), 0
    while n_active:
        act, count = dec.active()
        assert count == n_active
        idx = act.cpu().numpy()
        assert np.all(np.diff(idx) > 0)                              # the compaction is stable: the active list stays sorted
        n_active = dec.step(torch.from_numpy(supplied.rows(it)[idx]))
        it += 1
    return [x.cpu().numpy() for x in out], it


def check_against_reference(cfg, A, grids, dec, got, want, max_actions):
    corr, ncorr, frame, status = got
    lists, frames, stats = want
    n = len(grids)
    assert [list(map(int, corr[i, :ncorr[i]])) for i in range(n)] == lists
    assert np.all(corr[np.arange(max_actions)[None, :] >= ncorr[:, None]] == -1)
    assert np.array_equal(frame, frames) and np.array_equal(status, stats)
    rows = dec.rows(n).cpu().numpy()
    legal, completed = (WR.words_to_sets(w.cpu().numpy()) for w in dec.words(n))
    for i in range(n):
        obs, want_legal = R.state_after(grids[i], lists[i], cfg["d"], cfg["error_model"], cfg["use_Y"])
        assert np.array_equal(rows[i], obs), i
        assert legal[i] == want_legal and completed[i] == set(lists[i]), i
        assert max(legal[i]) == A - 1


def wide_decoder(dq, cfg, A, masked, max_actions, chunk):
    layers = lattice.num_actions(cfg["d"], cfg["error_model"], cfg["use_Y"])[1]
    shape = (cfg["volume_depth"] + layers, 2 * cfg["d"] + 1, 2 * cfg["d"] + 1)
    return dq.WideBatchDecoder(shape, WR.C_LAYERS, WR.FF_LAYERS, A, cfg["d"], cfg["error_model"], cfg["use_Y"], cfg["volume_depth"],
                               masked_greedy=masked, max_actions=max_actions, chunk=chunk)


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("k", range(len(STEP_CFG)), ids=STEP_IDS)
def test_stepping_equals_the_restatement(dq, torch_mod, k, masked):
    cfg, A, grids = step_inputs(k)
    dec = wide_decoder(dq, cfg, A, masked, STEP_MAX, STEP_N)
    try:
        got, it = drive(torch_mod, dec, grids, WR.SuppliedQ(STEP_N, A, seed=7 + k))
        assert it <= STEP_MAX
        check_against_reference(cfg, A, grids, dec, got, step_reference(k, masked), STEP_MAX)
    finally:
        dec.close()


@pytest.mark.parametrize("k", range(len(STEP_CFG)), ids=STEP_IDS)
def test_stepping_cases_reach_all_three_statuses(k):
    stats = np.concatenate([step_reference(k, masked)[2] for masked in (False, True)])
    for code in (R.IDENTITY, R.REPEAT, R.STOPPED):
        assert int((stats == code).sum()) >= 5, (STEP_IDS[k], code)


@pytest.mark.parametrize("k", range(len(STEP_CFG)), ids=STEP_IDS)
def test_stepping_to_the_natural_end(dq, torch_mod, k):
    cfg, A, grids = step_inputs(k, n=8)
    dec = wide_decoder(dq, cfg, A, False, A - 1, 8)
    try:
        got, it = drive(torch_mod, dec, grids, WR.SuppliedQ(8, A, seed=50 + k))
        want = WR.reference_decode(cfg, grids, WR.SuppliedQ(8, A, seed=50 + k), False, A - 1)
        check_against_reference(cfg, A, grids, dec, got, want, A - 1)
        assert it == max(len(c) + (s != R.STOPPED) for c, s in zip(want[0], want[2]))
    finally:
        dec.close()


def test_a_non_finite_supplied_q_is_refused_and_the_handle_serves_the_next_decode(dq, torch_mod):
    cfg, A, grids = step_inputs(0, n=8)
    dec = wide_decoder(dq, cfg, A, True, STEP_MAX, 8)
    try:
        dec.pack(grids)
        q = WR.SuppliedQ(8, A, seed=1).rows(0).copy()
        q[5, 3] = np.inf                                             # not even a legal action's value: the row is not to be chosen from
        with pytest.raises(dq.DeepQError) as ei:
            dec.step(torch_mod.from_numpy(q))
        assert ei.value.status == dq._lib.DQ_ERR_RANGE
        with pytest.raises(dq.DeepQError) as ei:                     # the decode is over
            dec.step(torch_mod.from_numpy(q))
        assert ei.value.status == dq._lib.DQ_ERR_STATE
        got, _ = drive(torch_mod, dec, grids, WR.SuppliedQ(8, A, seed=7))
        want = WR.reference_decode(cfg, grids, WR.SuppliedQ(8, A, seed=7), True, STEP_MAX)
        check_against_reference(cfg, A, grids, dec, got, want, STEP_MAX)
    finally:
        dec.close()


# ---- 3. run against the per-call loop -------------------------------------------------------------------------------------------------------
RUN = {"d9_dp": (dict(d=9, error_model="DP", use_Y=False, volume_depth=3), 150), "d15_dpy": (dict(d=15, error_model="DP", use_Y=True, volume_depth=3), 60)}
RUN_P = 0.03


@pytest.fixture(scope="module", params=sorted(RUN))
def run_agent(request, dq, torch_mod):
    cfg, n = RUN[request.param]
    grids = env_volumes(dq, cfg, n, RUN_P, (0xDEC0, 0x0D))
    spec, flat = WR.sensitive_network(cfg, grids)
    agent, env = make_agent(dq, cfg, WR.weights_of(spec, flat))
    yield request.param, cfg, spec, flat, grids, agent
    release(agent)
    env.close()


def assert_same_or_near_tie(cfg, spec, flat, grids, got, want, masked, max_disagree):
    """Per volume: equal action lists, or the first differing step is a near-tie of the float64 oracle (tests/test_decode_gpu.py)."""
    bad = [i for i in range(len(want)) if got[i] != want[i]]
    assert len(bad) <= max_disagree, (len(bad), bad[:5])
    for i in bad:
        k = 0
        while k < min(len(got[i]), len(want[i])) and got[i][k] == want[i][k]:
            k += 1
        obs, legal = R.state_after(grids[i], got[i][:k], cfg["d"], cfg["error_model"], cfg["use_Y"])
        q = O.forward(spec, flat, obs[None])[0][0]
        cand = np.asarray(sorted(legal) if masked else range(len(q)))
        top = np.sort(q[cand])[-2:]
        tol = max(1e-5, 2e-6 * float(np.abs(q).max()))
        assert top[1] - top[0] <= tol, (i, got[i], want[i], top[1] - top[0], tol)
    return bad


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("max_actions", [3, 8])
def test_run_equals_the_forward_loop(run_agent, max_actions, masked):
    name, cfg, spec, flat, grids, agent = run_agent
    res = agent.decode_wide(grids, masked_greedy=masked, max_actions=max_actions)
    got = WR.lists(res)
    want, frames, stats = [], [], []
    for g in grids:
        c, f, s = R.decode_volume(g, agent.compute_q_values, cfg["d"], cfg["error_model"], cfg["use_Y"], masked, max_actions=max_actions)
        want.append(c); frames.append(f); stats.append(s)
    bad = assert_same_or_near_tie(cfg, spec, flat, grids, got, want, masked, max_disagree=len(grids) // 100)
    same = [i for i in range(len(grids)) if i not in bad]
    assert np.array_equal(res.frame[same], np.asarray(frames)[same])
    assert np.array_equal(res.status[same], np.asarray(stats)[same])
    assert np.all(res.corrections[np.arange(max_actions)[None, :] >= res.n_corrections[:, None]] == -1)
    assert int(res.n_corrections.sum()) > 0
    if max_actions == 3:
        for code in (R.IDENTITY, R.REPEAT, R.STOPPED):
            assert int((res.status == code).sum()) >= 1, (name, code)


# ---- 4. the environment stepped greedily ----------------------------------------------------------------------------------------------------
ENV_CASES = {"d9_dp_depth5": dict(d=9, error_model="DP", use_Y=False, volume_depth=5), "d11_x_depth3": dict(d=11, error_model="X", use_Y=False, volume_depth=3)}


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("name", sorted(ENV_CASES))
def test_decode_wide_equals_the_wide_environment_stepped_greedily(dq, torch_mod, name, masked):
    torch = torch_mod
    cfg, n_env = ENV_CASES[name], 64
    A, layers = lattice.num_actions(cfg["d"], cfg["error_model"], cfg["use_Y"])
    env = dq.VectorEnv(n_envs=n_env, p_phys=0.02, p_meas=0.02, seed=(77, 5), **cfg)
    assert env.wide
    net = dq.QNetwork(env.obs_shape, WR.C_LAYERS, WR.FF_LAYERS, A, max_batch=n_env)
    dec = wide_decoder(dq, cfg, A, masked, None, n_env)
    try:
        env.reset()
        grids = np.ascontiguousarray(env.obs.cpu().numpy()[:, :cfg["volume_depth"], ::2, ::2])
        params = torch.from_numpy(WR.sensitive_network(cfg, grids)[1]).cuda()
        actions = [[] for _ in range(n_env)]
        running = np.ones(n_env, bool)
        for t in range(A + 1):
            q = net.forward(params, env.obs)
            a = env.act_step(t, q=q, eps=0.0, masked_greedy=masked, auto_reset=False).cpu().numpy()
            for i in np.nonzero(running)[0]:
                if a[i] == A - 1 or int(a[i]) in actions[i]:
                    running[i] = False
                else:
                    actions[i].append(int(a[i]))
            if not running.any():
                break
        assert not running.any()
        res = dec.decode(params, grids)
        assert WR.lists(res) == actions
        assert sum(len(x) for x in actions) > n_env // 2
    finally:
        dec.close()
        net.close()
        env.close()


# ---- 5. order, chunking, partitions ---------------------------------------------------------------------------------------------------------
def test_order_chunking_and_partitions_are_bit_identical(dq, torch_mod):
    cfg = dict(d=9, error_model="X", use_Y=False, volume_depth=3)
    n = 2 * 1024 + 37
    grids = env_volumes(dq, cfg, n, 0.03, (9, 9))
    spec, flat = WR.sensitive_network(cfg, grids[:150])
    agent, env = make_agent(dq, cfg, WR.weights_of(spec, flat))
    try:
        full = agent.decode_wide(grids, chunk=4096)
        assert len(full.iterations) == 1 and full.iterations[0] >= 2
        assert int((full.n_corrections >= 1).sum()) > 1024          # more than one compaction partition is still active after the first iteration
        for chunk in (1000, 64):
            part = agent.decode_wide(grids, chunk=chunk)
            assert len(part.iterations) == -(-n // chunk)
            for f in FIELDS:
                assert np.array_equal(getattr(part, f), getattr(full, f)), (chunk, f)
        perm = np.random.default_rng(3).permutation(n)
        mixed = agent.decode_wide(grids[perm], chunk=4096)
        for f in FIELDS:
            assert np.array_equal(getattr(mixed, f), getattr(full, f)[perm]), f
        one = agent.decode_wide(grids[123])
        assert one.correction_list() == list(map(int, full.corrections[123, :full.n_corrections[123]]))
    finally:
        release(agent)
        env.close()


# ---- 6. non-finite weights raise ------------------------------------------------------------------------------------------------------------
def test_non_finite_weights_raise_instead_of_choosing(dq, torch_mod):
    torch = torch_mod
    cfg = dict(d=9, error_model="DP", use_Y=False, volume_depth=3)
    grids = WR.sparse_grids(cfg, 16, seed=4)
    spec, flat = WR.sensitive_network(cfg, grids)
    bad = flat.copy()
    bad[-7] = np.nan                                                # one bias of the last Dense layer
    dec = wide_decoder(dq, cfg, 163, False, None, 64)
    try:
        with pytest.raises(dq.DeepQError) as ei:
            dec.decode(torch.from_numpy(bad).cuda(), grids)
        assert ei.value.status == dq._lib.DQ_ERR_RANGE
        res = dec.decode(torch.from_numpy(flat).cuda(), grids)      # healthy weights: the guard stays silent
        assert np.all(res.n_corrections >= 0) and np.all(res.status >= 1)
    finally:
        dec.close()


# ---- 7. scoring -----------------------------------------------------------------------------------------------------------------------------
SCORE_CFG = dict(d=9, error_model="DP", use_Y=False, volume_depth=5)
SCORE_N, SCORE_P, SCORE_SEED, SCORE_BASE = 2048, 0.01, (0xC0DE, 0x5EED), 4096
VERDICT_COUNTERS = ("volumes", "trivial", "in_codespace", "success", "alive", "corrections")


@pytest.fixture(scope="module")
def score_agent(dq, torch_mod):
    grids = env_volumes(dq, SCORE_CFG, 150, 0.03, (2, 3))
    spec, flat = WR.sensitive_network(SCORE_CFG, grids)
    agent, env = make_agent(dq, SCORE_CFG, WR.weights_of(spec, flat), p=SCORE_P)
    yield agent, env, spec, flat
    release(agent)
    env.close()


def test_the_union_find_row_is_memory_experiment_wides(dq, score_agent):
    agent, env, spec, flat = score_agent
    mine, uf = agent.decode_benchmark_wide(env, SCORE_N, seed=SCORE_SEED, env_id_base=SCORE_BASE, baseline="union_find", no_decoder=True)
    want = dq.memory_experiment_wide((9, "DP"), SCORE_N, rounds=5, window=5, commit=5, p_phys=SCORE_P, seed=SCORE_SEED, env_id_base=SCORE_BASE,
                                     no_decoder=True)
    assert uf.counters == want.counters and uf.no_decoder.counters == want.no_decoder.counters
    assert mine.counters["volumes"] == SCORE_N and mine.counters["trivial"] == want.counters["trivial"]
    assert mine.counters["identity"] + mine.counters["repeat"] + mine.counters["stopped"] == SCORE_N
    assert mine.counters["alive"] == mine.counters["success"] and mine.counters["corrections"] > 0
    assert mine.no_decoder.counters == want.no_decoder.counters
    assert uf.counters["success"] > want.no_decoder.counters["success"]        # (the decoder helps at this rate: the rows are not all alike)
    tup = agent.decode_benchmark_wide((9, "DP", False, 5), SCORE_N, p_phys=SCORE_P, seed=SCORE_SEED, env_id_base=SCORE_BASE)
    assert tup.counters == mine.counters                                        # the tuple form with explicit rates and seed: the same volumes


def test_an_agent_that_only_takes_the_identity_scores_as_no_decoder(dq, score_agent):
    agent, env, spec, flat = score_agent
    lazy = flat.copy()
    lazy[-1] += 1e4                                                 # the identity's advantage above every other Q
    agent.model.set_weights(WR.weights_of(spec, lazy))
    try:
        r = agent.decode_benchmark_wide(env, SCORE_N, seed=SCORE_SEED, env_id_base=SCORE_BASE, no_decoder=True)
    finally:
        agent.model.set_weights(WR.weights_of(spec, flat))
    assert r.counters["identity"] == SCORE_N and r.counters["corrections"] == 0
    for name in VERDICT_COUNTERS:
        assert r.counters[name] == r.no_decoder.counters[name], name


def test_rates_equal_one_call_per_rate(dq, score_agent):
    agent, env, spec, flat = score_agent
    a, b = 0.006, 0.02
    both = agent.decode_benchmark_wide(env, SCORE_N, rates=[a, b], seed=SCORE_SEED, env_id_base=SCORE_BASE, baseline="union_find")
    for k, rate in enumerate((a, b)):
        one = agent.decode_benchmark_wide((9, "DP", False, 5), SCORE_N, p_phys=rate, seed=SCORE_SEED, env_id_base=SCORE_BASE + k * SCORE_N,
                                          baseline="union_find")
        for row in (0, 1):
            assert both[row][rate].counters == one[row].counters, (rate, row)
        assert both[0][rate].p_phys == rate
    assert both[1][b].counters["success"] < both[1][a].counters["success"]


@pytest.mark.parametrize("final_round", ["faulty", "perfect"])
def test_returned_volumes_decode_to_the_same_frames(dq, score_agent, final_round):
    agent, env, spec, flat = score_agent
    t = {}
    r = agent.decode_benchmark_wide(env, SCORE_N, seed=SCORE_SEED, env_id_base=SCORE_BASE, return_volumes=True, final_round=final_round, chunk=1024,
                                    timings=t)
    assert set(t) == {"run", "decode", "verdict"} and len(r.decode.iterations) == 2
    assert tuple(r.volumes.shape) == (SCORE_N, 5, 10, 10) and r.counters["volumes"] == SCORE_N
    again = agent.decode_wide(r.volumes, to_host=False)
    for f in FIELDS:
        assert bool((getattr(again, f) == getattr(r.decode, f)).all()), f
    status, ncorr, verdict = r.decode.status.cpu().numpy(), r.decode.n_corrections.cpu().numpy(), r.verdict.cpu().numpy()
    assert dq.decoder.counters_from_arrays(verdict, r.trivial.cpu().numpy(), status, ncorr) == [r.counters[k] for k in dq.decoder.COUNTER_NAMES]
