"""Batched decoding on the device (DQNAgent.decode, decoder.BatchDecoder, csrc/decode.hip) against the per-call path, the environment and
the README's known answer (DESIGN.md "Batched decoding").

Exactness: decode and the per-call dqn.forward loop run the same fused forward, so their choices agree exactly.  Where two paths of
different summation order (patch words vs uint8 images, or the batched vs the single-sample forward) choose differently, the test shows
the step is a near-tie: the float64 oracle's top-two gap there is within the forward's documented bound max(1e-5, 2e-6 max |Q|)."""
import numpy as np
import pytest

import decode_ref as R
import shipped
from oracle import dqn_oracle as O
from oracle import lattice

pytestmark = pytest.mark.gpu

P = 0.007
N_REAL = 2000
LATTICE = {fam: dict(cfg) for fam, cfg in shipped.CONFIGS.items()}


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _agent(dq, family, env=None):
    weights, flat = shipped.shipped_weights(family, str(P))
    cfg = LATTICE[family]
    if env is None:
        env = dq.Surface_Code_Environment_Multi_Decoding_Cycles(p_phys=P, p_meas=P, static_decoder=None, **cfg)
    model = dq.build_convolutional_nn(shipped.C_LAYERS, shipped.FF_LAYERS, env.observation_space.shape, env.num_actions)
    agent = dq.DQNAgent(model=model, nb_actions=env.num_actions, memory=dq.SequentialMemory(limit=1000, window_length=1), nb_steps_warmup=100,
                        target_model_update=100, policy=dq.GreedyQPolicy(masked_greedy=True), test_policy=dq.GreedyQPolicy(masked_greedy=True),
                        gamma=0.99, enable_dueling_network=True)
    agent.compile(dq.Adam(lr=1e-4))
    agent._bind(env)
    agent.model.set_weights(weights)
    return agent, flat, env


def real_volumes(dq, cfg, n, p=P, seed=(0xDEC0, 0xDE)):
    """n volumes of the environment at rate p: each lattice's first volume after reset, as grids uint8 [n, depth, d+1, d+1]."""
    env = dq.VectorEnv(n_envs=n, p_phys=p, p_meas=p, seed=seed, **cfg)
    env.reset()
    st = env.export_state().cpu().numpy().view(np.uint64)
    return R.words_to_grids(cfg["d"], st[:, 11:11 + cfg["volume_depth"]])


@pytest.fixture(scope="module", params=["d5_x", "d5_dp"])
def family_agent(request, dq, torch_mod):
    fam = request.param
    agent, flat, env = _agent(dq, fam)
    grids = real_volumes(dq, LATTICE[fam], N_REAL)
    yield fam, agent, flat, grids
    agent._decoder = None


def _spec(family):
    cfg = LATTICE[family]
    A, layers = lattice.num_actions(cfg["d"], cfg["error_model"], cfg["use_Y"])
    n = 2 * cfg["d"] + 1
    return O.QNetSpec((cfg["volume_depth"] + layers, n, n), shipped.C_LAYERS, shipped.FF_LAYERS, A)


def _lists(res):
    return [list(map(int, res.corrections[i, :res.n_corrections[i]])) for i in range(len(res.n_corrections))]


def assert_same_or_near_tie(family, flat, grids, got, want, masked, max_disagree):
    """Per volume: equal action lists, or the first differing step is a near-tie of the float64 oracle."""
    cfg = LATTICE[family]
    spec = _spec(family)
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
    return len(bad)


# ---- 1. README known answer ---------------------------------------------------------------------------------------------------------
def test_readme_volume_decodes_to_the_documented_answer(dq, torch_mod):
    agent, flat, env = _agent(dq, "d5_x")
    vol = shipped.readme_faulty_syndromes()
    for form in ("uint8", "patch"):
        res = agent.decode(vol, action_planes="readme", masked_greedy=False, obs_form=form)
        assert res.correction_list() == shipped.README_CORRECTIONS
        assert int(res.status) == R.IDENTITY or int(res.status) == R.REPEAT
        frame = np.zeros((5, 5), np.uint8)
        frame[4, 1] = 1                                             # X on qubit 21
        assert np.array_equal(res.frame, frame)
    # environment mode: the host loop over dqn.forward's Q-values with environment action planes
    for masked in (False, True):
        res = agent.decode(vol, masked_greedy=masked, obs_form="uint8")
        want, frame, status = R.decode_volume(vol, agent.compute_q_values, 5, "X", False, masked)
        assert res.correction_list() == want and np.array_equal(res.frame, frame) and int(res.status) == status


# ---- 2. against the per-call path ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True])
def test_decode_equals_the_forward_loop(family_agent, masked):
    fam, agent, flat, grids = family_agent
    cfg = LATTICE[fam]
    res = agent.decode(grids, masked_greedy=masked, obs_form="uint8")
    got = _lists(res)
    want, frames, stats = [], [], []
    for g in grids:
        c, f, s = R.decode_volume(g, agent.compute_q_values, cfg["d"], cfg["error_model"], cfg["use_Y"], masked)
        want.append(c); frames.append(f); stats.append(s)
    assert_same_or_near_tie(fam, flat, grids, got, want, masked, max_disagree=len(grids) // 200)
    same = [i for i in range(len(grids)) if got[i] == want[i]]
    assert np.array_equal(res.frame[same], np.asarray(frames)[same])
    assert np.array_equal(res.status[same], np.asarray(stats)[same])
    assert np.all(res.corrections[np.arange(res.corrections.shape[1])[None, :] >= res.n_corrections[:, None]] == -1)
    assert int(res.n_corrections.sum()) > 0


# ---- 3. patch words vs uint8 images -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True])
def test_patch_words_equal_uint8_images(family_agent, masked):
    fam, agent, flat, grids = family_agent
    a = agent.decode(grids, masked_greedy=masked, obs_form="uint8")
    b = agent.decode(grids, masked_greedy=masked, obs_form="patch")
    assert agent._decoder.obs_form == "patch"
    n = assert_same_or_near_tie(fam, flat, grids, _lists(b), _lists(a), masked, max_disagree=len(grids) // 200)
    if n == 0:
        assert np.array_equal(a.frame, b.frame) and np.array_equal(a.status, b.status)


# ---- 4. against the environment -----------------------------------------------------------------------------------------------------
ENV_CASES = [("d5_dp", dict(d=5, error_model="DP", use_Y=False, volume_depth=5), 0.007, True),
             ("d7_x", dict(d=7, error_model="X", use_Y=False, volume_depth=5), 0.01, False)]


@pytest.mark.parametrize("name,cfg,p,shipped_w", ENV_CASES, ids=[c[0] for c in ENV_CASES])
@pytest.mark.parametrize("masked", [False, True])
def test_decode_equals_the_environment_stepped_greedily(dq, torch_mod, name, cfg, p, shipped_w, masked):
    torch = torch_mod
    n_env = 512
    d, depth = cfg["d"], cfg["volume_depth"]
    A, layers = lattice.num_actions(d, cfg["error_model"], cfg["use_Y"])
    shape = (depth + layers, 2 * d + 1, 2 * d + 1)
    env = dq.VectorEnv(n_envs=n_env, p_phys=p, p_meas=p, seed=(77, 5), **cfg)
    net = dq.QNetwork(shape, shipped.C_LAYERS, shipped.FF_LAYERS, A, max_batch=n_env)
    if shipped_w:
        params = torch.from_numpy(shipped.shipped_weights("d5_dp", str(P))[1]).cuda()
    else:
        params = net.init_params((11, 12))
    dec = dq.decoder.BatchDecoder(shape, shipped.C_LAYERS, shipped.FF_LAYERS, A, d, cfg["error_model"], cfg["use_Y"], depth,
                                  masked_greedy=masked, obs_form="uint8", chunk=n_env)
    env.reset()
    st0 = env.export_state().cpu().numpy().view(np.uint64)
    grids = R.words_to_grids(d, st0[:, 11:11 + depth])
    actions = [[] for _ in range(n_env)]
    before = [None] * n_env
    running = np.ones(n_env, bool)
    for t in range(A + 1):
        st = env.export_state().cpu().numpy().view(np.uint64)
        q = net.forward(params, env.obs)
        a = env.act_step(t, q=q, eps=0.0, masked_greedy=masked, auto_reset=False).cpu().numpy()
        for i in np.nonzero(running)[0]:
            if a[i] == A - 1 or int(a[i]) in actions[i]:
                running[i] = False
                before[i] = (int(st[i, 0]), int(st[i, 1]))
            else:
                actions[i].append(int(a[i]))
        if not running.any():
            break
    assert not running.any()
    res = dec.decode(params, grids)
    assert _lists(res) == actions
    x0, z0 = st0[:, 0], st0[:, 1]
    for i in range(n_env):
        fx = sum(1 << q for q in range(d * d) if res.frame[i].reshape(-1)[q] in (1, 2))
        fz = sum(1 << q for q in range(d * d) if res.frame[i].reshape(-1)[q] in (2, 3))
        assert before[i] == (int(x0[i]) ^ fx, int(z0[i]) ^ fz), i
    assert sum(len(x) for x in actions) > 0
    dec.close()


# ---- 5. order and chunking ----------------------------------------------------------------------------------------------------------
def test_order_and_chunking_are_bit_identical(dq, torch_mod):
    agent, flat, env = _agent(dq, "d5_dp")
    big = real_volumes(dq, LATTICE["d5_dp"], 1 << 18, seed=(9, 9))
    full = agent.decode(big, chunk=1 << 18)
    assert agent._decoder.obs_form == "patch"
    fields = ("corrections", "n_corrections", "frame", "status")
    n = 5000
    perm = np.random.default_rng(3).permutation(n)
    a = agent.decode(big[:n][perm])
    for f in fields:
        assert np.array_equal(getattr(a, f), getattr(full, f)[:n][perm]), f
    b = agent.decode(big[:n], chunk=777)
    assert len(b.iterations) == -(-n // 777)
    for f in fields:
        assert np.array_equal(getattr(b, f), getattr(full, f)[:n]), f
    one = agent.decode(big[123])
    assert one.correction_list() == list(map(int, full.corrections[123, :full.n_corrections[123]]))


# ---- 6. max_actions -----------------------------------------------------------------------------------------------------------------
def test_max_actions_truncates(family_agent):
    fam, agent, flat, grids = family_agent
    full = agent.decode(grids)
    assert int(full.n_corrections.max()) >= 2
    for k in (1, 2):
        cut = agent.decode(grids, max_actions=k)
        assert cut.corrections.shape == (len(grids), k)
        assert np.array_equal(cut.corrections, full.corrections[:, :k])
        assert np.array_equal(cut.n_corrections, np.minimum(full.n_corrections, k))
        assert np.all(cut.status[full.n_corrections >= k] == R.STOPPED)
        short = full.n_corrections < k
        assert np.array_equal(cut.status[short], full.status[short]) and np.array_equal(cut.frame[short], full.frame[short])


# ---- the forward's range guard --------------------------------------------------------------------------------------------------------
def test_non_finite_weights_raise_instead_of_choosing(dq, torch_mod):
    torch = torch_mod
    _, flat = shipped.shipped_weights("d5_x", str(P))
    bad = flat.copy()
    bad[10] = np.nan
    dec = dq.decoder.BatchDecoder((6, 11, 11), shipped.C_LAYERS, shipped.FF_LAYERS, 26, 5, "X", False, 5, chunk=64)
    with pytest.raises(dq.DeepQError) as ei:
        dec.decode(torch.from_numpy(bad).cuda(), shipped.readme_faulty_syndromes())
    assert ei.value.status == dq._lib.DQ_ERR_RANGE and "forward" in str(ei.value)
    res = dec.decode(torch.from_numpy(flat).cuda(), shipped.readme_faulty_syndromes())          # healthy weights: the guard stays silent
    assert res.n_corrections >= 0
    dec.close()
