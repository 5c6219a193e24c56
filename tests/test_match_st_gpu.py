"""The space-time matching baseline on the device (decoder.matching_decode / score_matching, csrc/match_st.hip) against the
two checkers of tests/match_st_ref.py: every frame must pass the certificate -- its reported weight is the minimum, and some fault history of exactly
that weight reproduces the volume with a net data error equivalent to the frame -- so no tie-break of the kernel is replicated here."""
import numpy as np
import pytest

import decode_eval_ref as V
import match_st_ref as M
import shipped
from oracle import lattice, referee

pytestmark = pytest.mark.gpu

SEED = (1234, 5678)


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _env(dq, d, model, depth, p=0.01, ref=None):
    return dq.VectorEnv(n_envs=1, p_phys=p, p_meas=p, seed=SEED, referee=ref, d=d, error_model=model, use_Y=False, volume_depth=depth)


def _volumes_from_defects(d, depth, rows0=None, rows1=None):
    """One volume uint8 [depth, d+1, d+1] whose components have the given defect rows int [depth, n] (S_t = XOR of D_0 .. D_t)."""
    vol = np.zeros((depth, d + 1, d + 1), dtype=np.uint8)
    for comp, rows in ((0, rows0), (1, rows1)):
        if rows is None:
            continue
        C = M.Component(d, comp)
        s = np.bitwise_xor.accumulate(np.asarray(rows, dtype=np.int64), axis=0)
        for j, (a, b) in enumerate(C.cells):
            vol[:, a, b] = s[:, j]
    return vol


def _certify_all(d, depth, vol, res, which=None):
    bad = []
    for i in (range(len(vol)) if which is None else which):
        for comp in (0, 1):
            ok, w_min, hist = M.certify(d, comp, vol[i], res.frame[i], res.weight[i, comp], depth)
            if not ok:
                bad.append((i, comp, int(res.weight[i, comp]), w_min, hist))
    return bad


def _n_defects(d, vol):
    return np.stack([M.Component(d, comp).defects(vol).sum(axis=(1, 2)) for comp in (0, 1)], axis=1)


# ---- 1. exhaustive -------------------------------------------------------------------------------------------------------------------------
def test_every_volume_of_d3_depth2_passes_the_certificate_against_the_search_table(dq, torch_mod):
    d, depth = 3, 2
    m = lattice.Masks(d)
    N = 1 << (depth * m.n_stab)
    idx = np.arange(N, dtype=np.int64)
    vol = np.zeros((N, depth, d + 1, d + 1), dtype=np.uint8)
    for t in range(depth):
        for s, (a, b) in enumerate(m.order):
            vol[:, t, a, b] = (idx >> (t * m.n_stab + s)) & 1
    res = dq.decoder.matching_decode(vol, _env(dq, d, "DP", depth), chunk=20000, to_host=True)
    assert res.frame.shape == (N, d, d) and res.frame.dtype == np.uint8 and res.weight.dtype == np.int32 and res.frame.max() <= 3
    assert not res.inexact.any()
    assert np.array_equal(res.n_defects, _n_defects(d, vol))
    for comp in (0, 1):
        C, T = M.Component(d, comp), M.BfsTable(d, comp, depth)
        D = M.bits(C.defects(vol).reshape(N, -1))
        assert np.array_equal(res.weight[:, comp], T.open[D]), comp
        sig, cls = C.frame_syndrome_class(res.frame)
        m_last = M.bits(sig ^ C.syndromes(vol)[:, depth - 1])
        assert np.array_equal(T.dist[cls, m_last, D], res.weight[:, comp]), comp
    assert len(np.unique(res.frame.reshape(N, -1), axis=0)) > 50              # (not vacuous: many different corrections)


# ---- 2. / 3. depolarising samples ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def d5_sample(dq, torch_mod):
    d, depth, n = 5, 5, 4096
    env = _env(dq, d, "DP", depth, 0.011)
    vol, hid, triv = dq.decoder.sample_volumes(env, n, seed=SEED, to_host=True)
    res = dq.decoder.matching_decode(vol, env, chunk=n, to_host=True)
    return env, vol, res


def test_d5_depolarising_sample_is_decoded_exactly(dq, d5_sample):
    env, vol, res = d5_sample
    nd = _n_defects(5, vol)
    assert nd.max() <= 12                                                       # (computed with the numpy sampler: the exact path alone covers these)
    assert np.array_equal(res.n_defects, nd)
    assert not res.inexact.any()
    assert _certify_all(5, 5, vol, res) == []
    assert (res.frame.reshape(len(vol), -1).max(axis=1) > 0).sum() > 1000 and set(np.unique(res.frame)) == {0, 1, 2, 3}


def test_d7_depolarising_sample(dq, torch_mod):
    d, depth, n = 7, 7, 1024
    env = _env(dq, d, "DP", depth, 0.007)
    vol, hid, triv = dq.decoder.sample_volumes(env, n, seed=SEED, to_host=True)
    res = dq.decoder.matching_decode(vol, env, to_host=True)
    nd = _n_defects(d, vol)
    assert np.array_equal(res.n_defects, nd)
    big = (nd > 14).any(axis=1)
    assert big.sum() <= 11                                                      # (3 volumes in one component, 8 in the other, with the numpy sampler)
    assert not res.inexact[~big].any()                                          # inexact only where a component has more than 14 defects
    assert _certify_all(d, depth, vol, res, np.nonzero(~big)[0]) == []


# ---- 4. hand-built clusters ------------------------------------------------------------------------------------------------------------------
def _nearest(C, a0, b0, k):
    order = sorted(range(C.n), key=lambda j: ((C.cells[j][0] - a0) ** 2 + (C.cells[j][1] - b0) ** 2, j))
    return order[:k]


def test_hand_built_clusters(dq, torch_mod):
    d, depth = 7, 7
    C = M.Component(d, 0)
    # two groups of 8 defects (4 nodes x 2 rounds) at opposite corners of the lattice and at distant rounds: two clusters of 8 under the cluster
    # rule (restated on the host when this case was built; a pair is also linked when its class-1 path beats the boundary paths of odd total class)
    two = np.zeros((depth, C.n), dtype=np.int64)
    for j in _nearest(C, 1, 1, 4):
        two[0, j] = two[1, j] = 1
    for j in _nearest(C, 6, 1, 4):
        two[3, j] = two[4, j] = 1
    # one tight cluster of 15 defects: the 15 plaquettes nearest the centre, one round
    tight = np.zeros((depth, C.n), dtype=np.int64)
    tight[1, _nearest(C, 3.5, 3.5, 15)] = 1                                     # (round 1: the future boundary, 6 rounds away, is never the nearer one)
    last = np.zeros((depth, C.n), dtype=np.int64)
    last[depth - 1, _nearest(C, 3.5, 3.5, 1)] = 1
    pair = np.zeros((depth, C.n), dtype=np.int64)
    pair[2, _nearest(C, 3.5, 3.5, 1)] = pair[3, _nearest(C, 3.5, 3.5, 1)] = 1
    C1 = M.Component(d, 1)
    last1 = np.zeros((depth, C1.n), dtype=np.int64)
    last1[depth - 1, _nearest(C1, 3.5, 3.5, 1)] = 1
    two1 = np.zeros((depth, C1.n), dtype=np.int64)                              # the two groups once more, in the other component
    for j in _nearest(C1, 3.5, 1, 4):
        two1[0, j] = two1[1, j] = 1
    for j in _nearest(C1, 6, 6, 4):
        two1[3, j] = two1[4, j] = 1
    vol = np.stack([_volumes_from_defects(d, depth, two), _volumes_from_defects(d, depth, tight), _volumes_from_defects(d, depth, last, last1),
                    _volumes_from_defects(d, depth, pair), _volumes_from_defects(d, depth, None, two1)])
    res = dq.decoder.matching_decode(vol, _env(dq, d, "DP", depth), to_host=True)
    assert np.array_equal(res.n_defects, _n_defects(d, vol))
    assert res.n_defects[0].tolist() == [16, 0] and res.n_defects[1].tolist() == [15, 0] and res.n_defects[4].tolist() == [0, 16]
    # 16 defects in clusters of at most 14: exact, the un-clustered DP's weight
    assert res.inexact.tolist() == [0, 1, 0, 0, 0]
    assert res.weight[0, 0] == M.dp_open(C, two, depth) and res.weight[4, 1] == M.dp_open(C1, two1, depth) and _certify_all(d, depth, vol, res, [0, 2, 3, 4]) == []
    # 15 defects in one cluster: the documented fallback -- the first 14 (in (t, node) order) exactly, the 15th to its nearest boundary (ties: class
    # 0).  The reported weight is that sum; the frame closes the volume (no future boundary is nearer here) and belongs to a history no heavier.
    ts, nodes = np.nonzero(tight)
    pd, pb = M._tables(C, nodes, ts, depth, True)
    w = list(M._subset_dp(pd[:14, :14], pb[:14]))
    cp = int(pb[14, 1] < pb[14, 0])
    want = min(w[cp], w[1 ^ cp]) + int(pb[14, cp])
    ok, w_min, hist = M.certify(d, 0, vol[1], res.frame[1], res.weight[1, 0], depth)
    assert res.weight[1, 0] == want and w_min <= hist <= want, (w_min, hist, want, res.weight[1])
    sig, _ = C.frame_syndrome_class(res.frame[1:2])
    assert np.array_equal(sig[0], C.syndromes(vol[1:2])[0, depth - 1])
    # a single last-round defect: the future boundary; a same-site pair in consecutive rounds: one measurement error
    assert res.weight[2].tolist() == [1, 1] and not res.frame[2].any()
    assert res.weight[3].tolist() == [1, 0] and not res.frame[3].any()


# ---- 5. invariance ---------------------------------------------------------------------------------------------------------------------------
def test_outputs_do_not_depend_on_batch_position_chunking_or_the_call(dq, torch_mod, d5_sample):
    env, vol, res = d5_sample
    D = dq.decoder
    n = len(vol)
    same = lambda a, b, sel=slice(None): all(np.array_equal(getattr(a, k), getattr(b, k)[sel]) for k in ("frame", "weight", "n_defects", "inexact"))
    perm = np.random.default_rng(5).permutation(n)
    assert same(D.matching_decode(vol[perm], env, chunk=n, to_host=True), res, perm)
    assert same(D.matching_decode(vol, env, chunk=7, to_host=True), res)                          # 586 launches, the last of one volume
    busy = np.argsort(-res.n_defects.sum(axis=1), kind="stable")[:48]                             # chunk 1 on the volumes with the most defects
    assert res.n_defects[busy].sum(axis=1).min() >= 8
    assert same(D.matching_decode(vol[busy], env, chunk=1, to_host=True), res, busy)
    # two calls on one handle, the second after a smaller one
    torch = torch_mod
    ev = D.Evaluator(5, "DP", False, 5, chunk=n, device=env.device)
    try:
        dev_vol = torch.from_numpy(vol).to(env.device)
        outs = []
        for m in (n, 33, n):
            frame = torch.zeros((n, 5, 5), dtype=torch.uint8, device=env.device)
            weight = torch.zeros((n, 2), dtype=torch.int32, device=env.device)
            ev.match_into(dev_vol, m, frame, weight, None, None)                 # (optional outputs may be left out)
            outs.append((frame.cpu().numpy(), weight.cpu().numpy()))
        assert np.array_equal(outs[0][0], res.frame) and np.array_equal(outs[2][0], res.frame) and np.array_equal(outs[2][1], res.weight)
        assert np.array_equal(outs[1][0][:33], res.frame[:33]) and not outs[1][0][33:].any()
    finally:
        ev.close()


# ---- 6. scoring ------------------------------------------------------------------------------------------------------------------------------
def test_score_matching_counts_and_the_agent_side_by_side(dq, torch_mod):
    from oracle import c_oracle
    D = dq.decoder
    n, p, base = 1 << 16, 0.007, 77
    weights, flat = shipped.shipped_weights("d5_x", "0.007")
    env = dq.VectorEnv(n_envs=1, p_phys=p, p_meas=p, seed=SEED, referee="lut", **shipped.CONFIGS["d5_x"])
    got = D.score_matching(env, n, env_id_base=base, chunk=20000, no_decoder=True)
    vol, hid, triv = D.sample_volumes(env, n, env_id_base=base, to_host=True)
    res = D.matching_decode(vol, env, to_host=True)
    lx, lz = c_oracle.luts(5)
    verd = V.verdict(5, hid, res.frame, V.classify_with(referee.LutReferee(5, "X", lx, lz)))
    want = D.counters_from_arrays(verd, triv, np.full(n, D.STATUS_IDENTITY), (res.frame.reshape(n, -1) != 0).sum(axis=1))
    assert [got.counters[k] for k in D.COUNTER_NAMES] == want
    assert got.inexact == int(res.inexact.sum()) and got.p_phys == p
    print(f"matching failure {got.failure_rate:.5f} {got.failure_interval}, no decoder {got.no_decoder.failure_rate:.5f} {got.no_decoder.failure_interval}")
    assert got.failure_interval[1] < got.no_decoder.failure_interval[0]
    # beside the agent: the same matching result, and the default call returns what it returns without a baseline
    model = dq.build_convolutional_nn(shipped.C_LAYERS, shipped.FF_LAYERS, env.observation_space.shape, env.num_actions)
    agent = dq.DQNAgent(model=model, nb_actions=env.num_actions, memory=dq.SequentialMemory(limit=1000, window_length=1), nb_steps_warmup=100,
                        target_model_update=100, policy=dq.GreedyQPolicy(masked_greedy=True), test_policy=dq.GreedyQPolicy(masked_greedy=True),
                        gamma=0.99, enable_dueling_network=True)
    agent.compile(dq.Adam(lr=1e-4))
    agent._bind(env)
    agent.model.set_weights(weights)
    try:
        plain = agent.decode_benchmark(env, n, env_id_base=base, chunk=20000)
        both = agent.decode_benchmark(env, n, env_id_base=base, chunk=20000, baseline="matching")
        assert isinstance(plain, D.EvalResult) and isinstance(both, tuple) and len(both) == 2
        assert both[0].counters == plain.counters and both[1].counters == got.counters and both[1].inexact == got.inexact
        assert both[0].counters["volumes"] == n and both[0].inexact == 0
        by_rate = agent.decode_benchmark(env, 4096, rates=[0.003, p], env_id_base=base, baseline="matching")
        alone = D.score_matching(env, 4096, rates=[0.003, p], env_id_base=base)
        assert set(by_rate[1]) == {0.003, p} and all(by_rate[1][r].counters == alone[r].counters for r in alone)
        assert alone[p].counters == D.score_matching(env, 4096, p_phys=p, env_id_base=base + 4096).counters
    finally:
        agent._decoder = None
