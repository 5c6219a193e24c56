"""The refereed verdict at d = 3 .. 15 on the device (decoder_wide.verdict_wide / memory_experiment_wide / DQNAgent.decode_benchmark_wide with
referee="matching"; csrc/verdict_wide.hip): bytes and inexact flags bit for bit against the numpy restatement
(tests/verdict_wide_ref.py) with no volume left out, against the narrow verdict on the look-up referee where both exist, against the shipped wide
environment's step, and the counters of the scoring paths.  The conditions that make the inputs meaningful are asserted on the restatement in
tests/test_verdict_wide_cpu.py."""
import ctypes

import numpy as np
import pytest

import decode_wide_ref as WR
import verdict_wide_ref as V

pytestmark = pytest.mark.gpu

SEED = (0xC0DE, 0x5EED)


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return torch


def same(got, want, what):
    bad = np.flatnonzero(np.asarray(got) != np.asarray(want))
    assert not len(bad), (what, len(bad), bad[:8].tolist(), np.asarray(got)[bad[:8]].tolist(), np.asarray(want)[bad[:8]].tolist())


# ---- 5. exhaustive d = 3 -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["DP", "X"])
def test_every_hidden_state_of_d3(dq, torch_mod, model):
    hidden = V.exhaustive_d3(model)
    want = V.restatement(3, model).verdict(hidden)
    got, flags = dq.verdict_wide(hidden, None, 3, model, referee="matching", chunk=len(hidden), to_host=True)      # one call
    same(got, want["byte"], "byte")
    same(flags, want["inexact"], "inexact")
    assert not flags.any() and min(V.kinds(got).values()) > 0


# ---- 6. sparse and cancelled residuals -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,model", V.SPARSE_CASES)
def test_sparse_and_cancelled_residuals(dq, torch_mod, d, model):
    hidden, frame = V.sparse_case(d, model)
    want = V.sparse_expected(d, model)
    ev = dq.WideEvaluator(d, model, 1, chunk=64)                       # 257 volumes: four whole chunks and a last one of a single volume
    try:
        got, flags = dq.verdict_wide(hidden, frame, d, referee="matching", evaluator=ev, to_host=True)
        same(got, want["byte"], "byte")
        same(flags, want["inexact"], "inexact")
        third = V.SPARSE_N // 3
        got, flags = dq.verdict_wide(hidden[:third], None, d, referee="matching", evaluator=ev, to_host=True)     # the frame's zeros as NULL
        same(got, want["byte"][:third], "byte, frame NULL")
        same(flags, want["inexact"][:third], "inexact, frame NULL")
        k = 2 * third + 1
        got, flags = dq.verdict_wide(hidden[k:k + 1], frame[k:k + 1], d, referee="matching", evaluator=ev, to_host=True)      # n = 1
        assert (int(got[0]), int(flags[0])) == (int(want["byte"][k]), int(want["inexact"][k]))
        # the unrefereed launch on the same handle is what it was: alive := success, decoded 0, every other field the refereed byte's
        plain = dq.verdict_wide(hidden, frame, d, evaluator=ev, to_host=True)
        keep = V.IN_CODESPACE | (3 << V.CLASS_SHIFT) | V.SUCCESS
        same(plain & keep, want["byte"] & keep, "unrefereed fields")
        same((plain & V.ALIVE) != 0, (plain & V.SUCCESS) != 0, "unrefereed alive")
        assert not (plain >> V.DECODED_SHIFT).any()
    finally:
        ev.close()


# ---- 7. / 8. the scratch pool and the fallbacks ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pool", "fallback"])
def test_dense_residuals(dq, torch_mod, name):
    c = dict(pool=V.POOL_CASE, fallback=V.FALLBACK_CASE)[name]
    hidden, want = V.dense_case(name)
    got, flags = dq.verdict_wide(hidden, None, c["d"], c["error_model"], referee="matching", to_host=True)
    same(got, want["byte"], "byte")
    same(flags, want["inexact"], "inexact")                            # the device's flag is `flags != 0` of the C oracle
    assert set(np.unique(flags)) <= {0, 1}


def test_uncorrected_volumes_go_in_slices_with_the_same_bytes(dq, torch_mod, monkeypatch):
    """At d >= 13 the refereed verdict of uncorrected volumes is launched in slices (decoder_wide.refereed_uncorrected_into): here of 100 of 257."""
    DW = dq.decoder_wide
    hidden, _ = V.sparse_case(13, "DP")
    want = V.restatement(13, "DP").verdict(hidden)
    launches = []
    plain = DW.WideEvaluator.verdict_into
    monkeypatch.setattr(DW.WideEvaluator, "verdict_into", lambda self, h, f, m, out, **kw: (launches.append(m), plain(self, h, f, m, out, **kw))[1])
    monkeypatch.setattr(DW, "UNCORRECTED_REFEREE_SLICE", 100)
    got, flags = dq.verdict_wide(hidden, None, 13, "DP", referee="matching", to_host=True)
    assert launches == [100, 100, 57]
    same(got, want["byte"], "byte")
    same(flags, want["inexact"], "inexact")
    launches.clear()
    r = dq.memory_experiment_wide((13, "DP"), 257, 6, p_phys=0.01, seed=SEED, no_decoder=True, referee="matching")
    assert launches == [257, 100, 100, 57] and r.no_decoder.counters["volumes"] == 257


# ---- 9. the narrow verdict on the minimum-weight look-up referee -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,model", V.NARROW_CASES)
def test_equals_the_narrow_verdict_where_both_exist(dq, torch_mod, d, model):
    hidden, frame = V.sparse_case(d, model)
    env = dq.VectorEnv(n_envs=1, d=d, error_model=model, use_Y=False, volume_depth=3, p_phys=0.01, p_meas=0.01, seed=SEED, referee="lut")
    try:
        narrow, _ = dq.decoder.verdict(hidden, frame, env, to_host=True)
        narrow0, _ = dq.decoder.verdict(hidden, None, env, to_host=True)
    finally:
        env.close()
    got, flags = dq.verdict_wide(hidden, frame, d, model, referee="matching", to_host=True)
    got0, _ = dq.verdict_wide(hidden, None, d, model, referee="matching", to_host=True)
    same(got, narrow, "byte")
    same(got0, narrow0, "byte, frame NULL")
    assert not flags.any() and min(V.kinds(got).values()) >= 1


# ---- 10. the shipped wide environment's step -----------------------------------------------------------------------------------------------------------------
# (the rates: high enough that at least 5 of the 256 episodes end, low enough that a few dozen volumes at most walk a fallback cluster's 2^20 subsets)
@pytest.mark.parametrize("d,model,p", [(9, "DP", 0.06), (9, "X", 0.08), (13, "DP", 0.025), (13, "X", 0.02), (15, "DP", 0.02), (15, "X", 0.015)])
def test_equals_the_wide_environments_step(dq, torch_mod, d, model, p):
    n, W = 256, (d * d + 63) // 64
    env = dq.VectorEnv(n_envs=n, d=d, error_model=model, use_Y=False, volume_depth=3, p_phys=p, p_meas=p, seed=SEED, env_id_base=d * 1000)
    try:
        assert env.wide
        env.reset(write_obs=False)
        st = env.export_state().cpu().numpy().view(np.uint64)            # x[W] z[W] ... (include/deepq_hip.h dq_envb_export_state)
        bit = lambda words: ((words[:, np.arange(d * d) >> 6] >> (np.arange(d * d) & 63).astype(np.uint64)) & np.uint64(1)).astype(bool)
        hidden = V.codes(bit(st[:, :W]), bit(st[:, W:2 * W])).reshape(n, d, d)
        action = torch_mod.full((n,), int(env.identity_index), dtype=torch_mod.int32, device=env.device)
        env.step(action, auto_reset=False, write_obs=False)
        reward, done, inexact = env.reward.cpu().numpy(), env.done.cpu().numpy(), env.inexact.cpu().numpy()
    finally:
        env.close()
    got, flags = dq.verdict_wide(hidden, None, d, model, referee="matching", to_host=True)
    same((got & V.SUCCESS) != 0, reward == 1, "success")
    same((got & V.ALIVE) != 0, done == 0, "alive")
    same(flags, inexact, "inexact")
    assert (done != 0).sum() >= 5 and (done == 0).sum() >= 5, (int(done.sum()), n)


# ---- 11. memory_experiment_wide ---------------------------------------------------------------------------------------------------------------------------------
def _counts(d, model, hidden, frame):
    want = V.restatement(d, model).verdict(hidden.cpu().numpy(), None if frame is None else frame.cpu().numpy())
    return int(((want["byte"] & V.ALIVE) != 0).sum()), int(want["inexact"].sum()), int(((want["byte"] & V.SUCCESS) != 0).sum())


@pytest.mark.parametrize("d", [9, 13])
def test_memory_experiment_wide_refereed(dq, torch_mod, d):
    kw = dict(rounds=6, p_phys=0.01, seed=SEED, env_id_base=77, no_decoder=True)
    ev = dq.WideEvaluator(d, "DP", None, chunk=200)                    # 512 streams: chunks of 200, 200, 112
    try:
        plain = dq.memory_experiment_wide((d, "DP"), 512, evaluator=ev, **kw)
        ref, streams = dq.memory_experiment_wide((d, "DP"), 512, evaluator=ev, referee="matching", return_streams=True, **kw)
        for row, row0, frame in ((ref, plain, streams["frame"]), (ref.no_decoder, plain.no_decoder, None)):
            for name in row.counters:
                if name != "alive":
                    assert row.counters[name] == row0.counters[name], name
            alive, inexact, success = _counts(d, "DP", streams["hidden"], frame)
            assert row.counters["alive"] >= row.counters["success"] == success
            assert (row.counters["alive"], row.inexact) == (alive, inexact)
            assert row0.counters["alive"] == row0.counters["success"] and row0.inexact == 0
        assert ref.counters["alive"] > ref.counters["success"]          # a faulty last round leaves residuals outside the code space that the referee completes
        closed = dq.memory_experiment_wide((d, "DP"), 512, evaluator=ev, referee="matching", final_round="perfect", **kw)
        assert closed.counters["in_codespace"] == 512 and closed.counters["alive"] == closed.counters["success"] and closed.inexact == 0
        assert closed.no_decoder.counters["alive"] >= closed.no_decoder.counters["success"]      # (no correction: the residual is the error, outside the code space)
        a, b = 0.006, 0.014                                             # (no_decoder stays out of this leg: uncorrected errors at the higher rate walk the scratch pool)
        rates = dict(rounds=6, seed=SEED)
        both = dq.memory_experiment_wide((d, "DP"), 512, evaluator=ev, referee="matching", rates=[a, b], env_id_base=77, **rates)
        for k, rate in enumerate((a, b)):
            one = dq.memory_experiment_wide((d, "DP"), 512, evaluator=ev, referee="matching", p_phys=rate, env_id_base=77 + 512 * k, **rates)
            assert both[rate].counters == one.counters and both[rate].inexact == one.inexact, rate
        assert both[b].counters["success"] < both[a].counters["success"] and both[b].counters["alive"] > both[b].counters["success"]      # (the rates tell)
    finally:
        ev.close()


# ---- 12. decode_benchmark_wide ------------------------------------------------------------------------------------------------------------------------------------
SCORE_CFG = dict(d=9, error_model="DP", use_Y=False, volume_depth=5)
SCORE_N, SCORE_P, SCORE_BASE = 512, 0.01, 4096


@pytest.fixture(scope="module")
def score_agent(dq, torch_mod):
    grids_env = dq.VectorEnv(n_envs=150, p_phys=0.03, p_meas=0.03, seed=(2, 3), **SCORE_CFG)
    try:
        grids_env.reset()
        grids = np.ascontiguousarray(grids_env.obs.cpu().numpy()[:, :SCORE_CFG["volume_depth"], ::2, ::2])
    finally:
        grids_env.close()
    spec, flat = WR.sensitive_network(SCORE_CFG, grids)
    env = dq.VectorEnv(n_envs=2, p_phys=SCORE_P, p_meas=SCORE_P, seed=(5, 6), **SCORE_CFG)
    model = dq.build_convolutional_nn(WR.C_LAYERS, WR.FF_LAYERS, env.obs_shape, env.num_actions)
    agent = dq.DQNAgent(model=model, nb_actions=env.num_actions, memory=dq.SequentialMemory(limit=64, window_length=1), nb_steps_warmup=100,
                        target_model_update=100, policy=dq.GreedyQPolicy(masked_greedy=True), test_policy=dq.GreedyQPolicy(masked_greedy=True),
                        gamma=0.99, enable_dueling_network=True)
    agent.compile(dq.Adam(lr=1e-4))
    agent._bind(env)
    agent.model.set_weights(WR.weights_of(spec, flat))
    yield agent, env, spec, flat
    for name in ("_wide_decoder", "_decoder"):
        dec = getattr(agent, name, None)
        if dec is not None:
            dec.close()
        setattr(agent, name, None)
    env.close()


def test_decode_benchmark_wide_refereed(dq, score_agent):
    agent, env, spec, flat = score_agent
    kw = dict(seed=SEED, env_id_base=SCORE_BASE, no_decoder=True)
    mine, uf = agent.decode_benchmark_wide(env, SCORE_N, baseline="union_find", referee="matching", **kw)
    want = dq.memory_experiment_wide((9, "DP"), SCORE_N, rounds=5, window=5, commit=5, p_phys=SCORE_P, referee="matching", **kw)
    assert uf.counters == want.counters and uf.inexact == want.inexact
    assert uf.no_decoder.counters == want.no_decoder.counters and uf.no_decoder.inexact == want.no_decoder.inexact
    assert mine.no_decoder.counters == want.no_decoder.counters and mine.no_decoder.inexact == want.no_decoder.inexact
    assert uf.counters["alive"] > uf.counters["success"] and mine.counters["alive"] >= mine.counters["success"]
    plain, uf0 = agent.decode_benchmark_wide(env, SCORE_N, baseline="union_find", **kw)
    for got, old in ((mine, plain), (uf, uf0), (mine.no_decoder, plain.no_decoder)):
        assert {k: v for k, v in got.counters.items() if k != "alive"} == {k: v for k, v in old.counters.items() if k != "alive"}
        assert old.counters["alive"] == old.counters["success"] and old.inexact == 0
    lazy = flat.copy()
    lazy[-1] += 1e4                                                 # the identity's advantage above every other Q
    agent.model.set_weights(WR.weights_of(spec, lazy))
    try:
        r = agent.decode_benchmark_wide(env, SCORE_N, referee="matching", **kw)
    finally:
        agent.model.set_weights(WR.weights_of(spec, flat))
    assert r.counters["identity"] == SCORE_N and r.counters["corrections"] == 0
    for name in ("volumes", "trivial", "in_codespace", "success", "alive", "corrections"):
        assert r.counters[name] == r.no_decoder.counters[name], name
    assert r.inexact == r.no_decoder.inexact and r.counters["alive"] > r.counters["success"]


# ---- 13. refused arguments ---------------------------------------------------------------------------------------------------------------------------------------
def test_refused_arguments_leave_the_handle_usable(dq, torch_mod):
    torch = torch_mod
    L = dq.lib()
    hidden, frame = V.sparse_case(9, "DP")
    want = V.sparse_expected(9, "DP")
    ev = dq.WideEvaluator(9, "DP", 1, chunk=8)
    other = ctypes.c_void_p()
    assert L.dq_match_create(11, ctypes.byref(other)) == 0
    try:
        m = ev._referee()
        h, f = torch.from_numpy(hidden[:8].copy()).cuda(), torch.from_numpy(frame[:8].copy()).cuda()
        out, flags = torch.full((8,), 255, dtype=torch.uint8, device="cuda"), torch.full((8,), 255, dtype=torch.uint8, device="cuda")
        stream = ev._stream()
        call = lambda handle, ref, n: L.dq_wide_uf_verdict_refereed(handle, ref, h.data_ptr(), f.data_ptr(), n, out.data_ptr(), flags.data_ptr(), stream)
        for handle, ref, n in ((ev._h, None, 8), (ev._h, other, 8), (ev._h, m, 0), (ev._h, m, -1), (ev._h, m, 9), (None, m, 8)):
            assert call(handle, ref, n) == -1, (ref, n)                 # DQ_ERR_INVALID
            assert b"dq_wide_uf_verdict_refereed" in L.dq_last_error()
        assert L.dq_wide_uf_verdict_refereed(ev._h, m, None, None, 8, out.data_ptr(), None, stream) == -1
        torch.cuda.synchronize()
        assert bool((out == 255).all()) and bool((flags == 255).all())          # nothing was launched
        assert call(ev._h, m, 8) == 0                                           # the handle serves the next call
        torch.cuda.synchronize()
        same(out.cpu().numpy(), want["byte"][:8], "byte")
        same(flags.cpu().numpy(), want["inexact"][:8], "inexact")
    finally:
        L.dq_match_destroy(other)
        ev.close()
