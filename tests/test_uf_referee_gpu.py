"""The union-find referee on the device (csrc/uf_plane_dev.h uf_plane_classify; include/deepq_hip.h dq_uf_referee_decode, dq_envb_set_referee,
dq_wide_uf_verdict_refereed_uf; VectorEnv(referee="uf"), referee.UnionFindReferee, verdict_wide / memory_experiment_wide(referee="uf"))
against the numpy rule of tests/uf_referee_ref.py.  Every comparison is bit for bit.  The sampled syndromes and their classes under the rule are computed once
per distance and shared."""
import functools
import importlib

import numpy as np
import pytest

import uf_referee_ref as U
import verdict_wide_ref as V

pytestmark = pytest.mark.gpu

SEED = (0x5EED, 0xD0DEC0DE)


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return torch


@pytest.fixture(scope="module")
def referee_mod():
    return importlib.import_module("deepq-decoding_amd.referee")


def same(got, want, what):
    bad = np.flatnonzero(np.asarray(got) != np.asarray(want))
    assert not len(bad), (what, len(bad), bad[:8].tolist(), np.asarray(got)[bad[:8]].tolist(), np.asarray(want)[bad[:8]].tolist())


# ---- 1. UnionFindReferee.decode against the rule -------------------------------------------------------------------------------------------------------------
SAMPLED = {7: 512, 9: 512, 13: 512, 15: 512}


@functools.lru_cache(maxsize=None)
def case(d):
    """(defects uint64 [N, 2, 2], the rule's classes uint8 [N], rows on which the matching referee is asked too: d <= 9) -- read-only.
    d = 3: all 2^4 x 2^4 syndromes of both components.  d = 5: all 4096 syndromes of component 0, then 256 sampled ones of both.  d = 7 .. 15: 512 syndromes
    of i.i.d. component errors, half at p = 0.03 and half at p = 0.10 (at d = 15 about 30 defects per component), then the all-ones syndrome and the
    empty one."""
    n = (d * d - 1) // 2
    if d == 3:
        k = np.arange(256, dtype=np.uint64)
        defects = np.zeros((256, 2, 2), dtype=np.uint64)
        defects[:, 0, 0], defects[:, 1, 0] = k & np.uint64(15), k >> np.uint64(4)
        ask = np.ones(256, dtype=bool)
    elif d == 5:
        defects = np.zeros((4096 + 256, 2, 2), dtype=np.uint64)
        defects[:4096, 0, 0] = np.arange(4096, dtype=np.uint64)
        defects[4096:] = U.sample_defects(5, 0.10, 256, 505)[0]
        ask = np.ones(len(defects), dtype=bool)
    else:
        half = SAMPLED[d] // 2
        ones = np.array([[(1 << min(n, 64)) - 1, (1 << max(n - 64, 0)) - 1]] * 2, dtype=np.uint64)
        defects = np.concatenate([U.sample_defects(d, 0.03, half, 100 * d + 3)[0], U.sample_defects(d, 0.10, half, 100 * d + 10)[0], ones[None],
                                  np.zeros((1, 2, 2), dtype=np.uint64)])
        # The matching referee is asked where it answers from LDS or a few pool walks: d <= 9.  At d >= 13 and p = 0.10 nearly every component holds a cluster
        # beyond 14 defects, each a walk of up to 2^20 subsets through one of eight locked slots, and at p = 0.03 alone both referees are simply right.
        ask = np.zeros(len(defects), dtype=bool)
        ask[:SAMPLED[d] if d <= 9 else 0] = True
    cls = U.classify_words(d, "DP", defects)
    for a in (defects, cls, ask):
        a.setflags(write=False)
    return defects, cls, ask


@pytest.mark.parametrize("d", [3, 5, 7, 9, 13, 15])
def test_decode_is_the_rule(dq, torch_mod, referee_mod, d):
    defects, want, ask = case(d)
    ref = referee_mod.UnionFindReferee(d, "DP")
    cls, flags = ref.decode(defects)
    got = cls.cpu().numpy()
    same(got, want, f"class, d = {d}")
    assert not flags.any().item() and ref.nodes == (d * d - 1) // 2
    same(ref.decode(defects, both=False)[0].cpu().numpy(), want & 1, "component 0 alone")
    same(referee_mod.UnionFindReferee(d, "X").decode(defects)[0].cpu().numpy(), want & 1, "the X model asks component 0 only")
    for i in (0, len(defects) // 2, len(defects) - 2):                                  # a batch of 1
        assert int(ref.decode(defects[i:i + 1])[0].cpu().numpy()[0]) == int(want[i])
    assert set(got.tolist()) == {0, 1, 2, 3}
    # pack / predict: MatchingReferee's protocol
    grids = U.grids_of(d, defects[:64])
    same(ref.pack(grids).reshape(-1), defects[:64].reshape(-1), "pack")
    same(np.argmax(ref.predict(grids.reshape(64, -1)), axis=1), want[:64], "predict")
    if 5 <= d <= 9:                                                                     # (at d = 3 the two referees agree on all but a handful of syndromes)
        match = referee_mod.MatchingReferee(d, "DP").decode(defects[ask])[0].cpu().numpy()
        differ = int((match != got[ask]).sum())
        print(f"d = {d}: the union-find referee differs from the matching referee on {differ} of {int(ask.sum())}")
        assert differ * 100 >= int(ask.sum())


def test_all_ones_at_full_width(dq, torch_mod, referee_mod):
    """n = 112: every node of both components a defect."""
    defects, want, _ = case(15)
    i = len(defects) - 2
    assert int(defects[i, 0, 0]) == 2 ** 64 - 1 and int(defects[i, 0, 1]) == 2 ** 48 - 1
    got = referee_mod.UnionFindReferee(15, "DP").decode(defects[i:i + 1])[0].cpu().numpy()
    assert int(got[0]) == int(want[i])


# ---- 2. the same classes from the closed stream decoder ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [5, 9, 15])
def test_class_of_the_closed_one_round_stream_decode(dq, torch_mod, d):
    defects, want, _ = case(d)
    grids = U.grids_of(d, defects)[:, None]                                            # [N, 1, d+1, d+1]
    r = dq.stream_decode_wide(grids, d, window=1, commit=1, final_round="perfect", to_host=True)
    same(U.frame_class(d, r.frame), want, f"class of the frame, d = {d}")


# ---- 3. / 4. the environment's step ---------------------------------------------------------------------------------------------------------------------------
ENV_CASES = {
    "d5wide": dict(d=5, error_model="DP", use_Y=False, volume_depth=5, p_phys=0.03, p_meas=0.03, backend="wide"),
    "d9dp": dict(d=9, error_model="DP", use_Y=False, volume_depth=5, p_phys=0.012, p_meas=0.012),
    "d15dpy": dict(d=15, error_model="DP", use_Y=True, volume_depth=3, p_phys=0.012, p_meas=0.012),
}
ENV_N, ENV_STEPS = 64, 24


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("name", list(ENV_CASES))
def test_step_under_both_referees(dq, torch_mod, name):
    kw = ENV_CASES[name]
    d = kw["d"]
    uf = dq.VectorEnv(n_envs=ENV_N, seed=SEED, referee="uf", **kw)
    mt = dq.VectorEnv(n_envs=ENV_N, seed=SEED, referee="matching", **kw)
    ev = dq.WideEvaluator(d, kw["error_model"], window=kw["volume_depth"], chunk=ENV_N, device=uf.device)
    try:
        assert uf.wide and mt.wide and uf.referee_kind == "uf" and mt.referee_kind == "matching"
        meta = 5 * ((d * d + 63) // 64) + 1 + 2 * uf.legal_words
        done_bit = np.uint64(1) << np.uint64(32)

        def records(env):
            st = _u64(env.export_state()).copy()
            done = (st[:, meta] & done_bit) != 0
            st[:, meta] &= ~done_bit
            return st, done

        same(uf.reset().cpu().numpy().reshape(-1), mt.reset().cpu().numpy().reshape(-1), "reset observation")
        differ = 0
        for t in range(ENV_STEPS):
            before, done_before = records(uf)
            same(before.reshape(-1), records(mt)[0].reshape(-1), ("state", t))
            a = uf.select_actions(t) if t % 3 == 2 else uf.uf_select_wide(ev)           # a uniformly legal action on every third step
            a = a.clone()
            uf.inexact.fill_(7)
            uf.step(a, auto_reset=False)
            mt.step(a, auto_reset=False)
            for what in ("obs", "reward", "legal", "lifetime", "was_reset"):
                same(getattr(uf, what).cpu().numpy().reshape(-1), getattr(mt, what).cpu().numpy().reshape(-1), (what, t))
            x, z = U.state_planes(before, d)
            reward, done = U.step_rule_batch(d, kw["error_model"], kw["use_Y"], x, z, a.cpu().numpy(), done_before)
            same(uf.reward.cpu().numpy(), reward, ("reward under the rule", t))
            same(uf.done.cpu().numpy(), done, ("done under the rule", t))
            same(records(uf)[1], done != 0, ("the record's done bit", t))
            assert not uf.inexact.any().item()
            differ += int((uf.done != mt.done).sum())
        ended = int(uf.done.sum())
        print(f"{name}: {ended} of {ENV_N} lattices ended under the union-find referee, {int(mt.done.sum())} under the matching referee; "
              f"{differ} lattice-steps with different done flags")
        assert ended >= 1
    finally:
        ev.close()
        uf.close()
        mt.close()


def test_the_referee_switches_back_and_forth(dq, torch_mod):
    """Two handles in lockstep on the same seed and actions, so their records agree in everything but the done bit; one of them changes its referee between
    steps.  Whenever it is back on matching, its step is the matching handle's from the same record: every output, the flags included, and done wherever the
    two records' done bits agreed in front of the step (done is sticky)."""
    kw = ENV_CASES["d9dp"]
    d = kw["d"]
    a_env = dq.VectorEnv(n_envs=ENV_N, seed=SEED, referee="uf", **kw)
    b_env = dq.VectorEnv(n_envs=ENV_N, seed=SEED, referee="matching", **kw)
    try:
        a_env.reset()
        b_env.reset()
        meta = 5 * ((d * d + 63) // 64) + 1 + 2 * a_env.legal_words
        done_bit = lambda e: (_u64(e.export_state())[:, meta] >> np.uint64(32)) & np.uint64(1)
        compared = 0
        for t in range(16):
            kind = ("matching", "uf", "uf", "matching")[t % 4]
            a_env.set_referee_kind(kind)
            assert a_env.referee_kind == kind
            agree = done_bit(a_env) == done_bit(b_env)
            act = b_env.select_actions(t).clone()
            a_env.inexact.fill_(7)
            a_env.step(act, auto_reset=False)
            b_env.step(act, auto_reset=False)
            for what in ("obs", "reward", "legal", "lifetime", "was_reset") + (("inexact",) if kind == "matching" else ()):
                same(getattr(a_env, what).cpu().numpy().reshape(-1), getattr(b_env, what).cpu().numpy().reshape(-1), (what, kind, t))
            if kind == "matching":
                same(a_env.done.cpu().numpy()[agree], b_env.done.cpu().numpy()[agree], ("done after switching back", t))
                compared += int(agree.sum())
            else:
                assert not a_env.inexact.any().item()
        assert compared >= ENV_N * 4
        with pytest.raises(ValueError):
            a_env.set_referee_kind("union_find")
        L = importlib.import_module("deepq-decoding_amd._lib")
        assert L.lib().dq_envb_set_referee(a_env._h, 2) == -1 and L.lib().dq_envb_set_referee(a_env._h, -1) == -1      # DQ_ERR_INVALID, the setting stays
        assert a_env.referee_kind == "matching"
    finally:
        a_env.close()
        b_env.close()


# ---- 5. the refereed verdict -----------------------------------------------------------------------------------------------------------------------------------
def test_verdict_of_every_x_pattern_of_d3(dq, torch_mod):
    hidden = V.exhaustive_d3("X")
    want = U.restatement(3, "X").verdict(hidden)["byte"]
    got, flags = dq.verdict_wide(hidden, None, 3, "X", referee="uf", chunk=len(hidden), to_host=True)
    same(got, want, "byte")
    assert not flags.any() and flags.shape == got.shape and min(V.kinds(got).values()) > 0


@pytest.mark.parametrize("d,model", V.SPARSE_CASES)
def test_verdict_of_sparse_and_cancelled_residuals(dq, torch_mod, d, model):
    hidden, frame = V.sparse_case(d, model)
    want = U.restatement(d, model).verdict(hidden, frame)["byte"]
    ev = dq.WideEvaluator(d, model, 1, chunk=64)                       # 257 volumes: four whole chunks and a last one of a single volume
    try:
        got, flags = dq.verdict_wide(hidden, frame, d, referee="uf", evaluator=ev, to_host=True)
        same(got, want, "byte")
        assert not flags.any()
        third = V.SPARSE_N // 3
        got, _ = dq.verdict_wide(hidden[:third], None, d, referee="uf", evaluator=ev, to_host=True)     # the frame's zeros as NULL
        same(got, want[:third], "byte, frame NULL")
        assert min(V.kinds(want).values()) > 0
    finally:
        ev.close()


def test_uncorrected_d15_volumes_in_one_launch(dq, torch_mod, monkeypatch):
    """4096 uncorrected d = 15 volumes: the case the matching referee has to slice goes in one launch, and the no_decoder counters are the bytes'."""
    DW = dq.decoder_wide
    n = 4096
    hidden = V.iid_hidden(15, n, 0.06, np.random.default_rng(1515))           # (verdict_wide_ref.FALLBACK_CASE's density: lists beyond 32, clusters beyond 20)
    want = U.restatement(15, "DP").verdict(hidden)["byte"]
    launches = []
    plain = DW.WideEvaluator.verdict_into
    monkeypatch.setattr(DW.WideEvaluator, "verdict_into", lambda self, h, f, m, out, **kw: (launches.append((m, kw.get("referee"))), plain(self, h, f, m, out, **kw))[1])
    got, flags = dq.verdict_wide(hidden, None, 15, "DP", referee="uf", to_host=True)
    assert launches == [(n, "uf")]
    same(got, want, "byte")
    assert not flags.any()
    k = V.kinds(want)
    assert k["dead"] >= 1 and k["alive_outside"] >= 1, k
    launches.clear()
    r, streams = dq.memory_experiment_wide((15, "DP"), 512, 5, p_phys=0.01, seed=SEED, env_id_base=9, no_decoder=True, referee="uf", return_streams=True)
    assert launches == [(512, "uf"), (512, "uf")]
    hid, frm = streams["hidden"].cpu().numpy(), streams["frame"].cpu().numpy()
    for row, frame in ((r, frm), (r.no_decoder, None)):
        b = U.restatement(15, "DP").verdict(hid, frame)["byte"]
        assert row.counters["volumes"] == 512 and row.inexact == 0
        assert row.counters["alive"] == int(((b & V.ALIVE) != 0).sum()) and row.counters["success"] == int(((b & V.SUCCESS) != 0).sum())
        assert row.counters["in_codespace"] == int(((b & V.IN_CODESPACE) != 0).sum())
    assert r.no_decoder.counters["alive"] < r.counters["alive"]


# ---- 6. episodes --------------------------------------------------------------------------------------------------------------------------------------------------
def test_union_find_outlives_the_identity_under_its_own_referee(dq, torch_mod):
    """An ordering, not a tolerance: d = 9 DP, volume_depth 5, p = 0.012, 64 lattices, one episode each, both policies on the same seed and ids, under the
    episode loop's hard cap."""
    cfg = dict(d=9, error_model="DP", use_Y=False, volume_depth=5, p_phys=0.012, p_meas=0.012)
    env = dq.VectorEnv(n_envs=64, seed=SEED, referee="uf", **cfg)
    try:
        uf = dq.WideUnionFindAgent()
        h_uf = uf.test(env, nb_episodes=64, verbose=0, nb_max_episode_steps=200000)
        ident = dq.WideUnionFindAgent(policy="identity")
        h_id = ident.test(env, nb_episodes=64, verbose=0, nb_max_episode_steps=200000)
        life_uf, life_id = (np.asarray(h.history["episode_lifetime"], dtype=np.float64) for h in (h_uf, h_id))
        assert env.referee_kind == "uf" and len(life_uf) == 64 and len(life_id) == 64 and uf.last_inexact_steps == 0
        print(f"mean lifetime under the union-find referee: union-find {life_uf.mean():.1f}, identity {life_id.mean():.1f}")
        assert life_uf.mean() > life_id.mean()
    finally:
        env.close()
