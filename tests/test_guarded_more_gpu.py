"""The entry points DESIGN.md section 30 listed as not covered, between guard bands (tests/guarded.py; the rule and the helpers are
tests/test_guarded_gpu.py's, unchanged): the small ones, the sampled runs, the teachers of both environments, the wide agent decode and the update
that carries the environment step.  Every case chooses its inputs on the CPU, asserts there that the branches it exists for occur, and then shows per
fill (a) every guard intact, (b) every pure input unchanged, (c) every output and every in/out buffer bit-identical between the fills, (d) the outputs
equal to the family's reference and every in/out buffer equal to it IN FULL -- the slots of a ring a call must leave alone included."""
import ctypes
import functools
import importlib

import numpy as np
import pytest

import guarded as G
import test_guarded_gpu as T
import test_qnet_gpu as TQ
from oracle import dqn_oracle as O
from test_guarded_gpu import ENV_SEED, _mod, arr, both_fills, untouched

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def host_rates(torch, fill, ph, pm):
    """The two HOST arrays of per-stream rates (double, 8-byte aligned and nothing coarser) between guards of their own; returns (arena, ph view, pm view)."""
    h = G.Arena("cpu", fill)
    h.request("p_phys", ph.shape, torch.float64, 8, init=ph)
    h.request("p_meas", pm.shape, torch.float64, 8, init=pm)
    return h, h.take("p_phys").numpy(), h.take("p_meas").numpy()


def u64(raw, shape=(-1,)):
    return arr(raw, np.uint64, shape)


# ---- the small ones ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [5, 33])
def test_replay_sample_multi(dq, torch_mod, batch):
    """dq_replay_sample_multi: index_dev int32 [3][batch] on a full ring of 9 slots x 5 lattices (exactly n_slots * n_envs flag bytes) whose candidate
    slots wrap below slot 0; row u = oracle/memory_oracle.py's rows of update t0 + u.  batch 5 draws without replacement, 33 > 30 candidates with."""
    torch = torch_mod
    Q = _mod("qnet")
    from oracle import memory_oracle as M
    rng = np.random.RandomState(4)
    n_envs, n_slots, head, filled, U = 5, 9, 3, 9, 3
    term = (rng.rand(n_slots, n_envs) < 0.15).astype(np.uint8)
    seed, t0, base = (8, 9), 55, 1000
    want = np.stack([M.device_replay_rows(term, n_envs, n_slots, head, filled, batch, seed, t0 + u, sample_base=base) for u in range(U)])
    assert term.any() and len({tuple(r) for r in want}) == U and (want // n_envs).max() > head       # a redraw can occur; the rows differ; the slots wrap

    def run(a):
        a.request("term", term.shape, torch.uint8, 1, init=term)
        a.request("index", (U, batch), torch.int32, 4)
        Q.replay_sample_multi(a.take("term"), n_envs, n_slots, head, filled, batch, seed, t0, U, sample_base=base, out=a.take("index"))

    out, _ = both_fills(run)
    assert np.array_equal(arr(out["index"], np.int32, (U, batch)), want)


def _bookkeeping_case(n, steps=12):
    """Inputs of `steps` vector steps of n lattices and the serial restatement of dq_test_bookkeeping on them: (done, was_reset, reward, lifetime [steps][n],
    quota [n]) and (records in append order per step, quota, ep_reward, ep_len after the last step)."""
    rng = np.random.RandomState(100 + n)
    done = (rng.rand(steps, n) < 0.3).astype(np.uint8)
    was_reset = np.zeros((steps, n), np.uint8)
    was_reset[1:] = done[:-1]                                       # auto-reset: the step after a done is spent on the reset ...
    done[was_reset != 0] = 0                                        # ... and ends nothing
    done[steps - 1, n - 1], was_reset[steps - 1, n - 1] = 1, 0       # the last lattice ends an episode in the last step
    done[steps - 2, n - 1] = 0
    done[steps - 1, :n - 1] = 0                                     # ... and it alone: which record a table one row short loses is then known
    reward = (rng.rand(steps, n) < 0.5).astype(np.float32)
    lifetime = rng.randint(1, 1000, size=(steps, n)).astype(np.int32)
    quota = rng.randint(0, 3, size=n).astype(np.int32)
    quota[n - 1] = steps                                            # it still owes episodes then
    q, r, ln, recs, unpaid = quota.copy(), np.zeros(n, np.float32), np.zeros(n, np.int32), [], 0
    for k in range(steps):
        for i in range(n):
            wr = was_reset[k, i] != 0
            if not wr:
                r[i] = np.float32(r[i] + reward[k, i])
                ln[i] += 1
            if done[k, i] and not wr:
                if q[i] > 0:
                    q[i] -= 1
                    recs.append((k, i, int(r[i:i + 1].view(np.int32)[0]), int(ln[i]), int(lifetime[k, i])))
                else:
                    unpaid += 1
                r[i], ln[i] = 0.0, 0
    return (done, was_reset, reward, lifetime, quota), (np.array(recs, dtype=np.int32).reshape(-1, 5), q, r, ln, unpaid)


@pytest.mark.parametrize("short", [0, 1], ids=["exact", "one-row-short"])
@pytest.mark.parametrize("n", [5, 33])
def test_test_bookkeeping(dq, torch_mod, n, short):
    """dq_test_bookkeeping over 12 vector steps: records_dev has exactly as many rows as the restatement appends (the last append, made in the last step,
    touches the guard), and once one row fewer: the header's rule for a full table -- the record is dropped, its quota is paid, counter_dev[0] counts it --
    without a store past the table.  quota, the running reward and length, and the counter are in/out and compared in full."""
    torch = torch_mod
    lib = _mod("_lib")
    (done, was_reset, reward, lifetime, quota), (recs, q_ref, r_ref, l_ref, unpaid) = _bookkeeping_case(n)
    steps, total = len(done), len(recs)
    assert total >= 3 and unpaid >= 1 and was_reset.any() and recs[-1][0] == steps - 1 and (recs[:, 0] < steps - 1).sum() == total - 1
    cap = total - short
    L, P = lib.lib(), lib.ptr

    def run(a):
        a.request("done", done.shape, torch.uint8, 1, init=done)
        a.request("was_reset", done.shape, torch.uint8, 1, init=was_reset)
        a.request("reward", done.shape, torch.float32, 4, init=reward)
        a.request("lifetime", done.shape, torch.int32, 4, init=lifetime)
        a.request("quota", (n,), torch.int32, 4, init=quota, inout=True)
        a.request("ep_reward", (n,), torch.float32, 4, init=np.zeros(n, np.float32), inout=True)
        a.request("ep_len", (n,), torch.int32, 4, init=np.zeros(n, np.int32), inout=True)
        a.request("records", (cap, 5), torch.int32, 4)
        a.request("counter", (1,), torch.int32, 4, init=np.zeros(1, np.int32), inout=True)
        k = a.take
        for s in range(steps):
            lib.check(L.dq_test_bookkeeping(P(k("done")[s]), P(k("was_reset")[s]), P(k("reward")[s]), P(k("lifetime")[s]), n, s, P(k("quota")),
                                            P(k("ep_reward")), P(k("ep_len")), P(k("records")), cap, P(k("counter")), lib.current_stream()))

    out, _ = both_fills(run)
    assert arr(out["counter"], np.int32).tolist() == [total]          # (beyond the capacity too: that is how the host sees that records were lost)
    assert np.array_equal(arr(out["quota"], np.int32), q_ref) and np.array_equal(arr(out["ep_len"], np.int32), l_ref)
    assert np.array_equal(out["ep_reward"], r_ref.view(np.uint8))
    got = arr(out["records"], np.int32, (cap, 5))
    order = lambda x: x[np.lexsort((x[:, 1], x[:, 0]))]
    assert np.array_equal(order(got), order(recs[:cap]))            # (one record in the last step: the dropped one is the last)


def _state_words(st, ref):
    rs = ref.export()
    assert np.array_equal(st[:, 0], rs["xmask"]) and np.array_equal(st[:, 1], rs["zmask"])
    assert np.array_equal(st[:, 2], rs["true_word"]) and np.array_equal(st[:, 3], rs["summed"])
    assert np.array_equal(st[:, 5], rs["round"]) and np.array_equal(st[:, 11:], rs["volume"])
    assert np.array_equal(st[:, 6:8], rs["completed"]) and np.array_equal(st[:, 8:10], ref.legal)
    assert np.array_equal(st[:, 10], ref.lifetime.astype(np.uint64) | (ref.done.astype(np.uint64) << np.uint64(32)))


@pytest.mark.parametrize("n", [5, 33])
@pytest.mark.parametrize("name", ["d3dp", "c3", "c5"])
def test_narrow_export_and_import_state(dq, torch_mod, name, n):
    """dq_env_export_state into exactly [n][state_words] words (8-byte aligned), dq_env_import_state from such a buffer into a twin: the export of the
    imported state reproduces it, and the twin stepped from it gives the bits of the original and of the C oracle."""
    from oracle import c_oracle
    torch = torch_mod
    lib = _mod("_lib")
    cfg, base = T.NARROW[name], 4096 * 3
    L, P = lib.lib(), lib.ptr

    def run(a):
        env = dq.VectorEnv(n_envs=n, seed=ENV_SEED, env_id_base=base, **cfg)
        twin = dq.VectorEnv(n_envs=n, seed=ENV_SEED, env_id_base=base, **cfg)
        ref = c_oracle.COracleEnv(n_envs=n, seed=ENV_SEED, env_id_base=base, **cfg)
        sw = env.state_words
        a.request("state", (n, sw), torch.int64, 8)
        a.request("state_in", (n, sw), torch.int64, 8, init=np.zeros((n, sw), np.int64), inout=True)      # (written by a device copy, read by the import)
        a.request("state_twin", (n, sw), torch.int64, 8)
        k, st = a.take, lib.current_stream()
        env.reset(); twin.reset(); ref.reset()
        for t in range(4):
            act = ref.policy_uniform_legal(t)
            env.step(torch.from_numpy(act).cuda(), auto_reset=True)
            ref.step(act, auto_reset=True)
        lib.check(L.dq_env_export_state(env._h, P(k("state")), st))
        _state_words(k("state").cpu().numpy().view(np.uint64), ref)
        k("state_in").copy_(k("state"))
        lib.check(L.dq_env_import_state(twin._h, P(k("state_in")), st))
        lib.check(L.dq_env_export_state(twin._h, P(k("state_twin")), st))
        for t in range(4, 8):                                       # (the done flag an auto-reset reads is the record's: it travels with the state)
            act = ref.policy_uniform_legal(t)
            ref.step(act, auto_reset=True)
            for e in (env, twin):
                e.step(torch.from_numpy(act).cuda(), auto_reset=True)
                assert np.array_equal(e.obs.cpu().numpy(), ref.obs) and np.array_equal(e.reward.cpu().numpy(), ref.reward), (name, t)
                assert np.array_equal(e.done.cpu().numpy(), ref.done) and np.array_equal(e.legal.cpu().numpy().view(np.uint64), ref.legal), (name, t)
                assert np.array_equal(e.was_reset.cpu().numpy(), ref.was_reset), (name, t)
        assert torch.equal(env.export_state(), twin.export_state())
        torch.cuda.synchronize()
        env.close(); twin.close()

    out, _ = both_fills(run)
    assert np.array_equal(out["state_in"], out["state"]) and np.array_equal(out["state_twin"], out["state"])


@pytest.mark.parametrize("name", list(T.WIDE))
def test_wide_export_state(dq, torch_mod, name):
    """dq_envb_export_state into exactly [n][state_words] words after the 6 oracle steps of the wide cases: the wide C oracle's exported state."""
    import test_env_wide_gpu as TW
    from oracle import c_oracle
    torch = torch_mod
    lib = _mod("_lib")
    cfg, p, base = T.WIDE[name]
    n = 5

    def run(a):
        env = dq.VectorEnv(n_envs=n, seed=TW.SEED, env_id_base=base, backend="wide", p_phys=p, p_meas=p, **cfg)
        ref = c_oracle.COracleWideEnv(n_envs=n, seed=TW.SEED, env_id_base=base, p_phys=p, p_meas=p, **cfg)
        a.request("state", (n, env.state_words), torch.int64, 8)
        env.reset(); ref.reset()
        for t in range(6):
            act = ref.policy_uniform_legal(t)
            env.step(torch.from_numpy(act).cuda(), auto_reset=True)
            ref.step(act, auto_reset=True)
        lib.check(lib.lib().dq_envb_export_state(env._h, lib.ptr(a.take("state")), lib.current_stream()))
        want = ref.export_state()
        torch.cuda.synchronize()
        env.close()
        return want

    out, want = both_fills(run)
    assert np.array_equal(u64(out["state"], want.shape), want)


def _pack_bits(table):
    bits = np.packbits(np.asarray(table, dtype=np.uint8), bitorder="little")
    return np.concatenate([bits, np.zeros((-len(bits)) % 4, np.uint8)]).view(np.int32).copy()


@pytest.mark.parametrize("d", [3, 5])
def test_caller_owned_referee_tables(dq, torch_mod, d):
    """dq_env_set_referee with tables of exactly ceil(2^((d*d-1)/2) / 32) words -- ONE word at d = 3, where a table is 16 bits behind a uint32_t pointer --
    holding the built-in minimum-weight referee: 40 steps of 33 lattices at p = 0.03 equal the C oracle run with the same tables, terminations included."""
    from oracle import c_oracle
    torch = torch_mod
    lib = _mod("_lib")
    cfg = dict(d=d, error_model="DP", use_Y=False, volume_depth=d, p_phys=0.03, p_meas=0.03)
    n, base = 33, 7
    lx, lz = c_oracle.luts(d)
    wx, wz = _pack_bits(lx), _pack_bits(lz)
    assert len(wx) == -(-(1 << ((d * d - 1) // 2)) // 32) and lx.any() and lz.any()
    ended = []

    def run(a):
        env = dq.VectorEnv(n_envs=n, seed=ENV_SEED, env_id_base=base, referee=None, **cfg)
        ref = c_oracle.COracleEnv(n_envs=n, seed=ENV_SEED, env_id_base=base, lut=(lx, lz), **cfg)
        a.request("lut_x", wx.shape, torch.int32, 4, init=wx)
        a.request("lut_z", wz.shape, torch.int32, 4, init=wz)
        lib.check(lib.lib().dq_env_set_referee(env._h, lib.ptr(a.take("lut_x")), lib.ptr(a.take("lut_z"))))
        env.reset(); ref.reset()
        count = 0
        for t in range(40):
            act = ref.policy_uniform_legal(t)
            env.step(torch.from_numpy(act).cuda(), auto_reset=True)
            ref.step(act, auto_reset=True)
            assert np.array_equal(env.obs.cpu().numpy(), ref.obs) and np.array_equal(env.reward.cpu().numpy(), ref.reward), t
            assert np.array_equal(env.done.cpu().numpy(), ref.done) and np.array_equal(env.was_reset.cpu().numpy(), ref.was_reset), t
            count += int(ref.done.sum())
        ended.append(count)
        torch.cuda.synchronize()
        env.close()

    both_fills(run)
    assert ended[0] >= 1, ended


def test_caller_owned_joint_referee_table(dq, torch_mod):
    """dq_env_set_referee_joint at d = 3: 2^8 entries of 2 bits = exactly 16 words, tabulated on the host from the built-in component tables
    (VectorEnv.set_referee_predict's packing): the C oracle's trajectory with those tables."""
    from oracle import c_oracle, referee as oref
    torch = torch_mod
    lib = _mod("_lib")
    d, n, base = 3, 33, 7
    cfg = dict(d=d, error_model="DP", use_Y=False, volume_depth=d, p_phys=0.03, p_meas=0.03)
    lx, lz = c_oracle.luts(d)
    host = dq.VectorEnv(n_envs=1, referee=oref.LutReferee(d, "DP", lx, lz), **cfg)       # (tabulates the predictor once; its table is the case's input)
    words = host._lut[0].cpu().numpy().copy()
    host.close()
    assert words.shape == (16,) and words.any()
    ended = []

    def run(a):
        env = dq.VectorEnv(n_envs=n, seed=ENV_SEED, env_id_base=base, referee=None, **cfg)
        ref = c_oracle.COracleEnv(n_envs=n, seed=ENV_SEED, env_id_base=base, lut=(lx, lz), **cfg)
        a.request("lut", words.shape, torch.int32, 4, init=words)
        lib.check(lib.lib().dq_env_set_referee_joint(env._h, lib.ptr(a.take("lut"))))
        env.reset(); ref.reset()
        count = 0
        for t in range(40):
            act = ref.policy_uniform_legal(t)
            env.step(torch.from_numpy(act).cuda(), auto_reset=True)
            ref.step(act, auto_reset=True)
            assert np.array_equal(env.obs.cpu().numpy(), ref.obs) and np.array_equal(env.reward.cpu().numpy(), ref.reward), t
            assert np.array_equal(env.done.cpu().numpy(), ref.done) and np.array_equal(env.was_reset.cpu().numpy(), ref.was_reset), t
            count += int(ref.done.sum())
        ended.append(count)
        torch.cuda.synchronize()
        env.close()

    both_fills(run)
    assert ended[0] >= 1, ended


@pytest.mark.parametrize("n", [5, 33])
def test_referee_classes(dq, torch_mod, n):
    """dq_env_referee_classes of a Dense-stack referee at d = 7: actions int32 [n] in, classes uint8 [n] out at a byte offset; the host restatement
    FeedForwardReferee.logits_exact on the state after the move (tests/test_env_gpu.py's reference)."""
    import test_env_gpu as TE
    from oracle import lattice
    torch = torch_mod
    lib = _mod("_lib")
    d = 7
    cfg = dict(d=d, error_model="DP", use_Y=False, volume_depth=3, p_phys=0.03, p_meas=0.03)
    ff = TE._random_stack(dq, np.random.RandomState(23), d, 4)
    m = lattice.Masks(d)

    def run(a):
        env = dq.VectorEnv(n_envs=n, seed=ENV_SEED, env_id_base=3, referee=ff, **cfg)
        assert env.mlp_referee
        env.reset()
        for t in range(6):
            env.step(env.select_actions(t), auto_reset=True)
        move = env.select_actions(6).cpu().numpy()
        move[0] = env.identity_index
        st = env.export_state().cpu().numpy().view(np.uint64)
        x, z = [int(v) for v in st[:, 0]], [int(v) for v in st[:, 1]]
        for i, a_ in enumerate(move):                               # the class is that of the state AFTER the move
            if a_ < d * d:
                x[i] ^= 1 << int(a_)
            elif a_ < 2 * d * d:
                z[i] ^= 1 << int(a_ - d * d)
        grids = np.stack([m.word_to_grid(m.syndrome_word(xi, zi)).reshape(-1) for xi, zi in zip(x, z)])
        a.request("move", (n,), torch.int32, 4, init=move)
        a.request("classes", (n,), torch.uint8, 1)
        lib.check(lib.lib().dq_env_referee_classes(env._h, lib.ptr(a.take("move")), lib.ptr(a.take("classes")), lib.current_stream()))
        torch.cuda.synchronize()
        env.close()
        return np.argmax(ff.logits_exact(grids), axis=1).astype(np.uint8)

    out, want = both_fills(run)
    assert np.array_equal(out["classes"], want)
    if n == 33:
        assert len(set(want.tolist())) >= 2


# ---- the sampled runs ----------------------------------------------------------------------------------------------------------------------
def _rate_arrays(n):
    return np.ascontiguousarray(np.linspace(0.01, 0.03, n)), np.ascontiguousarray(np.linspace(0.02, 0.005, n))


RUN_OUT = (("hidden", "u8dd"), ("trivial", "u8"), ("frame", "u8dd"), ("weight", "i2"), ("ndef", "i2"), ("rounds", "i2"), ("syn", "syn"))
RUN_FORMS = (("uni_all", False, True), ("uni_min", False, False), ("each_all", True, True), ("each_min", True, False))


def _request_run_outputs(a, torch, tag, n, d, T, everything):
    """The outputs of one sampled run: hidden, trivial and frame always, the four nullable ones (weight, n_defects, rounds, syndromes) when `everything`."""
    shapes = {"u8dd": ((n, d, d), torch.uint8, 1), "u8": ((n,), torch.uint8, 1), "i2": ((n, 2), torch.int32, 4), "syn": ((n, T, d + 1, d + 1), torch.uint8, 1)}
    for key, kind in RUN_OUT[:3 if not everything else None]:
        a.request(f"{tag}_{key}", *shapes[kind])


def _check_run(out, tag, everything, syn, hid, triv, decoded, n, d):
    frame, weight, ndef, rounds = decoded
    assert np.array_equal(arr(out[f"{tag}_hidden"], np.uint8, hid.shape), hid), (tag, "hidden")
    assert np.array_equal(out[f"{tag}_trivial"], triv), (tag, "trivial")
    assert np.array_equal(arr(out[f"{tag}_frame"], np.uint8, (n, d, d)), frame), (tag, "frame")
    if everything:
        assert np.array_equal(arr(out[f"{tag}_syn"], np.uint8, syn.shape), syn), (tag, "syndromes")
        for key, want in (("weight", weight), ("ndef", ndef), ("rounds", rounds)):
            assert np.array_equal(arr(out[f"{tag}_{key}"], np.int32, (n, 2)), want), (tag, key)


@pytest.mark.parametrize("final_round", ["faulty", "perfect"])
@pytest.mark.parametrize("n", [5, 67])
def test_narrow_stream_runs(dq, torch_mod, n, final_round):
    """dq_stream_run_uf and dq_stream_run_uf_closed at d = 5 DP, window 5, T = 12, commit 2: uniform rates and per-stream double arrays (host memory,
    8-byte aligned, between guards of their own), each with every nullable output given and with every one NULL.  The syndromes are the sampler's
    restatement (closed_uf_ref.sample_streams), the rest stream_uf_ref / closed_uf_ref on them."""
    torch = torch_mod
    import closed_uf_ref as C
    import shipped
    import stream_uf_ref as S
    D = _mod("decoder")
    cfg = shipped.CONFIGS[T.DEC_FAMILY]
    d, depth, model = cfg["d"], cfg["volume_depth"], cfg["error_model"]
    rounds_T, commit, base, closed = 12, 2, 2 ** 32 - 3, final_round == "perfect"
    ph, pm = _rate_arrays(n)
    venv = T._lut_env(dq)
    ev = D.Evaluator(d, model, cfg["use_Y"], depth, chunk=n)
    try:
        def run(a):
            h, hp, hm = host_rates(torch, a.fill, ph, pm)
            for tag, each, everything in RUN_FORMS:
                _request_run_outputs(a, torch, tag, n, d, rounds_T, everything)
            for tag, each, everything in RUN_FORMS:
                k = (lambda key, tag=tag: a.take(f"{tag}_{key}")) if everything else (lambda key: None)
                ev.stream_run_into(venv, n, rounds_T, commit, base, ENV_SEED, hp if each else 0.011, hm if each else 0.011, a.take(f"{tag}_hidden"),
                                   a.take(f"{tag}_trivial"), a.take(f"{tag}_frame"), k("weight"), k("ndef"), k("rounds"), syndromes=k("syn"),
                                   final_round=final_round)
            torch.cuda.synchronize()
            h.verify()

        out, _ = both_fills(run)
    finally:
        ev.close(); venv.close()
    for each in (False, True):
        syn, hid, triv = C.sample_streams(d, model, rounds_T, n, ph if each else 0.011, pm if each else 0.011, ENV_SEED, base, closed=closed)
        decoded = (C.decode(d, syn, depth, commit, True) if closed else S.decode(d, syn, depth, commit))[:4]
        assert syn.any() and decoded[0].any()
        for tag, e, everything in RUN_FORMS:
            if e == each:
                _check_run(out, tag, everything, syn, hid, triv, decoded, n, d)


WIDE_RUN_MODES = [("unit", "perfect"), ("pair", "faulty"), ("pair", "perfect"), ("pairs", "faulty"), ("pairs", "perfect"),
                  ("triple", "faulty"), ("triple", "perfect"), ("triples", "faulty"), ("triples", "perfect")]


@pytest.mark.parametrize("mode,final_round", WIDE_RUN_MODES, ids=[f"{m}-{f}" for m, f in WIDE_RUN_MODES])
@pytest.mark.parametrize("d,n", T.UF_SHAPES)
def test_wide_uf_runs(dq, torch_mod, d, n, mode, final_round):
    """dq_wide_uf_run_closed (unit weights), dq_wide_uf_run_weighted (the pair (3, 2); per-stream uint8 [n][2] at a byte offset) and dq_wide_uf_run_correlated
    (the triple (4, 4, 1); per-stream uint8 [n][3]), open and closed: T = 5, window 2, commit 1, lattice ids that wrap; uniform rates and per-stream double
    arrays, each with every nullable output given and with every one NULL.  References: closed_uf_ref.sample_streams and test_guarded_gpu._uf_reference."""
    torch = torch_mod
    import closed_uf_ref as C
    DW = _mod("decoder_wide")
    closed, base = final_round == "perfect", 2 ** 32 - 2
    ph, pm = _rate_arrays(n)
    ev = DW.WideEvaluator(d, "DP", window=T.UF_W, chunk=n)
    try:
        def run(a):
            h, hp, hm = host_rates(torch, a.fill, ph, pm)
            if mode in ("pairs", "triples"):
                rows = T._uf_weight_rows(n, 2 if mode == "pairs" else 3)
                a.request("each", rows.shape, torch.uint8, 1, init=rows)
            for tag, each, everything in RUN_FORMS:
                _request_run_outputs(a, torch, tag, n, d, T.UF_T, everything)
            weights = {"unit": None, "pair": (3, 2), "triple": (4, 4, 1)}[mode] if mode in ("unit", "pair", "triple") else a.take("each")
            for tag, each, everything in RUN_FORMS:
                k = (lambda key, tag=tag: a.take(f"{tag}_{key}")) if everything else (lambda key: None)
                ev.run_into(n, T.UF_T, T.UF_C, base, ENV_SEED, hp if each else T.UF_P, hm if each else T.UF_P, a.take(f"{tag}_hidden"),
                            a.take(f"{tag}_trivial"), a.take(f"{tag}_frame"), k("weight"), k("ndef"), k("rounds"), syndromes=k("syn"),
                            final_round=final_round, weights=weights)
            torch.cuda.synchronize()
            h.verify()

        out, _ = both_fills(run)
    finally:
        ev.close()
    for each in (False, True):
        syn, hid, triv = C.sample_streams(d, "DP", T.UF_T, n, ph if each else T.UF_P, pm if each else T.UF_P, ENV_SEED, base, closed=closed)
        decoded = T._uf_reference(mode, d, syn, closed, n)
        assert syn.any() and (decoded[0].any() or (d, n) == (3, 1))     # (the one d = 3 stream at the array's rates decodes to the empty frame)
        for tag, e, everything in RUN_FORMS:
            if e == each:
                _check_run(out, tag, everything, syn, hid, triv, decoded, n, d)


# ---- the teachers --------------------------------------------------------------------------------------------------------------------------
EPS, SHARE = 0.5, 0.5


def _branches(rule, q, legal, n, seed, base, t):
    """(greedy, uniform, guided) lattice counts of the selection rule at policy counter t: with guide_share = 1 the rule's flags are its explore draws."""
    explore = rule(q, legal, np.zeros(n, np.int32), EPS, 1.0, True, seed, base, t)[1].astype(bool)
    guided = rule(q, legal, np.zeros(n, np.int32), EPS, SHARE, True, seed, base, t)[1].astype(bool)
    assert not (guided & ~explore).any()
    return int((~explore).sum()), int((explore & ~guided).sum()), int(guided.sum())


def _policy_counter(rule, q, legal, n, seed, base):
    """The first policy counter at which each of the three branches is taken by at least one lattice (chosen on the CPU, from the rule alone)."""
    for t in range(256):
        if min(_branches(rule, q, legal, n, seed, base, t)) >= 1:
            return t
    raise AssertionError("no policy counter below 256 takes all three branches")


@pytest.fixture(scope="module")
def narrow_evaluators(dq):
    """One decoder.Evaluator per lattice shape for the whole module: its matching and union-find tables are built once."""
    made = {}

    def get(name):
        if name not in made:
            cfg = T.NARROW[name]
            made[name] = dq.decoder.Evaluator(cfg["d"], cfg["error_model"], cfg["use_Y"], cfg["volume_depth"], chunk=33)
        return made[name]

    yield get
    for ev in made.values():
        ev.close()


TEACHER_P, TEACHER_STEPS = 0.03, 4


@functools.lru_cache(maxsize=None)
def _narrow_teacher_case(name, n):
    """The C oracle alone: n lattices at p = 0.03 after 4 uniform steps with auto-reset.  Returns the actions played, the volumes uint8 [n, depth, d+1, d+1],
    the completed sets, the done flags, the legal words, the state words compared with the device's, Q rows and the policy counter of the guided calls."""
    import union_find_ref as U
    from oracle import c_oracle, lattice
    dq = _mod("decoder")
    cfg = dict(T.NARROW[name], p_phys=TEACHER_P, p_meas=TEACHER_P)
    d, depth = cfg["d"], cfg["volume_depth"]
    base = 4096 * 3
    ref = c_oracle.COracleEnv(n_envs=n, seed=ENV_SEED, env_id_base=base, **cfg)
    ref.reset()
    played = []
    for t in range(TEACHER_STEPS):
        played.append(ref.policy_uniform_legal(t))
        ref.step(played[-1], auto_reset=True)
    rs = ref.export()
    vol = np.zeros((n, depth, d + 1, d + 1), dtype=np.uint8)
    for s, (a, b) in enumerate(lattice.Masks(d).order):
        vol[:, :, a, b] = ((rs["volume"] >> np.uint64(s)) & np.uint64(1)).astype(np.uint8)
    completed = [dq.completed_from_words(w0, w1) for w0, w1 in rs["completed"]]
    done = ref.done.astype(bool).copy()
    uf_frame = U.decode(d, vol, depth)[0]
    identity = ref.num_actions - 1
    uf_teacher = np.array([identity if done[i] else dq.frame_to_actions(uf_frame[i], completed[i], d, cfg["error_model"], cfg["use_Y"])[1]
                           for i in range(n)], dtype=np.int32)
    q = np.random.RandomState(17 + n).randn(n, ref.num_actions).astype(np.float32)
    legal = ref.legal.copy()
    t = _policy_counter(dq.guided_actions, q, legal, n, ENV_SEED, base) if n == 33 else TEACHER_STEPS
    return dict(cfg=cfg, base=base, played=played, vol=vol, completed=completed, done=done, legal=legal, state=rs, uf_teacher=uf_teacher, q=q, t=t,
                identity=identity)


@pytest.mark.parametrize("n", [5, 33])
@pytest.mark.parametrize("name", ["d3dp", "c3", "c5"])
def test_narrow_teachers(dq, torch_mod, narrow_evaluators, name, n):
    """dq_env_match_select, dq_env_uf_select, dq_env_guided_select and dq_env_guided_select_uf on lattices mid-episode (d = 3, 5, 7; the C oracle's state
    after 4 steps at p = 0.03): actions int32 [n], flags uint8 [n] at byte offsets, Q rows float [n][A].  The guided forms run at eps = guide_share = 0.5
    with q given (masked greedy) and NULL, with the flag outputs given and NULL.  References: decoder.frame_to_actions on the frame of union_find_ref (the
    union-find teacher) and of matching_decode on the same volumes (the matching teacher: the family's reference), and decoder.guided_actions."""
    torch = torch_mod
    D = dq.decoder
    c = _narrow_teacher_case(name, n)
    cfg, base, q, t, legal = c["cfg"], c["base"], c["q"], c["t"], c["legal"]
    d, model, use_Y = cfg["d"], cfg["error_model"], cfg["use_Y"]
    ev = narrow_evaluators(name)
    if n == 33:                                                     # every branch occurs: asserted on the rule alone, before any launch
        assert min(_branches(D.guided_actions, q, legal, n, ENV_SEED, base, t)) >= 1
        assert (c["uf_teacher"] != c["identity"]).sum() >= 3 and any(len(s) for s in c["completed"])
    want = {}

    def run(a):
        env = dq.VectorEnv(n_envs=n, seed=ENV_SEED, env_id_base=base, **cfg)
        env.reset()
        for s in range(TEACHER_STEPS):
            env.step(torch.from_numpy(c["played"][s]).cuda(), auto_reset=True)
        st = env.export_state().cpu().numpy().view(np.uint64)
        assert np.array_equal(st[:, 11:], c["state"]["volume"]) and np.array_equal(st[:, 6:8], c["state"]["completed"])
        assert np.array_equal(env.legal.cpu().numpy().view(np.uint64), legal) and np.array_equal(env.done.cpu().numpy().astype(bool), c["done"])
        if not want:                                                # the matching teacher's frame: matching_decode on ordinary tensors, once
            res = D.matching_decode(c["vol"], env, to_host=True, evaluator=ev)
            want["m_act"] = np.array([c["identity"] if c["done"][i] else D.frame_to_actions(res.frame[i], c["completed"][i], d, model, use_Y)[1]
                                      for i in range(n)], dtype=np.int32)
            want["m_inexact"] = np.where(c["done"], 0, res.inexact).astype(np.uint8)
        a.request("q", q.shape, torch.float32, 4, init=q)
        for k in ("m_act", "m_act0", "u_act", "gm_act", "gm_act0", "gu_act", "gu_act0"):
            a.request(k, (n,), torch.int32, 4)
        for k in ("m_inexact", "gm_guided", "gm_inexact", "gu_guided", "gu_inexact"):
            a.request(k, (n,), torch.uint8, 1)
        k = a.take
        env.match_select(ev, out=k("m_act"), out_inexact=k("m_inexact"))
        env.match_select(ev, out=k("m_act0"))
        env.match_select(ev, out=k("u_act"), method="union_find")
        for g, method in (("gm", "matching"), ("gu", "union_find")):
            env.guided_select(ev, t, q=k("q"), eps=EPS, guide_share=SHARE, masked_greedy=True, out=k(g + "_act"), out_guided=k(g + "_guided"),
                              out_inexact=k(g + "_inexact"), method=method)
            env.guided_select(ev, t, q=None, eps=EPS, guide_share=SHARE, masked_greedy=True, out=k(g + "_act0"), method=method)
        assert torch.equal(env.export_state().cpu(), torch.from_numpy(st.view(np.int64)))      # the selections do not modify the environment
        torch.cuda.synchronize()
        env.close()

    out, _ = both_fills(run)
    i32 = lambda key: arr(out[key], np.int32)
    assert np.array_equal(i32("m_act"), want["m_act"]) and np.array_equal(i32("m_act0"), want["m_act"])
    assert np.array_equal(out["m_inexact"], want["m_inexact"])
    assert np.array_equal(i32("u_act"), c["uf_teacher"])
    for g, teacher, flag in (("gm", want["m_act"], want["m_inexact"]), ("gu", c["uf_teacher"], np.zeros(n, np.uint8))):
        act, guided = D.guided_actions(q, legal, teacher, EPS, SHARE, True, ENV_SEED, base, t)
        assert np.array_equal(i32(g + "_act"), act) and np.array_equal(out[g + "_guided"], guided), g
        assert np.array_equal(out[g + "_inexact"], np.where(guided == 1, flag, 0)), g
        act0, _ = D.guided_actions(None, legal, teacher, EPS, SHARE, True, ENV_SEED, base, t)
        assert np.array_equal(i32(g + "_act0"), act0), g


WIDE_TEACHERS = ("unit", "pair", "triple", "pairs", "triples")


@functools.lru_cache(maxsize=None)
def _wide_teacher_case(name):
    """The wide C oracle alone: the 5 lattices of test_guarded_gpu.WIDE after its 6 steps.  Returns the actions played, the exported state, the legal words,
    Q rows, the policy counter and, per mode, the union-find rule's action for every lattice."""
    import correlated_env_uf_ref as CR
    import test_env_wide_gpu as TW
    import test_wide_env_uf_cpu as TWU
    import weighted_env_uf_ref as WR
    from oracle import c_oracle
    dq = importlib.import_module("deepq-decoding_amd")
    cfg, p, base = T.WIDE[name]
    n = 5
    ref = c_oracle.COracleWideEnv(n_envs=n, seed=TW.SEED, env_id_base=base, p_phys=p, p_meas=p, **cfg)
    ref.reset()
    q = T._wide_q(n, ref.num_actions)
    played = []
    for t in range(6):
        played.append(ref.policy_uniform_legal(t) if t % 2 == 0 else TW._policy_oracle(q, ref.legal, 0.3, False, t, base))
        ref.step(played[-1], auto_reset=True)
    recs = ref.export()
    teacher = {}
    for mode in WIDE_TEACHERS:
        rows = T._uf_weight_rows(n, 2 if mode == "pairs" else 3)
        acts = []
        for i, rec in enumerate(recs):
            if mode == "unit":
                acts.append(TWU.rule_action(dq, cfg, rec))
            elif mode in ("pair", "pairs"):
                acts.append(WR.rule_action(dq, cfg, rec, (3, 2) if mode == "pair" else tuple(int(x) for x in rows[i])))
            else:
                acts.append(CR.rule_action(dq, cfg, rec, (4, 4, 1) if mode == "triple" else tuple(int(x) for x in rows[i])))
        teacher[mode] = np.array(acts, dtype=np.int32)
    legal = ref.legal.copy()
    t = _policy_counter(dq.decoder_wide.guided_actions_wide, q, legal, n, TW.SEED, base)
    return dict(played=played, state=ref.export_state(), legal=legal, q=q, t=t, teacher=teacher, identity=ref.num_actions - 1)


@pytest.mark.parametrize("name", list(T.WIDE))
def test_wide_teachers(dq, torch_mod, name):
    """dq_envb_uf_select_weighted / _correlated and dq_envb_guided_select_uf with its _weighted and _correlated forms on the 5 lattices of the wide cases
    after their 6 oracle steps: unit weights, the pair (3, 2), the triple (4, 4, 1), per-lattice uint8 [n][2] and [n][3] rows at a byte offset; the guided
    forms at eps = guide_share = 0.5 with q given (masked greedy) and NULL, guided_dev given and NULL.  References: the rules of test_wide_env_uf_cpu,
    weighted_env_uf_ref and correlated_env_uf_ref on the C oracle's records, and decoder_wide.guided_actions_wide."""
    import test_env_wide_gpu as TW
    torch = torch_mod
    DW = dq.decoder_wide
    cfg, p, base = T.WIDE[name]
    n = 5
    c = _wide_teacher_case(name)
    q, t, legal = c["q"], c["t"], c["legal"]
    assert min(_branches(DW.guided_actions_wide, q, legal, n, TW.SEED, base, t)) >= 1      # every branch occurs, on the rule alone
    assert any((c["teacher"][m] != c["identity"]).any() for m in WIDE_TEACHERS)

    def run(a):
        env = dq.VectorEnv(n_envs=n, seed=TW.SEED, env_id_base=base, backend="wide", p_phys=p, p_meas=p, **cfg)
        ev = DW.WideEvaluator(env.d, env.error_model, window=env.volume_depth, chunk=n, device=env.device)
        env.reset()
        for s in range(6):
            env.step(torch.from_numpy(c["played"][s]).cuda(), auto_reset=True)
        state = env.export_state()
        assert np.array_equal(state.cpu().numpy().view(np.uint64), c["state"])
        a.request("q", q.shape, torch.float32, 4, init=q)
        a.request("pairs", (n, 2), torch.uint8, 1, init=T._uf_weight_rows(n, 2))
        a.request("triples", (n, 3), torch.uint8, 1, init=T._uf_weight_rows(n, 3))
        for m in WIDE_TEACHERS:
            for k in ("act", "g_act", "g_act0"):
                a.request(f"{m}_{k}", (n,), torch.int32, 4)
            a.request(f"{m}_guided", (n,), torch.uint8, 1)
        k = a.take
        for m in WIDE_TEACHERS:
            weights = {"unit": None, "pair": (3, 2), "triple": (4, 4)}[m] if m in ("unit", "pair", "triple") else k(m)
            kw = dict(weights=weights, correlated=1) if m == "triple" else dict(weights=weights)
            env.uf_select_wide(ev, out=k(f"{m}_act"), **kw)
            env.guided_select_wide(ev, t, q=k("q"), eps=EPS, guide_share=SHARE, masked_greedy=True, out=k(f"{m}_g_act"), out_guided=k(f"{m}_guided"), **kw)
            env.guided_select_wide(ev, t, q=None, eps=EPS, guide_share=SHARE, masked_greedy=True, out=k(f"{m}_g_act0"), **kw)
        assert torch.equal(env.export_state(), state)               # the records are read in place and never written
        torch.cuda.synchronize()
        ev.close()
        env.close()

    out, _ = both_fills(run)
    for m in WIDE_TEACHERS:
        teacher = c["teacher"][m]
        assert np.array_equal(arr(out[f"{m}_act"], np.int32), teacher), m
        act, guided = DW.guided_actions_wide(q, legal, teacher, EPS, SHARE, True, TW.SEED, base, t)
        assert np.array_equal(arr(out[f"{m}_g_act"], np.int32), act) and np.array_equal(out[f"{m}_guided"], guided), m
        act0, _ = DW.guided_actions_wide(None, legal, teacher, EPS, SHARE, True, TW.SEED, base, t)
        assert np.array_equal(arr(out[f"{m}_g_act0"], np.int32), act0), m


# ---- the wide agent decode -----------------------------------------------------------------------------------------------------------------
DECODE_WIDE = {"d9_dp_depth3": dict(d=9, error_model="DP", use_Y=False, volume_depth=3), "d15_dpy_depth2": dict(d=15, error_model="DP", use_Y=True, volume_depth=2)}
DW_N, DW_MAX = 5, 4


@functools.lru_cache(maxsize=None)
def _decode_wide_case(name):
    """On the CPU: 5 sparse volumes, supplied Q rows whose restatement ends volumes in all three statuses (the first such seed), the restatement's result,
    the active list of every iteration, and an action-plane-sensitive network with the float64 oracle's decode of the same volumes."""
    import decode_ref as R
    import decode_wide_ref as WR
    from oracle import lattice
    cfg = DECODE_WIDE[name]
    A, _ = lattice.num_actions(cfg["d"], cfg["error_model"], cfg["use_Y"])
    grids = WR.sparse_grids(cfg, DW_N, seed=31)
    for seed in range(400):
        supplied = WR.SuppliedQ(DW_N, A, seed=seed, identity_rate=0.2)
        want = WR.reference_decode(cfg, grids, supplied, True, DW_MAX)
        if {R.IDENTITY, R.REPEAT, R.STOPPED} <= set(int(s) for s in want[2]):
            break
    else:
        raise AssertionError("no seed below 400 reaches the three statuses")
    steps = [len(c) + int(s != R.STOPPED) for c, s in zip(want[0], want[2])]
    active = [[v for v in range(DW_N) if steps[v] > k] for k in range(max(steps))]
    qrows = [np.ascontiguousarray(supplied.rows(k)[act]) for k, act in enumerate(active)]
    spec, flat = WR.sensitive_network(cfg, grids)
    qfun = lambda obs: O.forward(spec, flat, np.asarray(obs, dtype=np.uint8)[None])[0][0]
    net_want = [R.decode_volume(g, qfun, cfg["d"], cfg["error_model"], cfg["use_Y"], True, max_actions=DW_MAX) for g in grids]
    return dict(cfg=cfg, A=A, grids=grids, want=want, active=active, qrows=qrows, spec=spec, flat=flat, net_want=net_want)


@pytest.mark.parametrize("name", sorted(DECODE_WIDE))
def test_decode_wide(dq, torch_mod, name):
    """dq_decode_wide_pack from guarded volumes (4-byte aligned), dq_decode_wide_step driven by supplied Q rows of exactly [n_active][num_actions] floats
    through all three statuses, and dq_decode_wide_run with guarded parameters, pack and outputs, on a handle of max_volumes = n = 5; 163 actions at
    d = 9 and 676 at d = 15 (11 legal words).  corrections [n][max_actions], n_corr, frame and status are the restatement's (tests/decode_ref.py under
    tests/decode_wide_ref.py's rows; under the float64 oracle's Q-values for the run, test_decode_wide_gpu's near-tie rule with no volume allowed to
    differ).  dq_decode_wide_rows, _words and _active return pointers into the handle's own buffers: they are read and compared, they cannot be guarded."""
    torch = torch_mod
    import decode_ref as R
    import decode_wide_ref as WR
    import test_decode_wide_gpu as TDW
    lib = _mod("_lib")
    c = _decode_wide_case(name)
    cfg, A, grids, flat = c["cfg"], c["A"], c["grids"], c["flat"]
    d, n = cfg["d"], DW_N
    lists, frames, stats = c["want"]
    assert {R.IDENTITY, R.REPEAT, R.STOPPED} <= set(int(s) for s in stats) and len(c["active"]) >= 2
    L, P = lib.lib(), lib.ptr

    def run(a):
        dec = TDW.wide_decoder(dq, cfg, A, True, DW_MAX, n)
        try:
            a.request("syn", grids.shape, torch.uint8, 4, init=grids)
            a.request("params", (flat.size,), torch.float32, 16, init=flat)
            if dec.net.packed_bytes:                                # (0 where the fused chains do not cover the network: d = 15 runs per layer, without a pack)
                a.request("packed", (dec.net.packed_bytes,), torch.uint8, 16)
            for k, rows in enumerate(c["qrows"]):
                a.request(f"q{k}", rows.shape, torch.float32, 4, init=rows)
            for tag in ("s", "r"):
                a.request(tag + "_corr", (n, DW_MAX), torch.int32, 4)
                a.request(tag + "_ncorr", (n,), torch.int32, 4)
                a.request(tag + "_frame", (n, d, d), torch.uint8, 1)
                a.request(tag + "_status", (n,), torch.uint8, 1)
            k, st = a.take, lib.current_stream()
            outs = lambda tag: [k(tag + s) for s in ("_corr", "_ncorr", "_frame", "_status")]
            lib.check(L.dq_decode_wide_pack(dec._h, P(k("syn")), n, *(P(x) for x in outs("s")), st))
            rows0 = dec.rows(n).cpu().numpy()
            assert np.array_equal(rows0, WR.initial_observations(cfg, grids))
            assert bool((k("s_corr") == -1).all())
            for it, act in enumerate(c["active"]):
                got, count = dec.active()
                assert count == len(act) and got.cpu().numpy().tolist() == act, it
                nxt = ctypes.c_int(-1)
                lib.check(L.dq_decode_wide_step(dec._h, P(k(f"q{it}")), ctypes.byref(nxt), st))
                assert nxt.value == (len(c["active"][it + 1]) if it + 1 < len(c["active"]) else 0), it
            TDW.check_against_reference(cfg, A, grids, dec, [x.cpu().numpy() for x in outs("s")], c["want"], DW_MAX)
            pk = dec.net.pack(k("params"), out=k("packed")) if dec.net.packed_bytes else None
            iters = dec.decode_into(k("params"), pk, k("syn"), n, *outs("r"))
            torch.cuda.synchronize()
            return iters
        finally:
            dec.close()

    out, iters = both_fills(run)
    corr, ncorr = arr(out["s_corr"], np.int32, (n, DW_MAX)), arr(out["s_ncorr"], np.int32)
    assert [list(map(int, corr[i, :ncorr[i]])) for i in range(n)] == lists
    assert np.array_equal(arr(out["s_frame"], np.uint8, (n, d, d)), frames) and np.array_equal(out["s_status"], stats.astype(np.uint8))
    # the run: the float64 oracle's decode
    corr, ncorr = arr(out["r_corr"], np.int32, (n, DW_MAX)), arr(out["r_ncorr"], np.int32)
    got = [list(map(int, corr[i, :ncorr[i]])) for i in range(n)]
    want = c["net_want"]
    assert TDW.assert_same_or_near_tie(cfg, c["spec"], flat, grids, got, [list(w[0]) for w in want], True, max_disagree=0) == []
    assert np.all(corr[np.arange(DW_MAX)[None, :] >= ncorr[:, None]] == -1)
    assert np.array_equal(arr(out["r_frame"], np.uint8, (n, d, d)), np.stack([w[1] for w in want]))
    assert np.array_equal(out["r_status"], np.asarray([w[2] for w in want], dtype=np.uint8))
    assert iters == max(len(w[0]) + int(w[2] != R.STOPPED) for w in want) and sum(len(g) for g in got) > 0


# ---- the update that carries the environment step ---------------------------------------------------------------------------------------------
RING_T, RING_FILLED, RING_CUR = 9, 7, 8                             # the step writes slot 8 and its successor observation wraps to slot 0
UPD_SEED, UPD_T, LR, GAMMA, STEP_EPS = (1, 2), 5, 1e-3, 0.99, 0.3
STATS0 = np.array([3, 5, 7, 9], dtype=np.int64)
RIDE_CASES = ([(name, n, B, "all") for name in ("c3", "d3dp", "c5") for n in (5, 33) for B in (5, 33)]
              + [("c3", 33, 1029, "all"), ("c3", 33, 2049, "all"),    # the first sizes past fused_backward's col_split 4 -> 2 and 2 -> 1 switches, one-row last tiles
                 ("c3", 5, 5, "bare"), ("d3dp", 33, 33, "bare"),     # stats_dev NULL, sample NULL
                 ("c3", 33, 33, "huber")])                           # a finite delta_clip


@functools.lru_cache(maxsize=None)
def _ride_case(name, n, B):
    """On the CPU: the C oracle's lattices after w uniform steps (n = 33: the first w at which the carried step both ends an episode and spends a lattice's
    step on an auto-reset), the carried step's results, the initial rings, the minibatch rows of this update and of the next one, and the TD inputs."""
    import test_env_wide_gpu as TW
    from oracle import c_oracle, memory_oracle as M
    cfg, base = T.NARROW[name], 4096 * 3
    shape, A = TQ.SHAPES[name]
    rng = np.random.RandomState(1000 + 7 * n + B)
    q_step = rng.randn(n, A).astype(np.float32)
    for w in range(2, 200):
        ref = c_oracle.COracleEnv(n_envs=n, seed=ENV_SEED, env_id_base=base, **cfg)
        ref.reset()
        played = []
        for t in range(w):
            played.append(ref.policy_uniform_legal(t))
            ref.step(played[-1], auto_reset=True)
        a_step = TW._policy_oracle(q_step, ref.legal, STEP_EPS, True, w, base)
        ref.step(a_step, auto_reset=True)
        if n != 33 or (ref.done.any() and ref.was_reset.any()):
            break
    wr = ref.was_reset != 0
    ended = (ref.done != 0) & ~wr
    stats = np.array([ended.sum(), ref.lifetime[ended].sum(), ((ref.reward == 1.0) & ~wr).sum(), (~wr).sum()], dtype=np.int64)
    rings = dict(obs=(rng.rand(RING_T, n, *shape) < 0.3).astype(np.uint8), action=rng.randint(0, A, size=(RING_T, n)).astype(np.int32),
                 reward=(rng.rand(RING_T, n) < 0.4).astype(np.float32), term=(rng.rand(RING_T, n) < 0.15).astype(np.uint8))
    index = M.device_replay_rows(rings["term"], n, RING_T, RING_CUR, RING_FILLED, B, UPD_SEED, UPD_T, sample_base=0).astype(np.int32)
    index_next = M.device_replay_rows(rings["term"], n, RING_T, 0, RING_FILLED + 1, B, UPD_SEED, UPD_T + 1, sample_base=0).astype(np.int32)
    # the update reads nothing the step writes: no minibatch row, and no successor row, lies in slot 8 (or its successor observation in slot 0)
    assert (index // n != RING_CUR).all() and ((index + n) % (RING_T * n) // n != 0).all()
    q1o, q1t = (rng.randn(B, A).astype(np.float32) for _ in range(2))
    m0, v0 = (rng.rand(_n_params(name)) * 1e-3).astype(np.float32), (rng.rand(_n_params(name)) * 1e-6).astype(np.float32)
    return dict(name=name, cfg=cfg, base=base, w=w, played=played, q_step=q_step, a_step=a_step, ref=ref, stats=stats, rings=rings, index=index,
                index_next=index_next, q1o=q1o, q1t=q1t, m0=m0, v0=v0)


def _n_params(name):
    shape, A = TQ.SHAPES[name]
    return O.QNetSpec(shape, TQ.C_LAYERS, TQ.FF_LAYERS, A, dueling=True).n_params


class _Ride:
    """The buffers of one form of the update (tag) in an arena, or on ordinary tensors (arena None: the twins)."""

    def __init__(self, torch, a, tag, c, net, flat, n, B, with_env, with_opt=True, wide=False):
        self.torch, self.a, self.tag, self.c, self.n, self.B = torch, a, tag, c, n, B
        shape, A = TQ.SHAPES[c["name"]]
        d = c["cfg"]["d"]
        self.d, self.A, self.shape, self.stride = d, A, shape, d * d + 3
        P = net.n_params
        r = c["rings"]
        self.spec = {}
        io = lambda key, arr_, dt, al: self._add(key, arr_.shape, dt, al, arr_, True)
        out = lambda key, shp, dt, al: self._add(key, shp, dt, al, None, False)
        inp = lambda key, arr_, dt, al: self._add(key, arr_.shape, dt, al, arr_, False)
        io("params", flat, torch.float32, 16)
        inp("q1o", c["q1o"], torch.float32, 4); inp("q1t", c["q1t"], torch.float32, 4); inp("index", c["index"], torch.int32, 4)
        # wide: the gradient and the moments 16-byte aligned (the final reduction's f32x4 form with 16-byte stores to grads, params, m, v) and the
        # observation ring 16-byte aligned (the step's 16-byte observation store); else 4-byte-only and byte aligned (their scalar forms)
        gmv, obs_align = (16, 16) if wide else (4, 1)
        io("obs_ring", r["obs"], torch.uint8, obs_align); io("action_ring", r["action"], torch.int32, 4)
        io("reward_ring", r["reward"], torch.float32, 4); io("term_ring", r["term"], torch.uint8, 1)
        out("q0", (B, A), torch.float32, 4); out("y", (B,), torch.float32, 4); out("dq", (B, A), torch.float32, 4)
        out("met", (_mod("qnet").TD_METRICS_FLOATS,), torch.float32, 4); out("grads", (P,), torch.float32, gmv)
        if not with_env and not with_opt:
            out("grads_phases", (P,), torch.float32, gmv)           # dq_qnet_backward_phase(.., 0) then (.., 1) on the TD launch's dq
            ref = c["ref"]                                          # the job's own bookkeeping pointers: the carried step's results as pure inputs
            inp("st_done", ref.done, torch.uint8, 1); inp("st_was_reset", ref.was_reset, torch.uint8, 1)
            inp("st_lifetime", ref.lifetime.view(np.int32), torch.int32, 4); inp("st_reward", ref.reward, torch.float32, 4)
            io("stats", STATS0, torch.int64, 8)
        if with_opt:
            io("m", c["m0"], torch.float32, gmv); io("v", c["v0"], torch.float32, gmv)
        if with_env:
            inp("q_step", c["q_step"], torch.float32, 4)
            out("legal", (n, 2), torch.int64, 8); out("lifetime", (n,), torch.int32, 4); out("was_reset", (n,), torch.uint8, 1)
            out("patch", (n, self.stride), torch.int32, 4); out("index_next", (B,), torch.int32, 4)
            io("stats", STATS0, torch.int64, 8)

    def _add(self, key, shape, dtype, align, init, inout):
        self.spec[key] = (tuple(shape), dtype, init)
        if self.a is not None:
            self.a.request(f"{self.tag}_{key}", shape, dtype, align, init=init, inout=inout)

    def materialise(self):
        """Arena views (after every form's requests were made), or ordinary tensors with the same contents."""
        torch = self.torch
        self.t = {}
        for key, (shape, dtype, init) in self.spec.items():
            if self.a is not None:
                self.t[key] = self.a.take(f"{self.tag}_{key}")
            elif init is None:                                      # (prefilled as the arena prefills an output)
                nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
                self.t[key] = torch.full((nbytes,), G.OUT_FILL, dtype=torch.uint8, device="cuda").view(dtype).view(shape)
            else:
                self.t[key] = torch.from_numpy(np.ascontiguousarray(init)).cuda()
        return self

    def forward(self, net):
        t, n = self.t, self.n
        net.forward(t["params"], t["obs_ring"].view(RING_T * n, *self.shape), index=t["index"], training=True, seed=UPD_SEED, t=UPD_T, sample_base=0,
                    out=t["q0"])

    def step_stats(self):
        """dq_td_job's done_dev, was_reset_dev, lifetime_dev, step_reward_dev, n and stats_dev (the plain forms: dq_episode_stats in the dense backward's
        first kernel): what the step that was just made wrote -- ring slot 8 and the step's own outputs --, or the oracle's results as inputs."""
        t = self.t
        if "st_done" in t:
            return (t["st_done"], t["st_was_reset"], t["st_lifetime"], t["st_reward"], self.n, t["stats"])
        return (t["term_ring"][RING_CUR], t["was_reset"], t["lifetime"], t["reward_ring"][RING_CUR], self.n, t["stats"])

    def td(self, delta_clip=None, step_stats=None):
        t = self.t
        return dict(step_stats=step_stats, q_online_s1=t["q1o"], q_target_s1=t["q1t"], q_s0=t["q0"], reward=t["reward_ring"].view(-1), terminal=t["term_ring"].view(-1),
                    action=t["action_ring"].view(-1), index=t["index"], gamma=GAMMA, grad_scale=1.0 / self.B, y=t["y"], dq=t["dq"], metrics=t["met"],
                    delta_clip=delta_clip)

    def sample_job(self):
        lib, t = _mod("_lib"), self.t
        sj = lib.SampleJob()
        sj.terminal_ring_dev, sj.n_slots, sj.head_slot, sj.filled_slots, sj.batch = lib.ptr(t["term_ring"]), RING_T, 0, RING_FILLED + 1, self.B
        sj.seed[0], sj.seed[1], sj.t, sj.sample_base, sj.index_dev = UPD_SEED[0], UPD_SEED[1], UPD_T + 1, 0, lib.ptr(t["index_next"])
        return sj

    def step(self, sample, stats):
        """dq_env_step_job's fields: the action, reward and done pointers lie inside ring slot 8, the observation pointer is ring slot 0."""
        t = self.t
        return dict(q=t["q_step"], eps=STEP_EPS, masked_greedy=1, seed=ENV_SEED, t=self.c["w"], action=t["action_ring"][RING_CUR], auto_reset=1,
                    obs=t["obs_ring"][0], reward=t["reward_ring"][RING_CUR], done=t["term_ring"][RING_CUR], legal=t["legal"], lifetime=t["lifetime"],
                    was_reset=t["was_reset"], sample=self.sample_job() if sample else None, stats=t["stats"] if stats else None)

    def arm(self, env):
        lib = _mod("_lib")
        lib.check(env.L.dq_env_patch_output(env._h, lib.ptr(self.t["patch"]), self.stride))

    def host(self):
        self.torch.cuda.synchronize()
        return {k: v.cpu().numpy().copy() for k, v in self.t.items()}


def _played_env(dq, torch, c, n, **kw):
    env = dq.VectorEnv(n_envs=n, seed=ENV_SEED, env_id_base=c["base"], **c["cfg"], **kw)
    env.reset()
    for s in range(c["w"]):
        env.step(torch.from_numpy(c["played"][s]).cuda(), auto_reset=True)
    return env


def _env_results(c, h, env_obs_of_patch, n, sample, stats, what):
    """The carried step against the C oracle, and every ring in full: only slot 8 of the action, reward and terminal rings and slot 0 of the observation
    ring changed."""
    ref, r = c["ref"], c["rings"]
    want = {k: v.copy() for k, v in r.items()}
    want["action"][RING_CUR], want["reward"][RING_CUR], want["term"][RING_CUR], want["obs"][0] = c["a_step"], ref.reward, ref.done, ref.obs
    for k in ("action", "reward", "term", "obs"):
        assert np.array_equal(h[k + "_ring"].view(np.uint8), want[k].view(np.uint8)), (what, k + " ring")
    assert np.array_equal(h["legal"].view(np.uint64), ref.legal) and np.array_equal(h["lifetime"].view(np.uint32), ref.lifetime), what
    assert np.array_equal(h["was_reset"], ref.was_reset), what
    d2 = c["cfg"]["d"] ** 2
    assert np.array_equal(env_obs_of_patch, ref.obs), (what, "patch")
    assert (h["patch"][:, d2:] == 0x77777777).all(), (what, "the words between d * d and the stride are left alone")
    if sample:
        assert np.array_equal(h["index_next"], c["index_next"]), (what, "index_next")
    else:
        assert untouched(h["index_next"].view(np.uint8)), what
    assert np.array_equal(h["stats"], STATS0 + c["stats"] if stats else STATS0), (what, "stats")


@pytest.mark.parametrize("name,n,B,variant", RIDE_CASES, ids=[f"{a}-n{b}-B{c_}-{v}" for a, b, c_, v in RIDE_CASES])
def test_update_carrying_the_environment_step(dq, torch_mod, name, n, B, variant):
    """dq_qnet_td_backward_adam_env with every pointer of dq_td_job, dq_env_step_job and dq_sample_job, the armed patch words (stride d * d + 3), params
    (16-byte aligned), grads, m and v in the arena; beside it, on buffers and environments of their own in the same arena, dq_env_act_step_sample +
    dq_qnet_td_backward_adam, dq_qnet_td_backward_phase0_env + dq_qnet_backward_phase(.., 1), and dq_qnet_td_backward_phase0 + dq_qnet_backward_phase(.., 1).
    The two plain forms carry the TD job's own bookkeeping pointers (done_dev, was_reset_dev, lifetime_dev, step_reward_dev, n, stats_dev in/out) -- in the
    _env forms td->n must be 0 and the step's stats_dev does that work -- against dq_episode_stats' sums.  Everything runs twice: with grads, m, v and the
    observation ring 16-byte aligned (the final reduction's f32x4 form, the step's 16-byte observation store) and 4-byte-only / byte aligned (their scalar
    forms), with equal bits.
    The step's action, reward and done pointers are ring slot 8, its observation pointer is ring slot 0 of rings of 9 slots (filled_slots 7).
    References: the C oracle for the step; a twin network and environment on ordinary tensors making the separate calls dq_env_act_step_sample, dq_td_step,
    dq_qnet_backward, dq_adam_step (y, dq, the step, the next minibatch: bit for bit; the gradient: _grad_bounds) and making dq_qnet_td_backward_adam
    (gradient, parameters and moments bit for bit: the fused TD launch forms gY2 as a scalar times a table row, the separate calls on the matrix pipe --
    test_qnet_gpu.test_td_backward_adam_equals_the_separate_calls); oracle/dqn_oracle.py for Q, y, loss, mean_q (tol()) and the gradient (_grad_bounds)."""
    torch = torch_mod
    Q, lib = _mod("qnet"), _mod("_lib")
    c = _ride_case(name, n, B)
    ref = c["ref"]
    if n == 33:
        assert ref.done.any() and ref.was_reset.any() and c["stats"][0] >= 1
    sample, stats, delta = variant != "bare", variant != "bare", 0.5 if variant == "huber" else None
    spec, net, params, flat, _, _ = TQ._setup(dq, torch, name, B)
    nconv = net.n_conv_params
    twins = {}

    def backward_adam(r, env=None, bookkeeping=False):
        r.forward(net)
        if env is None:
            net.td_backward_adam(r.t["params"], r.td(delta, r.step_stats() if bookkeeping else None), r.t["grads"], r.t["m"], r.t["v"], UPD_T, LR)
        else:
            r.arm(env)
            net.td_backward_adam_env(r.t["params"], r.td(delta), r.t["grads"], r.t["m"], r.t["v"], UPD_T, LR, 0.9, 0.999, 1e-7, env._h, r.step(sample, stats))
        Q.td_metrics(r.t["met"], B)

    def act_step(r, env, bookkeeping=True):
        s = r.step(sample, stats)
        r.arm(env)
        L, P = env.L, lib.ptr
        seed = (ctypes.c_uint32 * 2)(*ENV_SEED)
        args = (env._h, P(s["q"]), STEP_EPS, 1, seed, c["w"], P(s["action"]), 1, P(s["obs"]), P(s["reward"]), P(s["done"]), P(s["legal"]),
                P(s["lifetime"]), P(s["was_reset"]))
        if sample:
            lib.check(L.dq_env_act_step_sample(*args, ctypes.byref(s["sample"]), lib.current_stream()))
        else:
            lib.check(L.dq_env_act_step(*args, lib.current_stream()))
        if stats and bookkeeping:                                   # (the separate calls' bookkeeping: dq_episode_stats)
            lib.check(L.dq_episode_stats(P(s["done"]), P(s["was_reset"]), P(s["lifetime"]), P(s["reward"]), n, P(r.t["stats"]), lib.current_stream()))

    def run(a, wide):
        envs = [_played_env(dq, torch, c, n) for _ in range(3)]
        try:
            ride = _Ride(torch, a, "ride", c, net, flat, n, B, True, wide=wide)
            plain = _Ride(torch, a, "plain", c, net, flat, n, B, True, wide=wide)
            ph_env = _Ride(torch, a, "phenv", c, net, flat, n, B, True, with_opt=False, wide=wide)
            ph = _Ride(torch, a, "ph", c, net, flat, n, B, False, with_opt=False, wide=wide)
            for r in (ride, plain, ph_env, ph):
                r.materialise()
            backward_adam(ride, envs[0])
            act_step(plain, envs[1], bookkeeping=False)              # (its bookkeeping is the TD job's, in the backward that follows)
            backward_adam(plain, bookkeeping=stats)
            ph_env.forward(net)
            ph_env.arm(envs[2])
            net.td_backward_phase0_env(ph_env.t["params"], ph_env.td(delta), ph_env.t["grads"], envs[2]._h, ph_env.step(sample, stats))
            after0 = ph_env.t["grads"].cpu().numpy().copy()
            net.backward_phase(ph_env.t["params"], ph_env.t["dq"], ph_env.t["grads"], 1)
            ph.forward(net)
            net.td_backward_phase0(ph.t["params"], ph.td(delta, ph.step_stats() if stats else None), ph.t["grads"])
            net.backward_phase(ph.t["params"], ph.t["dq"], ph.t["grads"], 1)
            ph.forward(net)
            net.set_grad_scale(1.0 / B)
            net.backward_phase(ph.t["params"], ph.t["dq"], ph.t["grads_phases"], 0)
            after0_plain = ph.t["grads_phases"].cpu().numpy().copy()
            net.backward_phase(ph.t["params"], ph.t["dq"], ph.t["grads_phases"], 1)
            net.set_grad_scale(0.0)
            for r in (ph_env, ph):
                Q.td_metrics(r.t["met"], B)
            hosts = {r.tag: r.host() for r in (ride, plain, ph_env, ph)}
            patches = {r.tag: envs[0].patch_to_obs(r.t["patch"]).cpu().numpy() for r in (ride, plain, ph_env)}
            states = [e.export_state().cpu().numpy() for e in envs]
            if not twins:                                           # the twins on ordinary tensors, once
                e_sep, e_one = _played_env(dq, torch, c, n), None
                sep = _Ride(torch, None, "sep", c, net, flat, n, B, True).materialise()
                act_step(sep, e_sep)
                sep.forward(net)
                lib.check(lib.lib().dq_td_step(ctypes.byref(Q._td_job(sep.td(delta))), lib.current_stream()))
                net.set_grad_scale(1.0 / B)                         # (the loss scale dq carries: test_qnet_gpu's separate calls)
                net.backward(sep.t["params"], sep.t["dq"], grads=sep.t["grads"])
                net.set_grad_scale(0.0)
                Q.adam_step(sep.t["params"], sep.t["grads"], sep.t["m"], sep.t["v"], UPD_T, LR)
                Q.td_metrics(sep.t["met"], B)
                one = _Ride(torch, None, "one", c, net, flat, n, B, False).materialise()
                backward_adam(one)
                twins.update(sep=sep.host(), one=one.host(), sep_patch=e_sep.patch_to_obs(sep.t["patch"]).cpu().numpy(),
                             sep_state=e_sep.export_state().cpu().numpy())
                e_sep.close()
            return hosts, patches, states, (after0, after0_plain)
        finally:
            torch.cuda.synchronize()
            for e in envs:
                e.close()

    # the 16-byte forms (what ordinary, 256-byte aligned tensors take) and the scalar forms, between guards both, with equal bits
    out, (hosts, patches, states, (after0, after0_plain)) = both_fills(lambda a: run(a, True))
    out_scalar, _ = both_fills(lambda a: run(a, False))
    G.same_bits(out, out_scalar)
    sep, one = twins["sep"], twins["one"]
    bits = lambda x, y_: np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y_).view(np.uint8))
    # the carried step: the C oracle, every ring in full, and the lattices' records equal to the twin's
    _env_results(c, sep, twins["sep_patch"], n, sample, stats, "separate calls")
    for tag in ("ride", "plain", "phenv"):
        _env_results(c, hosts[tag], patches[tag], n, sample, stats, tag)
    for st in states:
        assert np.array_equal(st, twins["sep_state"])
    assert np.array_equal(hosts["ph"]["stats"], STATS0 + c["stats"] if stats else STATS0)      # dq_episode_stats' sums, from the TD job's own pointers
    for key, want_in in (("st_done", ref.done), ("st_was_reset", ref.was_reset), ("st_lifetime", ref.lifetime), ("st_reward", ref.reward)):
        assert np.array_equal(hosts["ph"][key].view(np.uint8), want_in.view(np.uint8)), key
    # the update
    idx = c["index"]
    rows = c["rings"]["obs"].reshape(RING_T * n, *TQ.SHAPES[name][0])[idx]
    keep = O.dropout_keep_mask(UPD_SEED, UPD_T, np.arange(B), 512, 0.2)
    q_ref, cache = O.forward(spec, flat, rows, training=True, keep_masks=[keep])
    rew, term, act = (c["rings"][k].reshape(-1)[idx] for k in ("reward", "term", "action"))
    h = hosts["ride"]
    assert np.abs(h["q0"] - q_ref).max() < TQ.tol(q_ref)
    y_ref = O.td_targets(c["q1o"].astype(np.float64), c["q1t"].astype(np.float64), rew, term, GAMMA)
    assert np.abs(h["y"] - y_ref).max() < TQ.tol(y_ref)
    if delta is None:
        loss_ref, mq_ref, _ = O.loss_and_grad(h["q0"].astype(np.float64), act, h["y"].astype(np.float64))
    else:
        import test_huber_gpu as TH
        diff32 = h["q0"][np.arange(B), act] - h["y"]
        assert 0 < (np.abs(diff32) > np.float32(delta)).sum() < B
        loss_ref, mq_ref = float(np.mean(TH.huber_h(diff32.astype(np.float64), delta))), float(h["q0"].max(axis=1).astype(np.float64).mean())
    g_ref = O.backward(spec, flat, cache, h["dq"].astype(np.float64))
    for tag in ("ride", "plain", "phenv", "ph"):
        g = hosts[tag]
        for key in ("q0", "y", "dq"):
            assert bits(g[key], sep[key]) and bits(g[key], one[key]), (tag, key)
        assert abs(g["met"][0] - loss_ref) < TQ.tol(loss_ref) and abs(g["met"][1] - mq_ref) < TQ.tol(mq_ref), tag
        assert bits(g["grads"], one["grads"]), (tag, "gradient")
        T._grad_bounds(spec, g["grads"], g_ref)
        T._grad_bounds(spec, g["grads"], sep["grads"].astype(np.float64))
        if tag in ("ride", "plain"):
            for key in ("params", "m", "v"):
                assert bits(g[key], one[key]), (tag, key)
            assert not bits(g["params"], flat)
        else:
            assert bits(g["params"], flat), tag
        for key in ("q1o", "q1t", "index"):
            assert bits(g[key], c[key])
    # phase 0 alone: the dense range is complete and the convolutional range of grads_dev is left alone (include/deepq_hip.h); the two phases of
    # dq_qnet_backward_phase give dq_qnet_backward's bits
    for first, whole in ((after0, hosts["phenv"]["grads"]), (after0_plain, hosts["ph"]["grads_phases"])):
        assert bits(first[nconv:], whole[nconv:]) and untouched(first[:nconv].view(np.uint8))
    assert bits(hosts["ph"]["grads_phases"], sep["grads"])


def test_a_step_that_cannot_ride_is_refused_with_every_buffer_untouched(dq, torch_mod):
    """include/deepq_hip.h: only the fused chains carry the environment step, and a step whose referee is the Dense stack does not ride:
    DQ_ERR_UNSUPPORTED from dq_qnet_td_backward_adam_env and dq_qnet_td_backward_phase0_env, with every output still 0x77, every in/out buffer still
    holding its initial contents and the lattices not stepped."""
    import test_env_gpu as TE
    torch = torch_mod
    lib = _mod("_lib")
    name, n, B = "c5", 5, 5
    c = _ride_case(name, n, B)
    ff = TE._random_stack(dq, np.random.RandomState(23), c["cfg"]["d"], 4)
    for what in ("per-layer", "dense-stack"):
        spec, net, params, flat, _, _ = TQ._setup(dq, torch, name, B, fused=what != "per-layer")

        def run(a):
            env = _played_env(dq, torch, c, n, **(dict(referee=ff) if what == "dense-stack" else {}))
            try:
                r = _Ride(torch, a, "r", c, net, flat, n, B, True).materialise()
                before = env.export_state().clone()
                r.forward(net)
                q0 = r.t["q0"].clone()
                for call in (lambda: net.td_backward_adam_env(r.t["params"], r.td(), r.t["grads"], r.t["m"], r.t["v"], UPD_T, LR, 0.9, 0.999, 1e-7, env._h,
                                                              r.step(True, True)),
                             lambda: net.td_backward_phase0_env(r.t["params"], r.td(), r.t["grads"], env._h, r.step(True, True))):
                    r.arm(env)
                    with pytest.raises(dq.DeepQError) as ei:
                        call()
                    assert ei.value.status == lib.DQ_ERR_UNSUPPORTED, what
                    env.disarm_patch_output()
                assert torch.equal(r.t["q0"], q0) and torch.equal(env.export_state(), before)
            finally:
                torch.cuda.synchronize()
                env.close()

        out, _ = both_fills(run)
        for key in ("y", "dq", "met", "grads", "legal", "lifetime", "was_reset", "patch", "index_next"):
            assert untouched(out["r_" + key]), (what, key)
        for key, init in (("params", flat), ("m", c["m0"]), ("v", c["v0"]), ("stats", STATS0), ("obs_ring", c["rings"]["obs"]),
                          ("action_ring", c["rings"]["action"]), ("reward_ring", c["rings"]["reward"]), ("term_ring", c["rings"]["term"])):
            assert np.array_equal(out["r_" + key], np.ascontiguousarray(init).reshape(-1).view(np.uint8)), (what, key)
