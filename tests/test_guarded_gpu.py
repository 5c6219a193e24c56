"""Every family of entry points between guard bands (tests/guarded.py): each caller buffer of a case lies in one
allocation as [64 KiB guard | payload | 64 KiB guard], at exactly the alignment include/deepq_hip.h states for it, its ragged end touching
the next guard.  Each case runs with the guards at 0x00 and at 0xFF and shows
  (a) every guard intact, (b) every input unchanged, (c) every output bit-identical between the two runs,
  (d) the outputs equal to the reference the family's own test uses (integers bit for bit, Q-values and gradients under test_qnet_gpu's bounds).
Handles are created at capacity == n, so the last-row paths are the ones that run."""
import ctypes
import functools
import importlib

import numpy as np
import pytest

import guarded as G
import test_qnet_gpu as TQ
from oracle import dqn_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def _mod(name):
    return importlib.import_module("deepq-decoding_amd." + name)


def both_fills(run):
    """run(arena) requests the buffers, takes them and launches; (a) and (b) are checked per run, (c) between the runs.  Returns the
    outputs' bytes of the first run (equal to the second's) and whatever run() returned there."""
    outs, extra = [], []
    for fill in G.FILLS:
        a = G.Arena("cuda", fill)
        extra.append(run(a))
        outs.append(a.verify())
    G.same_bits(outs[0], outs[1])
    return outs[0], extra[0]


def arr(raw, dtype, shape=(-1,)):
    return np.frombuffer(raw.tobytes(), dtype=dtype).reshape(shape)


def untouched(raw):
    return bool((raw == G.OUT_FILL).all())


def _grad_bounds(spec, g, g_ref):
    """test_qnet_gpu.test_training_forward_backward's bounds, as they stand there."""
    scale = np.abs(g_ref).max()
    assert np.abs(g - g_ref).max() < 2e-5 * max(scale, 1.0), (np.abs(g - g_ref).max(), scale)
    for (gk, gb), (rk, rb) in zip(spec.split(g), spec.split(g_ref)):
        for x, y in ((gk, rk), (gb, rb)):
            assert np.abs(x - y).max() <= 1e-4 * np.abs(y).max() + 1e-7


@pytest.mark.parametrize("fill", G.FILLS)
def test_arena_reports_a_stray_byte_on_the_device(torch_mod, fill):
    """The helper's own check on the device the kernels run on (tests/test_guarded_cpu.py has the full set): one changed byte just outside a payload, on
    either side, is named; the write lands inside the arena's own allocation."""
    torch = torch_mod
    for name, pos_of, side in (("q", lambda s, e: s - 1, "low"), ("cls", lambda s, e: e, "high")):
        a = G.Arena("cuda", fill)
        a.request("q", (5, 19), torch.float32, 4)
        a.request("cls", (7,), torch.uint8, 1)
        a.take("q").zero_()
        a.verify()
        lo, s, e, hi = a.span(name)
        a.raw()[pos_of(s, e)] = fill ^ 0x80
        with pytest.raises(AssertionError, match=f"'{name}' changed on its {side} side"):
            a.verify()


# ---- Q-network ------------------------------------------------------------------------------------------------------------------------
FWD_CASES = [("c1", 1), ("c1", 37), ("c3", 33), ("c5", 17), ("c3y", 5), ("d3dp", 3)]


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "per-layer"])
@pytest.mark.parametrize("name,batch", FWD_CASES)
def test_forward_inference(dq, torch_mod, name, batch, fused):
    torch = torch_mod
    spec, net, params, flat, obs, _ = TQ._setup(dq, torch, name, batch, fused=fused)
    A = spec.n_actions

    def run(a):
        a.request("params", (net.n_params,), torch.float32, 16, init=flat)
        a.request("obs", obs.shape, torch.uint8, 1, init=obs)       # the header allows any byte offset
        a.request("q", (batch, A), torch.float32, 4)
        net.forward(a.take("params"), a.take("obs"), out=a.take("q"))

    out, _ = both_fills(run)
    q_ref, _ = O.forward(spec, flat, obs)
    assert np.abs(arr(out["q"], np.float32, (batch, A)) - q_ref).max() < TQ.tol(q_ref)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "per-layer"])
def test_forward_with_replay_gather(dq, torch_mod, fused):
    """A ring of 7 rows read through index_dev with index_off = 5, index_mod = 7: the wrap is taken, the last row is the ring's last."""
    torch = torch_mod
    B = 33
    spec, net, params, flat, obs, rng = TQ._setup(dq, torch, "c3", B, fused=fused)
    ring = (rng.rand(7, *TQ.SHAPES["c3"][0]) < 0.3).astype(np.uint8)
    idx = (np.arange(B) % 7).astype(np.int32)
    rng.shuffle(idx)
    A = spec.n_actions

    def run(a):
        a.request("params", (net.n_params,), torch.float32, 16, init=flat)
        a.request("ring", ring.shape, torch.uint8, 1, init=ring)
        a.request("index", (B,), torch.int32, 4, init=idx)
        a.request("q", (B, A), torch.float32, 4)
        net.forward(a.take("params"), a.take("ring"), index=a.take("index"), index_off=5, index_mod=7, out=a.take("q"))

    out, _ = both_fills(run)
    q_ref = O.forward(spec, flat, ring[(idx + 5) % 7])[0]
    assert set(((idx + 5) % 7).tolist()) == set(range(7))
    assert np.abs(arr(out["q"], np.float32, (B, A)) - q_ref).max() < TQ.tol(q_ref)


def test_forward_from_patch_words(dq, torch_mod):
    """c3, 33 samples, observation rows of 32 patch words at exactly 16-byte alignment, with a caller-provided pack of exactly packed_bytes."""
    torch = torch_mod
    import test_compact_gpu as TC
    B = 33
    spec, net, params, flat, obs, patch, rng = TC._setup(dq, torch, "c3", B)
    words = patch.cpu().numpy()
    A = spec.n_actions

    def run(a):
        a.request("params", (net.n_params,), torch.float32, 16, init=flat)
        a.request("patch", words.shape, torch.int32, 16, init=words)
        a.request("packed", (net.packed_bytes,), torch.uint8, 16)
        a.request("q", (B, A), torch.float32, 4)
        pk = net.pack(a.take("params"), out=a.take("packed"))
        net.forward_multi([dict(params=a.take("params"), obs=a.take("patch"), patch=True, packed=pk, out=a.take("q"))])

    out, _ = both_fills(run)
    q_ref, _ = O.forward(spec, flat, obs)
    assert np.abs(arr(out["q"], np.float32, (B, A)) - q_ref).max() < TC.tol(q_ref)


def test_pack_writes_exactly_packed_bytes(dq, torch_mod):
    """pack(out=) into exactly packed_bytes; the pack equals an ordinary tensor's bit for bit and drives the same forward."""
    torch = torch_mod
    spec, net, params, flat, obs, _ = TQ._setup(dq, torch, "c3", 33)
    # (sections of the pack that this configuration does not use -- the patch-word kernels of a handle without set_patch_input -- are left alone: both
    # buffers start from the arena's output fill)
    want = net.pack(params, out=torch.full((net.packed_bytes,), G.OUT_FILL, dtype=torch.uint8, device="cuda")).cpu().numpy()
    q_want = net.forward(params, torch.from_numpy(obs).cuda(), packed=net.pack(params)).cpu().numpy()

    def run(a):
        a.request("params", (net.n_params,), torch.float32, 16, init=flat)
        a.request("obs", obs.shape, torch.uint8, 1, init=obs)
        a.request("packed", (net.packed_bytes,), torch.uint8, 16)
        a.request("q", (33, spec.n_actions), torch.float32, 4)
        pk = net.pack(a.take("params"), out=a.take("packed"))
        net.forward(a.take("params"), a.take("obs"), packed=pk, out=a.take("q"))

    out, _ = both_fills(run)
    assert np.array_equal(out["packed"], want)
    assert np.array_equal(arr(out["q"], np.float32, q_want.shape), q_want)


def test_alignment_requirements_are_refused_before_any_launch(dq, torch_mod):
    """include/deepq_hip.h: params_dev (fused chains) and packed_dev are 16-byte aligned; less is DQ_ERR_INVALID and nothing is written."""
    torch = torch_mod
    lib = _mod("_lib")
    spec, net, params, flat, obs, _ = TQ._setup(dq, torch, "c3", 5)
    a = G.Arena("cuda", 0x00)
    a.request("params4", (net.n_params,), torch.float32, 4, init=flat)
    a.request("params", (net.n_params,), torch.float32, 16, init=flat)
    a.request("obs", obs.shape, torch.uint8, 1, init=obs)
    a.request("packed8", (net.packed_bytes,), torch.uint8, 8)
    a.request("packed", (net.packed_bytes,), torch.uint8, 16)
    a.request("q", (5, spec.n_actions), torch.float32, 4)
    a.request("dq", (5, spec.n_actions), torch.float32, 4, init=np.zeros((5, spec.n_actions), np.float32))
    a.request("grads", (net.n_params,), torch.float32, 4)
    calls = [lambda: net.forward(a.take("params4"), a.take("obs"), out=a.take("q")),
             lambda: net.pack(a.take("params"), out=a.take("packed8")),
             lambda: net.forward(a.take("params"), a.take("obs"), packed=a.take("packed8"), out=a.take("q"))]
    for call in calls:
        with pytest.raises(dq.DeepQError) as ei:
            call()
        assert ei.value.status == lib.DQ_ERR_INVALID and "16-byte aligned" in str(ei.value)
    # the backward of a training forward (run on aligned parameters) refuses misaligned ones too
    net.forward(a.take("params"), a.take("obs"), training=True, seed=(1, 2), t=3, out=a.take("q"))
    with pytest.raises(dq.DeepQError) as ei:
        net.backward(a.take("params4"), a.take("dq"), grads=a.take("grads"))
    assert ei.value.status == lib.DQ_ERR_INVALID
    out = a.verify()
    assert untouched(out["packed8"]) and untouched(out["packed"]) and untouched(out["grads"])


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "per-layer"])
@pytest.mark.parametrize("name,batch", [("c1", 8), ("c3", 33)])
def test_training_forward_backward(dq, torch_mod, name, batch, fused):
    torch = torch_mod
    spec, net, params, flat, obs, rng = TQ._setup(dq, torch, name, batch, fused=fused)
    A = spec.n_actions
    seed, t, base = (3, 4), 12345678901, 77
    dq_ = (rng.randn(batch, A) / batch).astype(np.float32)

    def run(a):
        a.request("params", (net.n_params,), torch.float32, 16, init=flat)
        a.request("obs", obs.shape, torch.uint8, 1, init=obs)
        a.request("q", (batch, A), torch.float32, 4)
        a.request("dq", (batch, A), torch.float32, 4, init=dq_)
        a.request("grads", (net.n_params,), torch.float32, 4)
        net.forward(a.take("params"), a.take("obs"), training=True, seed=seed, t=t, sample_base=base, out=a.take("q"))
        net.backward(a.take("params"), a.take("dq"), grads=a.take("grads"))

    out, _ = both_fills(run)
    keep = O.dropout_keep_mask(seed, t, base + np.arange(batch), 512, 0.2)
    q_ref, cache = O.forward(spec, flat, obs, training=True, keep_masks=[keep])
    assert np.abs(arr(out["q"], np.float32, (batch, A)) - q_ref).max() < TQ.tol(q_ref)
    _grad_bounds(spec, arr(out["grads"], np.float32), O.backward(spec, flat, cache, dq_.astype(np.float64)))


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "per-layer"])
def test_backward_adam(dq, torch_mod, fused):
    """dq_qnet_backward_adam with params, m, v and the gradient in the arena: the bits of backward + adam_step on ordinary tensors
    (test_qnet_gpu.test_backward_adam_equals_backward_then_adam's reference), with the moments and the gradient 16-byte aligned (the final
    reduction's 16-byte form) and 4-byte-only aligned (its scalar form)."""
    torch = torch_mod
    Q = _mod("qnet")
    B = 33
    spec, net, params, flat, obs, rng = TQ._setup(dq, torch, "c3", B, fused=fused)
    obs_t = torch.from_numpy(obs).cuda()
    dq_np = (rng.randn(B, spec.n_actions) / B).astype(np.float32)
    dq_t = torch.from_numpy(dq_np).cuda()
    m0, v0 = (rng.rand(net.n_params) * 1e-3).astype(np.float32), (rng.rand(net.n_params) * 1e-6).astype(np.float32)
    pb, mb, vb = params.clone(), torch.from_numpy(m0).cuda(), torch.from_numpy(v0).cuda()
    net.forward(pb, obs_t, training=True, seed=(1, 2), t=2)
    gb = net.backward(pb, dq_t)
    Q.adam_step(pb, gb, mb, vb, 2, 1e-3)
    want = dict(params=pb, m=mb, v=vb, grads=gb)
    assert not torch.equal(pb, params)
    for align in (16, 4):

        def run(a):
            # (the fused chains need 16-byte parameters: include/deepq_hip.h; the per-layer path takes them at 4)
            a.request("params", (net.n_params,), torch.float32, 16 if fused else align)
            a.request("obs", obs.shape, torch.uint8, 1, init=obs)
            a.request("dq", dq_np.shape, torch.float32, 4, init=dq_np)
            a.request("m", (net.n_params,), torch.float32, align)
            a.request("v", (net.n_params,), torch.float32, align)
            a.request("grads", (net.n_params,), torch.float32, align)
            p, m, v = a.take("params"), a.take("m"), a.take("v")
            p.copy_(params); m.copy_(torch.from_numpy(m0)); v.copy_(torch.from_numpy(v0))
            net.forward(p, a.take("obs"), training=True, seed=(1, 2), t=2)
            net.backward_adam(p, a.take("dq"), a.take("grads"), m, v, 2, 1e-3)

        out, _ = both_fills(run)
        for k, w in want.items():
            assert np.array_equal(arr(out[k], np.float32), w.cpu().numpy()), (k, align)


@pytest.mark.parametrize("n", ["n_params", 10007, 3, 1])
def test_adam_step(dq, torch_mod, n):
    """dq_adam_step on exactly n elements: the float4 path (16-byte aligned buffers) and the scalar path (4-byte-only aligned ones) give the
    same bits, within test_qnet_gpu.test_td_target_loss_adam's bound of the float64 oracle; 10007 and 3 have n % 4 == 3."""
    torch = torch_mod
    Q = _mod("qnet")
    if n == "n_params":
        n = O.QNetSpec(TQ.SHAPES["c1"][0], TQ.C_LAYERS, TQ.FF_LAYERS, TQ.SHAPES["c1"][1], dueling=True).n_params
    rng = np.random.RandomState(9)
    p0, g0 = rng.randn(n).astype(np.float32), rng.randn(n).astype(np.float32)
    res = {}
    for align in (16, 4):

        def run(a):
            a.request("p", (n,), torch.float32, align)
            a.request("g", (n,), torch.float32, align, init=g0)
            a.request("m", (n,), torch.float32, align)
            a.request("v", (n,), torch.float32, align)
            p, m, v = a.take("p"), a.take("m"), a.take("v")
            p.copy_(torch.from_numpy(p0)); m.zero_(); v.zero_()
            for t in (1, 2, 3):
                Q.adam_step(p, a.take("g"), m, v, t, 1e-3)

        res[align], _ = both_fills(run)
    G.same_bits(res[16], res[4])
    pr, mr, vr = p0.astype(np.float64), np.zeros(n), np.zeros(n)
    for t in (1, 2, 3):
        pr, mr, vr = O.adam_step(pr, g0.astype(np.float64), mr, vr, t, 1e-3)
    for k, ref in (("p", pr), ("m", mr), ("v", vr)):
        assert np.abs(arr(res[4][k], np.float32) - ref).max() < 1e-6


# ---- TD and replay kernels -------------------------------------------------------------------------------------------------------------
def _td_data(B, A=19, R=40):
    rng = np.random.RandomState(9 + B)
    q1o, q1t, q0 = (rng.randn(B, A).astype(np.float32) for _ in range(3))
    q1o[B - 1, 3] = q1o[B - 1, 9] = q1o[B - 1].max() + 1.0         # a tie in the last row -> first maximum
    reward = (rng.rand(R) < 0.4).astype(np.float32)
    terminal = (rng.rand(R) < 0.2).astype(np.uint8)
    action = rng.randint(0, A, size=R).astype(np.int32)
    action[R - 1] = A - 1
    idx = rng.randint(0, R, size=B).astype(np.int32)
    idx[B - 1] = R - 1                                              # the last sample reads the rings' last row, its action is the last column
    return q1o, q1t, q0, reward, terminal, action, idx


@pytest.mark.parametrize("B", [5, 33])
def test_td_kernels(dq, torch_mod, B):
    """dq_td_target, dq_td_loss_grad, dq_td_loss_grad_clip, dq_td_update and dq_td_metrics at A = 19: references as in
    test_qnet_gpu.test_td_target_loss_adam and test_huber_gpu.test_per_layer_td_kernels_apply_the_huber_clamp_and_loss; metrics take exactly
    DQ_TD_METRICS_FLOATS floats, of which only [0], [1] and the partials of this batch's blocks are written."""
    torch = torch_mod
    Q = _mod("qnet")
    import test_huber_gpu as TH
    A, R, gamma, gs, delta = 19, 40, 0.99, 0.01, 0.5
    q1o, q1t, q0, reward, terminal, action, idx = _td_data(B, A, R)
    f32, MF = torch.float32, Q.TD_METRICS_FLOATS

    def run(a):
        for k, v in (("q1o", q1o), ("q1t", q1t), ("q0", q0), ("reward", reward)):
            a.request(k, v.shape, f32, 4, init=v)
        a.request("terminal", (R,), torch.uint8, 1, init=terminal)
        a.request("action", (R,), torch.int32, 4, init=action)
        a.request("index", (B,), torch.int32, 4, init=idx)
        for k in ("y", "y_upd"):
            a.request(k, (B,), f32, 4)
        for k in ("dq", "dq_clip", "dq_upd", "dq_step"):
            a.request(k, (B, A), f32, 4)
        for k in ("met", "met_clip", "met_upd", "met_step"):
            a.request(k, (MF,), f32, 4)
        t = a.take
        y = Q.td_target(t("q1o"), t("q1t"), t("reward"), t("terminal"), gamma, index=t("index"), out=t("y"))
        Q.td_loss_grad(t("q0"), t("action"), y, grad_scale=gs, index=t("index"), dq=t("dq"), metrics=t("met"))
        Q.td_loss_grad(t("q0"), t("action"), y, grad_scale=gs, index=t("index"), dq=t("dq_clip"), metrics=t("met_clip"), delta_clip=delta)
        Q.td_update(t("q1o"), t("q1t"), t("q0"), t("reward"), t("terminal"), t("action"), gamma, grad_scale=gs, index=t("index"), y=t("y_upd"),
                    dq=t("dq_upd"), metrics=t("met_upd"))
        Q.td_metrics(t("met_upd"), B)
        Q.td_update(t("q1o"), t("q1t"), t("q0"), t("reward"), t("terminal"), t("action"), gamma, grad_scale=gs, index=t("index"),
                    dq=t("dq_step"), metrics=t("met_step"), delta_clip=delta)
        Q.td_metrics(t("met_step"), B)

    out, _ = both_fills(run)
    y = arr(out["y"], np.float32)
    y_ref = O.td_targets(q1o.astype(np.float64), q1t.astype(np.float64), reward[idx], terminal[idx], gamma)
    assert np.abs(y - y_ref).max() < TQ.tol(y_ref)
    loss_ref, mq_ref, dq_ref = O.loss_and_grad(q0.astype(np.float64), action[idx], y.astype(np.float64))
    met = arr(out["met"], np.float32)
    assert abs(met[0] - loss_ref) < TQ.tol(loss_ref) and abs(met[1] - mq_ref) < TQ.tol(mq_ref)
    assert np.abs(arr(out["dq"], np.float32, (B, A)) - dq_ref * (gs * B)).max() < 1e-7        # (the oracle's dq carries 1 / B)
    # the fused launch: the separate kernels' bits
    assert np.array_equal(out["y_upd"], out["y"]) and np.array_equal(out["dq_upd"], out["dq"])
    assert np.array_equal(arr(out["met_upd"], np.float32)[:2], met[:2])
    # Huber at delta: float32 restatement, bit for bit
    a_b = action[idx]
    diff32 = q0[np.arange(B), a_b] - y
    assert 0 < (np.abs(diff32) > np.float32(delta)).sum() < B
    dqc = np.zeros((B, A), np.float32)
    dqc[np.arange(B), a_b] = TH.huber_c32(diff32, delta) * np.float32(gs)
    lossc = float(np.mean(TH.huber_h(diff32.astype(np.float64), delta)))
    for k, mk in (("dq_clip", "met_clip"), ("dq_step", "met_step")):
        assert np.array_equal(arr(out[k], np.float32, (B, A)), dqc), k
        assert abs(float(arr(out[mk], np.float32)[0]) - lossc) <= 1e-6 * lossc
    # the scratch part of metrics: two floats per block of four samples, the rest left alone
    used = 2 + 2 * ((B + 3) // 4)
    for mk in ("met", "met_clip", "met_upd", "met_step"):
        assert untouched(out[mk][4 * used:]), mk


@pytest.mark.parametrize("batch", [5, 33])
def test_replay_sample_post_step_and_episode_stats(dq, torch_mod, batch):
    """dq_replay_sample, dq_post_step and dq_episode_stats on n = 5 lattices; the ring's terminal flags take exactly n_slots * n_envs bytes.
    References: oracle/memory_oracle.py device_replay_rows and a direct count (test_qnet_gpu's)."""
    torch = torch_mod
    Q, lib = _mod("qnet"), _mod("_lib")
    from oracle import memory_oracle as M
    rng = np.random.RandomState(4)
    n_envs, n_slots, head, filled = 5, 9, 3, 9                      # a full ring whose candidate slots wrap below slot 0
    term = (rng.rand(n_slots, n_envs) < 0.15).astype(np.uint8)
    done, was_reset = (rng.rand(n_envs) < 0.6).astype(np.uint8), np.array([0, 0, 1, 0, 0], np.uint8)
    done[4], done[2] = 1, 1
    life, rew = rng.randint(1, 100, size=n_envs).astype(np.int32), np.array([1, 0, 1, 0, 1], np.float32)
    seed, t, base = (8, 9), 55, 1000
    L, p = lib.lib(), lib.ptr

    def run(a):
        a.request("term", term.shape, torch.uint8, 1, init=term)
        a.request("done", (n_envs,), torch.uint8, 1, init=done)
        a.request("was_reset", (n_envs,), torch.uint8, 1, init=was_reset)
        a.request("life", (n_envs,), torch.int32, 4, init=life)
        a.request("rew", (n_envs,), torch.float32, 4, init=rew)
        a.request("index", (batch,), torch.int32, 4)
        a.request("index_post", (batch,), torch.int32, 4)
        a.request("stats", (4,), torch.int64, 8)
        a.request("stats_post", (4,), torch.int64, 8)
        k = a.take
        k("stats").zero_(); k("stats_post").zero_()
        Q.replay_sample(k("term"), n_envs, n_slots, head, filled, batch, seed, t, sample_base=base, out=k("index"))
        lib.check(L.dq_episode_stats(p(k("done")), p(k("was_reset")), p(k("life")), p(k("rew")), n_envs, p(k("stats")), lib.current_stream()))
        lib.check(L.dq_post_step(p(k("term")), n_envs, n_slots, head, filled, batch, Q._seed_arr(seed), t, base, p(k("index_post")), p(k("done")),
                                 p(k("was_reset")), p(k("life")), p(k("rew")), n_envs, p(k("stats_post")), lib.current_stream()))

    out, _ = both_fills(run)
    want = M.device_replay_rows(term, n_envs, n_slots, head, filled, batch, seed, t, sample_base=base)
    assert np.array_equal(arr(out["index"], np.int32), want) and np.array_equal(out["index_post"], out["index"])
    ended = (done != 0) & (was_reset == 0)
    stats_ref = [int(ended.sum()), int(life[ended].sum()), int(((rew == 1.0) & (was_reset == 0)).sum()), int((was_reset == 0).sum())]
    assert arr(out["stats"], np.int64).tolist() == arr(out["stats_post"], np.int64).tolist()
    assert arr(out["stats"], np.int64).tolist() == stats_ref


# ---- narrow environment ----------------------------------------------------------------------------------------------------------------
ENV_SEED = (0x5EED, 0xD0DEC0DE)
NARROW = {"d3dp": dict(d=3, error_model="DP", use_Y=False, volume_depth=3, p_phys=0.01, p_meas=0.01),       # two lattices per wave
          "c3": dict(d=5, error_model="DP", use_Y=False, volume_depth=5, p_phys=0.011, p_meas=0.011),        # two lattices per wave
          "c5": dict(d=7, error_model="DP", use_Y=False, volume_depth=7, p_phys=0.005, p_meas=0.005)}        # one lattice per wave


def _env_views(env, a, torch, obs_align, patch=True, q=None):
    """The wrapper's own output tensors become views into the arena (every pointer a launch receives is then guarded)."""
    n = env.n_envs
    a.request("obs", (n,) + tuple(env.obs_shape), torch.uint8, obs_align)
    a.request("reward", (n,), torch.float32, 4)
    a.request("done", (n,), torch.uint8, 1)
    a.request("legal", (n, env.legal_words), torch.int64, 8)
    a.request("lifetime", (n,), torch.int32, 4)
    a.request("was_reset", (n,), torch.uint8, 1)
    a.request("action", (n,), torch.int32, 4)
    if env.wide:
        a.request("inexact", (n,), torch.uint8, 1)
    if patch:
        a.request("patch", (n, env.patch_stride), torch.int32, 4)
    if q is not None:
        a.request("q", q.shape, torch.float32, 4, init=q)
    for k in ("obs", "reward", "done", "legal", "lifetime", "was_reset") + (("inexact",) if env.wide else ()):
        setattr(env, k, a.take(k))
    a.take("done").zero_()


def _same_as_oracle(env, ref, a, what, patch=True):
    assert np.array_equal(env.obs.cpu().numpy(), ref.obs), (what, "obs")
    assert np.array_equal(env.reward.cpu().numpy(), ref.reward), (what, "reward")
    assert np.array_equal(env.done.cpu().numpy(), ref.done), (what, "done")
    assert np.array_equal(env.lifetime.cpu().numpy().view(np.uint32), ref.lifetime), (what, "lifetime")
    assert np.array_equal(env.legal.cpu().numpy().view(np.uint64), ref.legal), (what, "legal")
    assert np.array_equal(env.was_reset.cpu().numpy(), ref.was_reset), (what, "was_reset")
    if patch:
        words, d2 = a.take("patch"), env.d * env.d
        assert np.array_equal(env.patch_to_obs(words).cpu().numpy(), ref.obs), (what, "patch")
        assert bool((words[:, d2:] == 0x77777777).all()), (what, "the words between d * d and the stride are left alone")


@pytest.mark.parametrize("obs_align", [1, 16])
@pytest.mark.parametrize("n_envs", [5, 33])
@pytest.mark.parametrize("name", ["d3dp", "c3", "c5"])
def test_narrow_step_and_act_step(dq, torch_mod, name, n_envs, obs_align):
    """reset, select_actions(out=) + step and act_step with out_obs / out_patch / out_action in the arena, 8 steps with auto-reset, against the C
    oracle after every launch (test_env_gpu.test_full_size_vs_c_oracle's comparison).  The observation store has a 16-byte, a 4-byte and a byte
    form chosen per workgroup from the address: obs_align 1 and 16 run all of them."""
    from oracle import c_oracle
    torch = torch_mod
    cfg, base = NARROW[name], 4096 * 3
    events = {}

    def run(a):
        env = dq.VectorEnv(n_envs=n_envs, seed=ENV_SEED, env_id_base=base, **cfg)
        ref = c_oracle.COracleEnv(n_envs=n_envs, seed=ENV_SEED, env_id_base=base, **cfg)
        _env_views(env, a, torch, obs_align)
        obs, patch, action = a.take("obs"), a.take("patch"), a.take("action")
        env.reset(out_obs=obs, out_patch=patch)
        ref.reset()
        assert np.array_equal(obs.cpu().numpy(), ref.obs) and np.array_equal(env.legal.cpu().numpy().view(np.uint64), ref.legal)
        ev = dict(done=0, reset=0)
        for t in range(8):
            a_ref = ref.policy_uniform_legal(t)
            if t % 2 == 0:
                env.select_actions(t, out=action)
                env.step(action, auto_reset=True, out_obs=obs, out_patch=patch)
            else:
                env.act_step(t, out_obs=obs, out_action=action, out_patch=patch)
            assert np.array_equal(action.cpu().numpy(), a_ref), (name, "action", t)
            ref.step(a_ref, auto_reset=True)
            _same_as_oracle(env, ref, a, (name, t))
            ev["done"] += int(ref.done.sum()); ev["reset"] += int(ref.was_reset.sum())
        events.update(ev)
        torch.cuda.synchronize()
        env.close()

    both_fills(run)
    if n_envs == 33:
        assert events["done"] >= 1 and events["reset"] >= 1, events


@pytest.mark.parametrize("rings", ["all", "actions"])
@pytest.mark.parametrize("n_envs", [5, 33])
@pytest.mark.parametrize("name", ["d3dp", "c3", "c5"])
def test_narrow_act_steps_rings(dq, torch_mod, name, n_envs, rings):
    """act_steps over 4 steps into rings of n_slots = 3 from slot0 = 2: the slot number wraps inside the launch (d <= 5: one launch; d = 7: four).
    With every ring, and with the action ring alone.  Every surviving ring entry against the C oracle, as test_env_gpu.test_act_steps_entry_vs_c_oracle."""
    from oracle import c_oracle
    torch = torch_mod
    cfg, base, T, slot0, k = NARROW[name], 4096 * 3, 3, 2, 4

    def run(a):
        env = dq.VectorEnv(n_envs=n_envs, seed=ENV_SEED, env_id_base=base, **cfg)
        ref = c_oracle.COracleEnv(n_envs=n_envs, seed=ENV_SEED, env_id_base=base, **cfg)
        a.request("action_ring", (T, n_envs), torch.int32, 4)
        if rings == "all":
            a.request("reward_ring", (T, n_envs), torch.float32, 4)
            a.request("done_ring", (T, n_envs), torch.uint8, 1)
            a.request("obs_ring", (T, n_envs) + tuple(env.obs_shape), torch.uint8, 1)
            a.request("patch_ring", (T, n_envs, env.patch_stride), torch.int32, 4)
        _env_views(env, a, torch, 1, patch=False)
        env.reset(out_obs=a.take("obs"))
        ref.reset()
        g = (lambda key: a.take(key)) if rings == "all" else (lambda key: None)
        env.act_steps(k, 0, a.take("action_ring"), g("reward_ring"), g("done_ring"), obs_ring=g("obs_ring"), patch_ring=g("patch_ring"), slot0=slot0)
        host = {key: a.take(key).cpu().numpy() for key in (("action_ring", "reward_ring", "done_ring", "obs_ring") if rings == "all" else ("action_ring",))}
        for s in range(k):
            a_ref = ref.policy_uniform_legal(s)
            ref.step(a_ref, auto_reset=True)
            c, nx = (slot0 + s) % T, (slot0 + s + 1) % T
            if k - s <= T - 1:                  # (a launch longer than the ring overwrites its own oldest slots)
                assert np.array_equal(host["action_ring"][c], a_ref), (name, "action", s)
                if rings == "all":
                    assert np.array_equal(host["reward_ring"][c], ref.reward) and np.array_equal(host["done_ring"][c], ref.done), (name, s)
                    assert np.array_equal(host["obs_ring"][nx], ref.obs), (name, "obs", s)
                    words = a.take("patch_ring")[nx]
                    assert np.array_equal(env.patch_to_obs(words).cpu().numpy(), ref.obs), (name, "patch", s)
        if rings == "all":
            assert bool((a.take("patch_ring")[:, :, env.d * env.d:] == 0x77777777).all())
        assert np.array_equal(env.lifetime.cpu().numpy().view(np.uint32), ref.lifetime)
        assert np.array_equal(env.legal.cpu().numpy().view(np.uint64), ref.legal)
        assert np.array_equal(env.was_reset.cpu().numpy(), ref.was_reset)
        torch.cuda.synchronize()
        env.close()

    both_fills(run)


# ---- wide environment ------------------------------------------------------------------------------------------------------------------
# (rates and first lattice id chosen on the CPU with COracleWideEnv so that the 6 steps of 5 lattices hold a done and an auto-reset)
WIDE = {"d9dp": (dict(d=9, error_model="DP", use_Y=False, volume_depth=3), 0.01, 28),
        "d11dpy": (dict(d=11, error_model="DP", use_Y=True, volume_depth=3), 0.01, 10),
        "d15dpy": (dict(d=15, error_model="DP", use_Y=True, volume_depth=3), 0.015, 5)}


def _wide_q(n, A):
    return np.random.RandomState(17).randn(n, A).astype(np.float32)


def _wide_oracle_events(name, n=5, steps=6):
    """The oracle alone (no GPU): the events of the case's trajectory -- even steps uniform over the legal moves, odd steps epsilon-greedy on q."""
    import test_env_wide_gpu as TW
    from oracle import c_oracle
    cfg, p, base = WIDE[name]
    ref = c_oracle.COracleWideEnv(n_envs=n, seed=TW.SEED, env_id_base=base, p_phys=p, p_meas=p, **cfg)
    ref.reset()
    q = _wide_q(n, (3 if cfg["use_Y"] else 2) * cfg["d"] ** 2 + 1)
    ev = dict(done=0, reset=0)
    for t in range(steps):
        a_ref = ref.policy_uniform_legal(t) if t % 2 == 0 else TW._policy_oracle(q, ref.legal, 0.3, False, t, base)
        ref.step(a_ref, auto_reset=True)
        ev["done"] += int(ref.done.sum()); ev["reset"] += int(ref.was_reset.sum())
    return ev


@pytest.mark.parametrize("name", list(WIDE))
def test_wide_step_act_step_and_policy(dq, torch_mod, name):
    """dq_envb_reset, dq_policy_select_wide + dq_envb_step and dq_envb_act_step (epsilon-greedy on q [n][A]) through _lib, and uf_select_wide(out=),
    with every pointer in the arena, n = 5 (one full workgroup of four lattices and a ragged one), legal [n][LW]; the wide C oracle after every launch
    (test_env_wide_gpu._run's comparison), 6 steps that hold a done and an auto-reset."""
    import test_env_wide_gpu as TW
    import test_wide_env_uf_cpu as TWU
    from oracle import c_oracle
    torch = torch_mod
    lib = _mod("_lib")
    cfg, p, base = WIDE[name]
    n, steps = 5, 6
    ev0 = _wide_oracle_events(name)
    assert ev0["done"] >= 1 and ev0["reset"] >= 1, ev0

    def run(a):
        env = dq.VectorEnv(n_envs=n, seed=TW.SEED, env_id_base=base, backend="wide", p_phys=p, p_meas=p, **cfg)
        ref = c_oracle.COracleWideEnv(n_envs=n, seed=TW.SEED, env_id_base=base, p_phys=p, p_meas=p, **cfg)
        q = _wide_q(n, env.num_actions)
        a.request("uf_action", (n,), torch.int32, 4)
        _env_views(env, a, torch, 1, patch=False, q=q)
        ev = dq.WideEvaluator(env.d, env.error_model, window=env.volume_depth, chunk=n, device=env.device)
        L, P, st = env.L, lib.ptr, lib.current_stream()
        k = a.take
        seed = (ctypes.c_uint32 * 2)(*TW.SEED)
        lib.check(L.dq_envb_reset(env._h, None, P(k("obs")), P(k("legal")), P(k("lifetime")), st))
        ref.reset()
        assert np.array_equal(k("obs").cpu().numpy(), ref.obs) and np.array_equal(k("legal").cpu().numpy().view(np.uint64), ref.legal)
        for t in range(steps):
            if t % 2 == 0:
                a_ref = ref.policy_uniform_legal(t)
                lib.check(L.dq_policy_select_wide(None, P(k("legal")), n, env.num_actions, env.legal_words, 1.0, 0, seed, base, t, P(k("action")), st))
                lib.check(L.dq_envb_step(env._h, P(k("action")), 1, P(k("obs")), P(k("reward")), P(k("done")), P(k("legal")), P(k("lifetime")),
                                         P(k("was_reset")), P(k("inexact")), st))
            else:
                a_ref = TW._policy_oracle(q, ref.legal, 0.3, False, t, base)
                lib.check(L.dq_envb_act_step(env._h, P(k("q")), 0.3, 0, seed, t, P(k("action")), 1, P(k("obs")), P(k("reward")), P(k("done")),
                                             P(k("legal")), P(k("lifetime")), P(k("was_reset")), P(k("inexact")), st))
            assert np.array_equal(k("action").cpu().numpy(), a_ref), (name, "action", t)
            ref.step(a_ref, auto_reset=True)
            _same_as_oracle(env, ref, a, (name, t), patch=False)
            assert np.array_equal(k("inexact").cpu().numpy(), ref.inexact), (name, "inexact", t)
            # the union-find decoder's action for every lattice as it stands now (uf_select_wide(out=); test_wide_env_uf_cpu.rule_action)
            env.uf_select_wide(ev, out=k("uf_action"))
            want = np.array([TWU.rule_action(dq, cfg, rec) for rec in ref.export()], dtype=np.int32)
            assert np.array_equal(k("uf_action").cpu().numpy(), want), (name, "uf_select_wide", t)
        assert np.array_equal(env.export_state().cpu().numpy().view(np.uint64), ref.export_state())
        torch.cuda.synchronize()
        ev.close()
        env.close()

    both_fills(run)


# ---- referees --------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _graphs(d):
    from oracle import matching_referee as M
    return M.ComponentGraph(d, 3), M.ComponentGraph(d, 1)


def _referee_case(d, N):
    """Defects uint64 [N][2][2] of i.i.d. component errors at p = 0.03, the matching referee's (class, inexact) by oracle/matching_referee.py and the
    union-find referee's class by tests/uf_referee_ref.py.  At d = 9 and 11 every cluster has at most 14 defects at this rate and the matching referee
    answers from LDS; at d = 15 some clusters go through its scratch pool and its flagged fallback, which the oracle restates."""
    import uf_referee_ref as U
    from oracle import matching_referee as M
    graphs = _graphs(d)
    defects = U.sample_defects(d, 0.03, 67, 100 * d + 3)[0][67 - N:]      # (the tail of one draw: N = 1 is its last row)
    n = (d * d - 1) // 2
    cls, flag = np.zeros(N, np.uint8), np.zeros(N, np.uint8)
    for i in range(N):
        parts = []
        for comp in (0, 1):
            nodes = [j for j in range(n) if (int(defects[i, comp, j >> 6]) >> (j & 63)) & 1]
            assert d == 15 or max([len(c) for c in graphs[comp].clusters(nodes[:M.MAX_LIST])] or [0]) <= 14
            parts.append(graphs[comp].weights(nodes))
        (wx0, wx1, ex), (wz0, wz1, ez) = parts
        cls[i], flag[i] = int(wx1 < wx0) + 2 * int(wz1 < wz0), int(not (ex and ez))
    return defects, cls, flag, U.classify_words(d, "DP", defects)


@pytest.mark.parametrize("N", [1, 5, 67])
@pytest.mark.parametrize("d", [9, 11, 15])
def test_referees(dq, torch_mod, d, N):
    """dq_match_decode and dq_uf_referee_decode: defects [N][2][2] uint64 at 8-byte alignment, classes and flags of N bytes at any byte offset; both
    components and component 0 alone."""
    torch = torch_mod
    lib = _mod("_lib")
    defects, m_cls, m_flag, u_cls = _referee_case(d, N)
    L = lib.lib()
    hm, hu = ctypes.c_void_p(), ctypes.c_void_p()
    lib.check(L.dq_match_create(d, ctypes.byref(hm)))
    lib.check(L.dq_wide_uf_create(d, lib.DQ_MODEL_DP, 1, N, ctypes.byref(hu)))
    try:
        def run(a):
            a.request("defects", (N, 2, 2), torch.int64, 8, init=defects.view(np.int64))
            for k in ("m_cls", "m_flag", "m_cls0", "u_cls", "u_cls0"):
                a.request(k, (N,), torch.uint8, 1)
            P, st, k = lib.ptr, lib.current_stream(), a.take
            lib.check(L.dq_match_decode(hm, P(k("defects")), N, 1, P(k("m_cls")), P(k("m_flag")), st))
            lib.check(L.dq_match_decode(hm, P(k("defects")), N, 0, P(k("m_cls0")), None, st))
            lib.check(L.dq_uf_referee_decode(hu, P(k("defects")), N, 1, P(k("u_cls")), st))
            lib.check(L.dq_uf_referee_decode(hu, P(k("defects")), N, 0, P(k("u_cls0")), st))

        out, _ = both_fills(run)
    finally:
        L.dq_match_destroy(hm)
        L.dq_wide_uf_destroy(hu)
    assert np.array_equal(out["m_cls"], m_cls) and np.array_equal(out["m_flag"], m_flag) and (d == 15 or not m_flag.any())
    assert np.array_equal(out["m_cls0"], m_cls & 1)
    assert np.array_equal(out["u_cls"], u_cls) and np.array_equal(out["u_cls0"], u_cls & 1)


# ---- wide union-find family ------------------------------------------------------------------------------------------------------------
UF_T, UF_W, UF_C, UF_P = 5, 2, 1, 0.02
UF_SHAPES = [(d, n) for d in (3, 11, 15) for n in (1, 5)]        # 9-, 121- and 225-byte frames; d = 11 runs in no other test of these kernels


@functools.lru_cache(maxsize=None)
def _uf_streams(d, n):
    import decode_eval_ref as V
    return V.sample_volumes(d, "DP", UF_T, n, UF_P, UF_P, ENV_SEED, 50)


def _uf_weight_rows(n, cols):
    rows = np.array([[3, 2, 1], [1, 1, 1], [4, 4, 2], [2, 5, 1], [6, 3, 3]], dtype=np.uint8)[:n, :cols]
    return np.ascontiguousarray(rows)


def _uf_reference(mode, d, syn, closed, n):
    import closed_uf_ref as C
    import correlated_uf_ref as CU
    import weighted_uf_ref as WU
    import wide_uf_ref as W
    if mode == "unit":
        return (C.decode(d, syn, UF_W, UF_C, True) if closed else W.decode(d, syn, UF_W, UF_C))[:4]
    if mode == "pair":
        return WU.decode(d, syn, UF_W, UF_C, closed, (3, 2))[:4]
    if mode == "triple":
        return CU.decode(d, syn, UF_W, UF_C, closed, (4, 4, 1))[:4]
    if mode == "pairs":
        return WU.decode(d, syn, UF_W, UF_C, closed, _uf_weight_rows(n, 2).astype(np.int64))[:4]
    return CU.decode(d, syn, UF_W, UF_C, closed, _uf_weight_rows(n, 3).astype(np.int64))[:4]


@pytest.mark.parametrize("mode", ["unit", "pair", "triple", "pairs", "triples"])
@pytest.mark.parametrize("d,n", UF_SHAPES)
def test_wide_uf_decode_into(dq, torch_mod, d, n, mode):
    """WideEvaluator(chunk = n).decode_into in every mode -- unit weights, weights = (3, 2), correlated (4, 4, 1), per-stream uint8 [n][2] and [n][3] at any
    byte offset --, each with the final round faulty and perfect; T = 5, window 2, commit 1.  Syndromes, frame, weight, n_defects and rounds in the arena."""
    torch = torch_mod
    DW = _mod("decoder_wide")
    syn = _uf_streams(d, n)[0]
    ev = DW.WideEvaluator(d, "DP", window=UF_W, chunk=n)
    try:
        def run(a):
            a.request("syn", syn.shape, torch.uint8, 1, init=syn)
            if mode in ("pairs", "triples"):
                rows = _uf_weight_rows(n, 2 if mode == "pairs" else 3)
                a.request("each", rows.shape, torch.uint8, 1, init=rows)
            for fr in ("faulty", "perfect"):
                a.request("frame_" + fr, (n, d, d), torch.uint8, 1)
                for k in ("weight_", "ndef_", "rounds_"):
                    a.request(k + fr, (n, 2), torch.int32, 4)
            weights = {"unit": None, "pair": (3, 2), "triple": (4, 4, 1)}[mode] if mode in ("unit", "pair", "triple") else a.take("each")
            for fr in ("faulty", "perfect"):
                ev.decode_into(a.take("syn"), n, UF_T, UF_C, a.take("frame_" + fr), a.take("weight_" + fr), a.take("ndef_" + fr), a.take("rounds_" + fr),
                               final_round=fr, weights=weights)

        out, _ = both_fills(run)
    finally:
        ev.close()
    for fr in ("faulty", "perfect"):
        frame, weight, ndef, rounds = _uf_reference(mode, d, syn, fr == "perfect", n)
        assert np.array_equal(arr(out["frame_" + fr], np.uint8, (n, d, d)), frame), (mode, fr, "frame")
        for k, want in (("weight_", weight), ("ndef_", ndef), ("rounds_", rounds)):
            assert np.array_equal(arr(out[k + fr], np.int32, (n, 2)), want), (mode, fr, k)
    assert syn.any()


@pytest.mark.parametrize("d,n", UF_SHAPES)
def test_wide_uf_run_into_and_verdict_into(dq, torch_mod, d, n):
    """run_into with per-stream rates and the syndromes output, then verdict_into of the sampled errors with and without the frame, unrefereed and with
    referee = "matching" (its inexact flags in the arena) and "uf".  References: decode_eval_ref.sample_volumes, wide_uf_ref, verdict_wide_ref, uf_referee_ref."""
    torch = torch_mod
    DW = _mod("decoder_wide")
    import decode_eval_ref as V
    import uf_referee_ref as U
    import verdict_wide_ref as VW
    import wide_uf_ref as W
    ph = np.ascontiguousarray(np.linspace(0.01, 0.03, n))
    pm = np.ascontiguousarray(np.linspace(0.02, 0.005, n))
    base = 2 ** 32 - 2                                              # the lattice ids wrap
    ev = DW.WideEvaluator(d, "DP", window=UF_W, chunk=n)
    kinds = [(r, f) for r in (None, "matching", "uf") for f in (True, False)]
    try:
        def run(a):
            a.request("hidden", (n, d, d), torch.uint8, 1)
            a.request("trivial", (n,), torch.uint8, 1)
            a.request("frame", (n, d, d), torch.uint8, 1)
            for k in ("weight", "ndef", "rounds"):
                a.request(k, (n, 2), torch.int32, 4)
            a.request("syn", (n, UF_T, d + 1, d + 1), torch.uint8, 1)
            for r, f in kinds:
                a.request(f"verdict_{r}_{f}", (n,), torch.uint8, 1)
                if r == "matching":
                    a.request(f"inexact_{f}", (n,), torch.uint8, 1)
            k = a.take
            ev.run_into(n, UF_T, UF_C, base, ENV_SEED, ph, pm, k("hidden"), k("trivial"), k("frame"), k("weight"), k("ndef"), k("rounds"), syndromes=k("syn"))
            for r, f in kinds:
                ev.verdict_into(k("hidden"), k("frame") if f else None, n, k(f"verdict_{r}_{f}"), referee=r,
                                inexact=k(f"inexact_{f}") if r == "matching" else None)

        out, _ = both_fills(run)
    finally:
        ev.close()
    syn, hid, triv = V.sample_volumes(d, "DP", UF_T, n, ph, pm, ENV_SEED, base)
    frame, weight, ndef, rounds = W.decode(d, syn, UF_W, UF_C)[:4]
    assert np.array_equal(arr(out["syn"], np.uint8, syn.shape), syn) and np.array_equal(arr(out["hidden"], np.uint8, hid.shape), hid)
    assert np.array_equal(out["trivial"], triv) and np.array_equal(arr(out["frame"], np.uint8, frame.shape), frame)
    for key, want in (("weight", weight), ("ndef", ndef), ("rounds", rounds)):
        assert np.array_equal(arr(out[key], np.int32, (n, 2)), want), key
    for r, f in kinds:
        fr = frame if f else None
        if r is None:
            want = V.verdict(d, hid, fr, W.classify_none)
        elif r == "matching":
            res = VW.restatement(d, "DP").verdict(hid, fr)
            want = res["byte"]
            assert np.array_equal(out[f"inexact_{f}"], res["inexact"]), (r, f)
        else:
            want = U.restatement(d, "DP").verdict(hid, fr)["byte"]
        assert np.array_equal(out[f"verdict_{r}_{f}"], want), (r, f)


# ---- narrow decode and evaluation (d = 5 DP) ---------------------------------------------------------------------------------------------
DEC_P, DEC_FAMILY = 0.009, "d5_dp"


def _lut_env(dq):
    import shipped
    return dq.VectorEnv(n_envs=1, p_phys=DEC_P, p_meas=DEC_P, seed=ENV_SEED, **shipped.CONFIGS[DEC_FAMILY])


@pytest.mark.parametrize("n", [5, 67])
def test_narrow_sample_run_verdict_count(dq, torch_mod, n):
    """dq_decode_sample -> dq_decode_run (the shipped d = 5 DP agent, masked greedy, uint8 observations) -> dq_decode_verdict (with and without the frame) ->
    dq_decode_count into counters of exactly n_blocks rows, every array in the arena: volumes 4-byte aligned, counters 8, corrections [n][max_actions],
    n_corr, frame and status.  References: decode_eval_ref (sampler, verdict), decode_ref.decode_volume on the float64 oracle's Q-values (equal action
    lists, or a near-tie of the oracle at the first difference: test_decode_gpu's rule), decoder.counters_from_arrays."""
    torch = torch_mod
    import decode_eval_ref as V
    import decode_ref as R
    import shipped
    import test_decode_gpu as TD
    from oracle import lattice, referee
    D = _mod("decoder")
    cfg = shipped.CONFIGS[DEC_FAMILY]
    d, depth, model = cfg["d"], cfg["volume_depth"], cfg["error_model"]
    A, layers = lattice.num_actions(d, model, cfg["use_Y"])
    _, flat = shipped.shipped_weights(DEC_FAMILY, str(DEC_P))
    flat = np.ascontiguousarray(flat, dtype=np.float32)
    base, block = 2 ** 32 - 3, 2
    n_blocks = (n + block - 1) // block
    venv = _lut_env(dq)
    ev = D.Evaluator(d, model, cfg["use_Y"], depth, chunk=n)
    dec = D.BatchDecoder((depth + layers, 2 * d + 1, 2 * d + 1), shipped.C_LAYERS, shipped.FF_LAYERS, A, d, model, cfg["use_Y"], depth, masked_greedy=True,
                         obs_form="uint8", chunk=n)
    MA = dec.max_actions
    try:
        def run(a):
            a.request("params", (flat.size,), torch.float32, 16, init=flat)
            a.request("packed", (dec.net.packed_bytes,), torch.uint8, 16)
            a.request("volumes", (n, depth, d + 1, d + 1), torch.uint8, 4)
            a.request("hidden", (n, d, d), torch.uint8, 1)
            a.request("trivial", (n,), torch.uint8, 1)
            a.request("corr", (n, MA), torch.int32, 4)
            a.request("ncorr", (n,), torch.int32, 4)
            a.request("frame", (n, d, d), torch.uint8, 1)
            a.request("status", (n,), torch.uint8, 1)
            a.request("verdict", (n,), torch.uint8, 1)
            a.request("verdict0", (n,), torch.uint8, 1)
            a.request("counters", (n_blocks, len(D.COUNTER_NAMES)), torch.int64, 8)
            a.request("counters0", (n_blocks, len(D.COUNTER_NAMES)), torch.int64, 8)
            k = a.take
            k("counters").zero_(); k("counters0").zero_()
            ev.sample_into(venv, n, base, ENV_SEED, DEC_P, DEC_P, k("volumes"), k("hidden"), k("trivial"))
            pk = dec.net.pack(k("params"), out=k("packed"))
            dec._decode_into(k("params"), pk, k("volumes"), n, k("corr"), k("ncorr"), k("frame"), k("status"))
            ev.verdict_into(venv, k("hidden"), k("frame"), n, k("verdict"))
            ev.verdict_into(venv, k("hidden"), None, n, k("verdict0"))
            ev.count_into(k("verdict"), k("trivial"), k("status"), k("ncorr"), n, 0, block, k("counters"))
            ev.count_into(k("verdict0"), k("trivial"), None, None, n, 0, block, k("counters0"))

        out, _ = both_fills(run)
        lx, lz = venv.get_referee()
    finally:
        dec.close(); ev.close(); venv.close()
    vol, hid, triv = V.sample_volumes(d, model, depth, n, DEC_P, DEC_P, ENV_SEED, base)
    assert np.array_equal(arr(out["volumes"], np.uint8, vol.shape), vol) and np.array_equal(arr(out["hidden"], np.uint8, hid.shape), hid)
    assert np.array_equal(out["trivial"], triv) and triv.sum() < n
    # the decode
    spec = TD._spec(DEC_FAMILY)
    qfun = lambda obs: O.forward(spec, flat, np.asarray(obs, dtype=np.uint8)[None])[0][0]
    corr, ncorr = arr(out["corr"], np.int32, (n, MA)), arr(out["ncorr"], np.int32)
    frame, status = arr(out["frame"], np.uint8, (n, d, d)), arr(out["status"], np.uint8)
    got = [list(map(int, corr[i, :ncorr[i]])) for i in range(n)]
    want = [R.decode_volume(vol[i], qfun, d, model, cfg["use_Y"], True) for i in range(n)]
    TD.assert_same_or_near_tie(DEC_FAMILY, flat, vol, got, [list(w[0]) for w in want], True, max_disagree=max(1, n // 20))
    for i in range(n):
        assert (corr[i, ncorr[i]:] == -1).all(), i                  # padded with -1
        if got[i] == list(want[i][0]):
            assert np.array_equal(frame[i], want[i][1]) and int(status[i]) == int(want[i][2]), i
    assert sum(len(g) for g in got) > 0
    # verdict of the frames the device produced, and the counters per block of two volumes
    classify = V.classify_with(referee.LutReferee(d, model, lx, lz))
    verd, verd0 = V.verdict(d, hid, frame, classify), V.verdict(d, hid, None, classify)
    assert np.array_equal(out["verdict"], verd) and np.array_equal(out["verdict0"], verd0)
    cnt, cnt0 = arr(out["counters"], np.int64, (n_blocks, -1)), arr(out["counters0"], np.int64, (n_blocks, -1))
    for b in range(n_blocks):
        s = slice(b * block, min(n, (b + 1) * block))
        assert cnt[b].tolist() == D.counters_from_arrays(verd[s], triv[s], status[s], ncorr[s]), b
        assert cnt0[b].tolist() == D.counters_from_arrays(verd0[s], triv[s]), b


@pytest.mark.parametrize("n", [5, 67])
def test_narrow_matching_union_find_and_streams(dq, torch_mod, n):
    """dq_decode_match, dq_decode_uf, dq_stream_decode_uf and dq_stream_decode_uf_closed on n volumes / streams in the arena (volumes 4-byte aligned, streams and frames at
    any byte offset, the int32 [n][2] arrays at 4).  References: match_st_ref's certificate (test_match_st_gpu), union_find_ref, stream_uf_ref, closed_uf_ref."""
    torch = torch_mod
    import types
    import closed_uf_ref as C
    import decode_eval_ref as V
    import shipped
    import stream_uf_ref as S
    import test_match_st_gpu as TM
    import union_find_ref as U
    D = _mod("decoder")
    cfg = shipped.CONFIGS[DEC_FAMILY]
    d, depth, model = cfg["d"], cfg["volume_depth"], cfg["error_model"]
    T, commit = 12, 2
    vol = V.sample_volumes(d, model, depth, n, 0.011, 0.011, ENV_SEED, 7)[0]
    syn = V.sample_volumes(d, model, T, n, 0.011, 0.011, ENV_SEED, 700)[0]
    ev = D.Evaluator(d, model, cfg["use_Y"], depth, chunk=n)
    try:
        def run(a):
            a.request("vol", vol.shape, torch.uint8, 4, init=vol)
            a.request("syn", syn.shape, torch.uint8, 1, init=syn)   # (the stream kernels read single cells: no alignment is asked of a stream)
            for who in ("m", "u", "s", "c"):
                a.request(who + "_frame", (n, d, d), torch.uint8, 1)
                a.request(who + "_weight", (n, 2), torch.int32, 4)
                a.request(who + "_ndef", (n, 2), torch.int32, 4)
                a.request(who + ("_inexact" if who == "m" else "_rounds"), (n,) if who == "m" else (n, 2), torch.uint8 if who == "m" else torch.int32,
                          1 if who == "m" else 4)
            k = a.take
            ev.match_into(k("vol"), n, k("m_frame"), k("m_weight"), k("m_ndef"), k("m_inexact"))
            ev.uf_into(k("vol"), n, k("u_frame"), k("u_weight"), k("u_ndef"), k("u_rounds"))
            ev.stream_uf_into(k("syn"), n, T, commit, k("s_frame"), k("s_weight"), k("s_ndef"), k("s_rounds"))
            ev.stream_uf_into(k("syn"), n, T, commit, k("c_frame"), k("c_weight"), k("c_ndef"), k("c_rounds"), final_round="perfect")

        out, _ = both_fills(run)
    finally:
        ev.close()
    fr = lambda who: arr(out[who + "_frame"], np.uint8, (n, d, d))
    i2 = lambda key: arr(out[key], np.int32, (n, 2))
    # matching: exact (no flag), the defect counts, and the certificate of minimum weight per component
    assert not out["m_inexact"].any() and np.array_equal(i2("m_ndef"), TM._n_defects(d, vol))
    assert TM._certify_all(d, depth, vol, types.SimpleNamespace(frame=fr("m"), weight=i2("m_weight"))) == []
    # union-find on volumes, on streams, and on streams closed by a perfect round
    for who, want in (("u", U.decode(d, vol, depth)), ("s", S.decode(d, syn, depth, commit)[:4]), ("c", C.decode(d, syn, depth, commit, True)[:4])):
        frame, weight, ndef, rounds = want
        assert np.array_equal(fr(who), frame), who
        assert np.array_equal(i2(who + "_weight"), weight) and np.array_equal(i2(who + "_ndef"), ndef) and np.array_equal(i2(who + "_rounds"), rounds), who
    assert fr("m").any() and fr("u").any() and fr("s").any()
