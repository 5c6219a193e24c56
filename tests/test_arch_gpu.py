"""GPU tests of the per-layer implicit-GEMM path (csrc/qnet.hip + csrc/gemm.h) on architectures beside the reference's, of minibatches smaller than
max_batch, and of both sides of every point where the library switches between the fused chains and the per-layer kernels -- all against the float64
oracle (oracle/dqn_oracle.py, itself checked against torch float64 autograd on the same inputs: tests/test_oracle_dqn.py) at the project's tolerances:

  Q                                max(1e-5, 2e-6 max |ref|)
  gradient, overall                2e-5 * max(1, max |g_ref|)
  gradient, per layer tensor       1e-4 * max |ref| + 1e-7
  weights after one Adam step      1e-6

No sample is left out of a gradient comparison: where the oracle's training forward has a ReLU pre-activation within 1e-6 of 0 (a "fragile" sample, whose
gradient depends on which side of the ReLU an fp32 sum lands), the side the device took is read back per sample (tests/relu_choices.py) and the oracle is
evaluated with it; the architecture list's inputs are chosen so that all but one entry have no such sample, and the counts are asserted."""
import functools

import numpy as np
import pytest

import architectures as AR
from oracle import dqn_oracle as O
from relu_choices import device_relu_choices

pytestmark = pytest.mark.gpu

REF_CONV, REF_FF = AR.REF_CONV, AR.REF_FF


def tol(ref):
    return max(1e-5, 2e-6 * float(np.abs(np.asarray(ref)).max()))


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def build(dq, torch, spec, flat, max_batch, per_layer=True):
    """(net, params on the device).  per_layer: set_fused(False) where the handle reports the fused chains; as created otherwise."""
    net = dq.QNetwork(spec.input_shape, spec.c_layers, spec.ff_layers, spec.n_actions, dueling=spec.dueling, max_batch=max_batch)
    assert net.n_params == spec.n_params == flat.size
    if per_layer and net.fused_supported:
        net.set_fused(False)
    return net, torch.from_numpy(flat).cuda()


def check_q(q, q_ref, label):
    err = float(np.abs(q - q_ref).max())
    print(f"{label}: Q error {err:.2e} (bound {tol(q_ref):.1e}, max |Q| {np.abs(q_ref).max():.3g})")
    assert q.shape == q_ref.shape and err < tol(q_ref), (label, err)
    return err


def check_grad(g, g_ref, spec, label):
    scale = float(np.abs(g_ref).max())
    err = float(np.abs(g - g_ref).max())
    worst = 0.0
    for li, ((gk, gb), (rk, rb)) in enumerate(zip(spec.split(g), spec.split(g_ref))):
        for a, b in ((gk, rk), (gb, rb)):
            e, s = float(np.abs(a - b).max()), float(np.abs(b).max())
            worst = max(worst, e / s if s > 0 else 0.0)
            assert e <= 1e-4 * s + 1e-7, (label, li, e, s)
    print(f"{label}: gradient error {err:.2e} of max |g| {scale:.3g} (bound {2e-5 * max(1.0, scale):.1e}); worst layer tensor {worst:.2e} of its largest element")
    assert scale > 0 and err < 2e-5 * max(scale, 1.0), (label, err, scale)
    return err


def reference_gradient(net, params, spec, flat, cache, dq_, fwd, label, expect_fragile=None):
    """The oracle's gradient for the training forward `fwd()` has just run on `net` -- every sample included.  Without a fragile sample: O.backward as it
    stands.  Else the device's side of each near-zero ReLU is identified through one-sample backwards (which read what fwd() saved; fwd() is run again
    by the identification, with the same result) and the oracle takes those bits."""
    fragile = O.fragile_samples(cache, thr=1e-6)
    n = int(fragile.sum())
    if expect_fragile is not None:
        assert n == expect_fragile, (label, n)
    if n == 0:
        return O.backward(spec, flat, cache, np.asarray(dq_, np.float64))
    choices = device_relu_choices(net, params, spec, flat, None, None, fwd, thr=1e-6, cache=cache, label=label)
    assert choices.n_samples == n
    return O.backward(spec, flat, cache, np.asarray(dq_, np.float64), relu_on=choices)


def train_and_compare(torch, net, params, spec, flat, obs_t, obs, keep, dropout, rng, label, expect_fragile=None, cache_q=None):
    """Training forward + backward of `net` on obs against the oracle; the backward twice, bit-identical.  Returns (Q error, gradient error)."""
    batch = obs.shape[0]
    fwd = lambda: net.forward(params, obs_t, batch=batch, training=True, **dropout)
    q = fwd().cpu().numpy()
    q_ref, cache = cache_q if cache_q is not None else O.forward(spec, flat, obs, training=True, keep_masks=keep)
    eq = check_q(q, q_ref, label + " training")
    dq_ = (rng.randn(batch, spec.n_actions) / batch).astype(np.float32)
    g_ref = reference_gradient(net, params, spec, flat, cache, dq_, fwd, label, expect_fragile)
    dq_t = torch.from_numpy(dq_).cuda()
    g = net.backward(params, dq_t).cpu().numpy()
    eg = check_grad(g, g_ref, spec, label)
    assert np.array_equal(g, net.backward(params, dq_t).cpu().numpy()), label         # deterministic: the same bits twice
    return eq, eg


# ---- the architecture list ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def arch_reference(name):
    """The entry's inputs and the oracle's inference and training forwards on them: computed once, shared by the tests below, never written to."""
    spec, B, flat, obs, rng, keep = AR.entry(name)
    q_inf = O.forward(spec, flat, obs)[0]
    q_train, cache = O.forward(spec, flat, obs, training=True, keep_masks=keep)
    return spec, B, flat, obs, keep, q_inf, q_train, cache


@pytest.mark.parametrize("name", sorted(AR.ARCHITECTURES))
def test_inference_forward(dq, torch_mod, name):
    """A direct observation batch, a ring gathered through index / index_off / index_mod with wrap-around, and a batch of one."""
    torch = torch_mod
    spec, B, flat, obs, keep, q_inf, _, _ = arch_reference(name)
    net, params = build(dq, torch, spec, flat, B)
    assert not (net.fused_supported and net.fused_enabled)
    obs_t = torch.from_numpy(obs).cuda()
    check_q(net.forward(params, obs_t).cpu().numpy(), q_inf, f"ARCH {name} B={B} inference")
    check_q(net.forward(params, obs_t[:1].contiguous()).cpu().numpy(), q_inf[:1], f"ARCH {name} B=1")
    rng = np.random.RandomState(77)
    R = 2 * B + 3
    ring = (rng.rand(R, *spec.input_shape) < 0.3).astype(np.uint8)
    ring[3] = obs[0]
    idx = rng.randint(0, R, size=B).astype(np.int32)
    idx[0], idx[-1], off = R - 1, 3, B + 1                          # (R - 1 + off wraps; so does about half of the others)
    assert ((idx.astype(np.int64) + off) >= R).sum() > 1 and ((idx.astype(np.int64) + off) < R).sum() > 1
    ring_t, idx_t = torch.from_numpy(ring).cuda(), torch.from_numpy(idx).cuda()
    q_ring = O.forward(spec, flat, ring[(idx.astype(np.int64) + off) % R])[0]
    check_q(net.forward(params, ring_t, index=idx_t, index_off=off, index_mod=R).cpu().numpy(), q_ring, f"ARCH {name} B={B} ring")
    q_one = net.forward(params, ring_t, index=idx_t[-1:].contiguous()).cpu().numpy()      # batch 1 through the gather, no offset: ring row 3 = obs[0]
    check_q(q_one, q_inf[:1], f"ARCH {name} B=1 ring")


@pytest.mark.parametrize("name", sorted(AR.ARCHITECTURES))
def test_training_forward_backward(dq, torch_mod, name):
    """Training forward (every dropout layer under its own mask) and backward against the oracle, every sample compared."""
    torch = torch_mod
    spec, B, flat, obs, keep, _, q_train, cache = arch_reference(name)
    net, params = build(dq, torch, spec, flat, B)
    rng = np.random.RandomState(AR.INPUT_SEED[name] + 1000)
    train_and_compare(torch, net, params, spec, flat, torch.from_numpy(obs).cuda(), obs, keep, AR.DROPOUT, rng, f"ARCH {name} B={B}",
                      expect_fragile=AR.FRAGILE[name], cache_q=(q_train, cache))


def full_td_update(dq, torch, net, params, spec, flat, obs, label, seed=(1, 2), t=1, lr=1e-4, gamma=0.99, rng_seed=21):
    """One complete DQN update through dq_qnet_td_backward_adam with a dq buffer -- on a network whose backward is not fused: dq_td_step, the per-layer
    backward, dq_adam_step -- against the oracle's td_targets / loss_and_grad / backward / adam_step (tests/test_qnet_gpu.py
    test_one_full_update_matches_oracle, on this route)."""
    from importlib import import_module
    Q = import_module("deepq-decoding_amd.qnet")
    B, A = obs.shape[0], spec.n_actions
    rng = np.random.RandomState(rng_seed)
    flat_t = flat + (rng.randn(flat.size) * 0.01).astype(np.float32)
    s1 = (rng.rand(B, *spec.input_shape) < 0.3).astype(np.uint8)
    reward, terminal = (rng.rand(B) < 0.5).astype(np.float32), (rng.rand(B) < 0.2).astype(np.uint8)
    action = rng.randint(0, A, size=B).astype(np.int32)
    cu = lambda a: torch.from_numpy(a).cuda()
    target, obs_t = cu(flat_t), cu(obs)
    p0 = params.clone()
    q1o, q1t = net.forward(p0, cu(s1)), net.forward(target, cu(s1))
    fwd = lambda: net.forward(p0, obs_t, training=True, seed=seed, t=t)
    q0 = fwd()
    # oracle
    keep = AR.keep_masks(spec, B, seed, t, 0)
    y_ref = O.td_targets(O.forward(spec, flat, s1)[0], O.forward(spec, flat_t, s1)[0], reward, terminal, gamma)
    q0_ref, cache = O.forward(spec, flat, obs, training=True, keep_masks=keep)
    loss_ref, mq_ref, dq_ref = O.loss_and_grad(q0_ref, action, y_ref)
    g_ref = reference_gradient(net, p0, spec, flat, cache, dq_ref, fwd, label)      # (its probes read the forward saved under p0)
    p_ref, _, _ = O.adam_step(flat.astype(np.float64), g_ref, np.zeros_like(g_ref), np.zeros_like(g_ref), 1, lr)
    # device
    p, m, v, g = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0), torch.empty_like(p0)
    y, dq_ = torch.empty(B, device="cuda"), torch.empty((B, A), device="cuda")
    met = torch.zeros(Q.TD_METRICS_FLOATS, dtype=torch.float32, device="cuda")
    td = dict(q_online_s1=q1o, q_target_s1=q1t, q_s0=q0, reward=cu(reward), terminal=cu(terminal), action=cu(action), gamma=gamma,
              grad_scale=1.0 / B, y=y, dq=dq_, metrics=met)
    net.td_backward_adam(p, td, g, m, v, 1, lr)
    Q.td_metrics(met, B)
    mt = met[:2].cpu().numpy()
    assert abs(mt[0] - loss_ref) < tol(loss_ref) and abs(mt[1] - mq_ref) < tol(mq_ref), (label, mt, loss_ref, mq_ref)
    assert np.abs(y.cpu().numpy() - y_ref).max() < tol(y_ref)
    assert np.abs(dq_.cpu().numpy() - dq_ref).max() < 1e-7
    check_grad(g.cpu().numpy(), g_ref, spec, label + " TD update")
    big = np.abs(g_ref) > 1e-6                                       # first Adam step moves every weight by ~lr * sign(g): compare where the gradient is not ~0
    err_p = float(np.abs(p.cpu().numpy() - p_ref)[big].max())
    print(f"{label} TD update: loss {mt[0]:.6f} (oracle {loss_ref:.6f}), weights after Adam off by {err_p:.2e} (bound 1e-6) on {int(big.sum())} of {big.size}")
    assert big.any() and err_p < 1e-6
    assert not torch.equal(p, p0)


WIDE = sorted(n for n in AR.ARCHITECTURES if n.startswith("wide_"))


@pytest.mark.parametrize("name", WIDE)
def test_the_wide_entries_run_per_layer(dq, torch_mod, name):
    """The networks of d = 11 .. 15 as created (the library chooses the path): A + 1 > 128 outputs, so neither fused chain covers them -- the support
    queries say so, and a silent change of dispatch fails here."""
    shape, c_layers, ff_layers, A, dueling, B = AR.ARCHITECTURES[name]
    assert (c_layers, ff_layers, dueling) == (REF_CONV, REF_FF, True) and expected_dispatch(shape, c_layers, ff_layers, A, dueling) == (False, False)
    net = dq.QNetwork(shape, c_layers, ff_layers, A, dueling=dueling, max_batch=B)
    assert net.n_params == AR.spec_of(name).n_params
    assert not net.fused_supported and not net.fused_backward_supported and net.packed_bytes == 0


# (the wide pair: dq_td_step, the per-layer backward and dq_adam_step at 365 and 677 head columns, 1.66 M and 3.59 M parameters)
@pytest.mark.parametrize("name", ["one_conv_no_hidden", "k1_s1_two_hidden", "ref_cin11", "wide_d11_dpy", "wide_d15_dpy"])
def test_one_full_td_update_through_the_per_layer_route(dq, torch_mod, name):
    torch = torch_mod
    spec, B, flat, obs, _, _, _, _ = arch_reference(name)
    net, params = build(dq, torch, spec, flat, B + 7)
    full_td_update(dq, torch, net, params, spec, flat, obs, f"ARCH {name} B={B}")


# ---- minibatches smaller than max_batch -----------------------------------------------------------------------------------------------------
def _ceil(a, b):
    return -(-a // b)


def wgrad_slices(M, K, N):
    """csrc/qnet.hip wgrad_slices restated: slices of the weight-gradient reduction over M rows."""
    tiles = _ceil(K, 128) * _ceil(N, 64)
    want = max(1, _ceil(768, tiles))
    rows = max(64, _ceil(_ceil(M, want), 32) * 32)
    return _ceil(M, rows)


def slices_needed(spec, batch):
    """Per layer: (slices, floats per slice) of a backward on `batch` samples."""
    out = []
    for (kind, L), (k, b) in zip(spec.layers, spec.param_shapes()):
        K, N = int(np.prod(k[:-1])), k[-1]
        rows = L["oh"] * L["ow"] if kind == "conv" else 1
        out.append((wgrad_slices(batch * rows, K, N), K * N + N))
    return out


def parent_workspace_short(spec, max_batch, batch):
    """Would a workspace sized from the slice counts AT max_batch (the rule before this test existed) be too small for `batch`?"""
    have = max(s * f for s, f in slices_needed(spec, max_batch))
    return any(s * f > have for s, f in slices_needed(spec, batch))


SUB_BATCH = {
    # the d = 7 shape of BASELINE.json (c5; volume_depth 16 always takes this path): 14 slices of Dense(512) at 705..896 samples, 11 at 1024
    "c5": (((9, 15, 15), REF_CONV, REF_FF, 99, True), 1024, 896, 5),
    # Flatten 1200 -> Dense(1024): 5 slices at 320 samples, 4 at 321
    "dense1024": (((2, 6, 6), [[48, 2, 1]], [[1024, 0.25]], 10, True), 321, 320, 5),
}


@pytest.mark.parametrize("name", sorted(SUB_BATCH))
def test_a_minibatch_smaller_than_max_batch_where_the_slice_count_steps_up(dq, torch_mod, name):
    """The weight-gradient slice count is not monotonic in the batch: these batches need MORE slices of the widest layer than max_batch does.  A
    workspace sized at max_batch refused them (DQ_ERR_STATE "workspace too small"); it is sized for the worst batch up to max_batch."""
    torch = torch_mod
    (shape, c_layers, ff_layers, A, dueling), max_batch, batch, seed = SUB_BATCH[name]
    spec = O.QNetSpec(shape, c_layers, ff_layers, A, dueling=dueling)
    assert parent_workspace_short(spec, max_batch, batch)           # (the case is what it claims to be)
    flat, obs, rng = AR.make_inputs(spec, batch, seed)
    net, params = build(dq, torch, spec, flat, max_batch)
    keep = AR.keep_masks(spec, batch, **AR.DROPOUT)
    train_and_compare(torch, net, params, spec, flat, torch.from_numpy(obs).cuda(), obs, keep, AR.DROPOUT, rng, f"SUB {name} B={batch} of {max_batch}")


SWEEPS = {
    # the Dense(1024) stack above: 257 and 319 are sizes the workspace of before was too small for (every size from 257 to 320 is)
    "per-layer": (SUB_BATCH["dense1024"][0], 321, (1, 37, 200, 257, 319), [257, 319]),
    # the reference's stack on the fused chains (whose workspaces do not depend on the batch)
    "fused": (((4, 7, 7), REF_CONV, REF_FF, 10, True), 417, (1, 37, 193, 352, 416), None),
    # the d = 15 stack with Y moves (architectures.py wide_d15_dpy) in an order that descends: after 64 samples the handle's activations, masks and
    # partial sums hold the rows of a larger batch than the one being computed.  No size up to 64 needs more workspace than 64 does (one slice of the
    # 2.77 M-element Dense(512) gradient at every size; the convolutions' slice counts grow with the batch up to 225, 196 and 169 at 64)
    "wide": (AR.ARCHITECTURES["wide_d15_dpy"][:5], 64, (37, 64, 1, 33, 5), []),
}


def workspace_need(spec, batch):
    """Floats of partial sums a backward on `batch` samples needs: the largest layer's slices * floats per slice."""
    return max(s * f for s, f in slices_needed(spec, batch))


@pytest.mark.parametrize("path", sorted(SWEEPS))
def test_batch_sizes_below_max_batch_on_one_handle(dq, torch_mod, path):
    """Five batch sizes up to max_batch on ONE handle, uint8 input, on either path: Q and gradient against the oracle at each size."""
    torch = torch_mod
    (shape, c_layers, ff_layers, A, dueling), max_batch, sizes, short = SWEEPS[path]
    spec = O.QNetSpec(shape, c_layers, ff_layers, A, dueling=dueling)
    if short is not None:
        assert [b for b in sizes if parent_workspace_short(spec, max_batch, b)] == short
    if path == "wide":
        # the sweep holds the batch with the largest workspace need of all batches the handle accepts, and, layer by layer, the one with the most slices
        every = range(1, max_batch + 1)
        assert max(sizes) <= max_batch and max(workspace_need(spec, b) for b in sizes) == max(workspace_need(spec, b) for b in every)
        for li in range(len(spec.layers)):
            assert max(slices_needed(spec, b)[li][0] for b in sizes) == max(slices_needed(spec, b)[li][0] for b in every), li
        assert any(a > b for a, b in zip(sizes, sizes[1:])) and any(a < b for a, b in zip(sizes, sizes[1:]))      # (it descends, and ascends again)
    flat, obs, rng = AR.make_inputs(spec, max(sizes), 5)
    net, params = build(dq, torch, spec, flat, max_batch, per_layer=path != "fused")
    assert (net.fused_supported and net.fused_backward_supported and net.fused_enabled) == (path == "fused")
    keep = AR.keep_masks(spec, max(sizes), **AR.DROPOUT)
    q_all, cache_all = O.forward(spec, flat, obs, training=True, keep_masks=keep)      # samples are independent: one oracle forward serves every size
    q_inf = O.forward(spec, flat, obs)[0]
    obs_t = torch.from_numpy(obs).cuda()
    for b in sizes:
        check_q(net.forward(params, obs_t, batch=b).cpu().numpy(), q_inf[:b], f"SWEEP {path} B={b} inference")
        train_and_compare(torch, net, params, spec, flat, obs_t, obs[:b], [k[:b] for k in keep], AR.DROPOUT, rng, f"SWEEP {path} B={b} of {max_batch}",
                          cache_q=(q_all[:b], O.sample_cache(cache_all, np.arange(b))))


# ---- both sides of every switch between the fused chains and the per-layer kernels -----------------------------------------------------------
def expected_dispatch(shape, c_layers, ff_layers, n_actions, dueling):
    """(forward fused, backward fused) from the limits DESIGN.md section 6 states: the reference's stack (Conv 64/3/2, 32/2/1, 32/2/1, Dense(512)), at most
    96 rows in the first kernel (10 input planes); forward: at most 128 outputs in the widest head layer (127 actions with a dueling head); backward: at
    most 112 (111 actions with one) and observations of at most 2045 bytes."""
    C, H, W = shape
    if [list(l) for l in c_layers] != REF_CONV or [l[0] for l in ff_layers] != [512]:
        return False, False
    widest = n_actions + 1 if dueling else n_actions
    fwd = 9 * C <= 96 and widest <= 128
    return fwd, fwd and widest <= 112 and C * H * W <= 2045


EDGES = {f"A{a}": ((7, 11, 11), a, True) for a in (63, 64, 65, 111, 112, 127, 128)}      # NT2 of plan_dense / plan_dense_bwd; last fused backward | mixed; last fused forward | per-layer
EDGES.update({f"A{a}-plain": ((7, 11, 11), a, False) for a in (112, 113)})
EDGES.update({f"C{c}": ((c, 11, 11), 51, True) for c in (1, 2, 3, 10, 11)})             # KG1 clamped to 3 below 33 kernel rows; K = 90 | 99
EDGES.update({"non-square": ((5, 9, 13), 51, True), "even-d": ((6, 13, 13), 51, True), "17x17": ((8, 17, 17), 51, True)})
EDGE_DISPATCH = {"A63": (1, 1), "A64": (1, 1), "A65": (1, 1), "A111": (1, 1), "A112": (1, 0), "A127": (1, 0), "A128": (0, 0), "A112-plain": (1, 1),
                 "A113-plain": (1, 0), "C1": (1, 1), "C2": (1, 1), "C3": (1, 1), "C10": (1, 1), "C11": (0, 0), "non-square": (1, 1), "even-d": (1, 1),
                 "17x17": (1, 0)}                                     # (8 x 17 x 17 = 2312 bytes: past the backward's observation limit)


@pytest.mark.parametrize("case", list(EDGES))
def test_both_sides_of_every_dispatch_switch(dq, torch_mod, case):
    """The reference stack as created (the library chooses the path), uint8 input, batch 37: which path answers is asserted through the support queries --
    a silent change of dispatch fails here --, and forward, training forward and backward agree with the oracle on whichever it is."""
    torch = torch_mod
    shape, A, dueling = EDGES[case]
    spec = O.QNetSpec(shape, REF_CONV, REF_FF, A, dueling=dueling)
    exp_f, exp_b = expected_dispatch(shape, REF_CONV, REF_FF, A, dueling)
    assert (exp_f, exp_b) == tuple(bool(x) for x in EDGE_DISPATCH[case])
    B = 37
    flat, obs, rng = AR.make_inputs(spec, B, 5)
    net, params = build(dq, torch, spec, flat, B, per_layer=False)
    assert net.fused_supported == exp_f and (net.packed_bytes > 0) == exp_f and net.fused_backward_supported == exp_b, \
        (case, net.fused_supported, net.packed_bytes, net.fused_backward_supported)
    obs_t = torch.from_numpy(obs).cuda()
    check_q(net.forward(params, obs_t).cpu().numpy(), O.forward(spec, flat, obs)[0], f"EDGE {case} inference")
    keep = AR.keep_masks(spec, B, **AR.DROPOUT)
    train_and_compare(torch, net, params, spec, flat, obs_t, obs, keep, AR.DROPOUT, rng, f"EDGE {case} (fused forward {exp_f}, backward {exp_b})")
    net.check_range()


MIXED = {"A120": ((7, 11, 11), 120), "d7-10planes": ((10, 15, 15), 99)}


@pytest.mark.parametrize("case", sorted(MIXED))
def test_the_mixed_network(dq, torch_mod, case):
    """Forward fused, backward not (120 actions with a dueling head; the 2250-byte observations of d = 7 with 10 input planes): inference forwards run
    on the fused chains -- also those that share a forward_multi call with a training job --, every training forward and every backward per layer."""
    torch = torch_mod
    shape, A = MIXED[case]
    spec = O.QNetSpec(shape, REF_CONV, REF_FF, A)
    B = 45
    flat, obs, rng = AR.make_inputs(spec, B, 5)
    net, params = build(dq, torch, spec, flat, B + 3, per_layer=False)
    assert net.fused_supported and net.packed_bytes > 0 and not net.fused_backward_supported
    obs_t = torch.from_numpy(obs).cuda()
    ring = torch.from_numpy((rng.rand(3 * B, *shape) < 0.3).astype(np.uint8)).cuda()
    idx = torch.from_numpy(rng.randint(0, 3 * B, size=B).astype(np.int32)).cuda()
    ring_obs = ring.cpu().numpy()[(idx.cpu().numpy().astype(np.int64) + 2 * B) % (3 * B)]
    target = torch.from_numpy(flat + (rng.randn(flat.size) * 0.01).astype(np.float32)).cuda()
    # the inference forward == forward_multi of the same job, bit for bit (both take the fused chains)
    q = net.forward(params, obs_t)
    assert torch.equal(q, net.forward_multi([dict(params=params, obs=obs_t)])[0])
    check_q(q.cpu().numpy(), O.forward(spec, flat, obs)[0], f"MIXED {case} inference")
    # training forward, backward: the per-layer path behind the same calls
    keep = AR.keep_masks(spec, B, **AR.DROPOUT)
    train_and_compare(torch, net, params, spec, flat, obs_t, obs, keep, AR.DROPOUT, rng, f"MIXED {case} B={B}")
    # one training and two inference jobs in one call: the inference jobs share one fused launch pair, the training job runs per layer -- each job the
    # kernels of a call of its own, so the three separate calls' Q-values bit for bit; and each within the Q tolerance of the oracle
    jobs = [dict(params=target, obs=ring, index=idx, index_off=2 * B, index_mod=3 * B), dict(params=params, obs=ring, index=idx, index_off=2 * B, index_mod=3 * B),
            dict(params=params, obs=obs_t, training=True, **AR.DROPOUT)]
    single = [net.forward(**j).clone() for j in jobs]
    multi = net.forward_multi(jobs)
    refs = [O.forward(spec, target.cpu().numpy(), ring_obs)[0], O.forward(spec, flat, ring_obs)[0], O.forward(spec, flat, obs, training=True, keep_masks=keep)[0]]
    for i, (a, b, r) in enumerate(zip(single, multi, refs)):
        check_q(b.cpu().numpy(), r, f"MIXED {case} job {i} of three")
        assert torch.equal(a, b), (case, i, float((a - b).abs().max()))
    # the same with the packed weights the jobs bring (what DQNCore passes), and with the jobs in another order
    pk_t, pk_p = net.pack(target), net.pack(params)
    packed = [dict(jobs[2]), dict(jobs[0], packed=pk_t), dict(jobs[1], packed=pk_p)]
    for a, b in zip((single[2], single[0], single[1]), net.forward_multi(packed)):
        assert torch.equal(a, b), case
    # the training forward of that call is what the backward differentiates
    dq_ = torch.from_numpy((rng.randn(B, A) / B).astype(np.float32)).cuda()
    g_multi = net.backward(params, dq_).clone()
    net.forward(**jobs[2])
    assert torch.equal(g_multi, net.backward(params, dq_))
    full_td_update(dq, torch, net, params, spec, flat, obs, f"MIXED {case} B={B}")
    net.check_range()                                               # healthy so far: silent
    # the fused forward's range guard reports here too (its word does not belong to the fused backward's workspace)
    bad = params.clone()
    bad[net.layers[1]["kernel_offset"] + 5] = 7.0e4                 # a parameter outside the f16 pieces' range
    net.forward(bad, obs_t)
    with pytest.raises(dq.DeepQError, match=r"\[forward\]"):
        net.check_range()
    net.check_range()                                               # (reported once)
    # ... while dq_qnet_adam_step on this handle does not guard: its gradients are the per-layer path's f32, and a non-finite element propagates as
    # in dq_adam_step (Keras), raising nothing
    g = torch.zeros_like(params)
    g[7] = float("nan")
    p, m, v = params.clone(), torch.zeros_like(params), torch.zeros_like(params)
    net.adam_step(p, g, m, v, 1, 1e-3)
    assert bool(torch.isnan(p[7])) and bool(torch.isfinite(p[8:]).all()) and torch.equal(p[8:], params[8:])
    net.check_range()
    assert net.range_discarded() == 0


# ---- dropout layers ---------------------------------------------------------------------------------------------------------------------------
def test_two_dropout_layers_of_equal_rate_draw_different_masks(dq, torch_mod):
    """Two hidden layers of 16 units, both with rate 0.5, read back through ONE training forward whose weights make every unit positive and its value
    a code of what was kept: layer 1 is the constant 1 (kept: 2), layer 2's unit k = 1 + sum_j 2^j h1[j] for every k (kept: twice that), the output
    layer the identity -- Q[b, k] = 0 where layer 2 dropped unit k, else 2 (1 + 2 sum_j keep1[b, j] 2^j): exact in f32.  The masks are the oracle's under
    the layers' ordinals 0 and 1 (include/deepq_hip.h dq_qnet_forward), and differ: Keras draws every Dropout layer independently."""
    torch = torch_mod
    U, B = 16, 96
    spec = O.QNetSpec((2, 5, 5), [[4, 2, 1]], [[U, 0.5], [U, 0.5]], U, dueling=False)
    P = [(np.zeros(k, np.float32), np.zeros(b, np.float32)) for k, b in spec.param_shapes()]
    P[1][1][:] = 1.0                                                 # Dense 1: kernel 0, bias 1
    P[2][0][:] = (2.0 ** np.arange(U))[:, None]                      # Dense 2: every unit the same code of its input
    P[2][1][:] = 1.0
    P[3][0][:] = np.eye(U, dtype=np.float32)
    flat = np.concatenate([np.concatenate([k.reshape(-1), b]) for k, b in P])
    obs = (np.random.RandomState(0).rand(B, 2, 5, 5) < 0.3).astype(np.uint8)
    net, params = build(dq, torch, spec, flat, B)
    seed, t, base = (9, 8), 2 ** 33 + 5, 4000
    q = net.forward(params, torch.from_numpy(obs).cuda(), training=True, seed=seed, t=t, sample_base=base).cpu().numpy().astype(np.float64)
    keep2 = q > 0
    assert keep2.any(axis=1).all()                                   # (a sample with all 16 units of layer 2 dropped would hide layer 1's mask: 2^-16 each)
    code = (q / 2 - 1) / 2
    assert all(len(set(code[b][keep2[b]])) == 1 for b in range(B))   # every kept unit of layer 2 carries the same code
    code = np.array([code[b][keep2[b]][0] for b in range(B)])
    assert np.array_equal(code, np.round(code)) and code.min() >= 0 and code.max() < 2 ** U
    keep1 = ((code.astype(np.int64)[:, None] >> np.arange(U)[None, :]) & 1).astype(bool)
    ref1, ref2 = (O.dropout_keep_mask(seed, t, base + np.arange(B), U, 0.5, layer=l) for l in (0, 1))
    print(f"DROPOUT two layers, rate 0.5: layer 1 keeps {keep1.mean():.3f}, layer 2 keeps {keep2.mean():.3f}, they agree on {(keep1 == keep2).mean():.3f} of the units "
          f"(independent draws: 0.5)")
    assert np.array_equal(keep1, ref1) and np.array_equal(keep2, ref2)
    assert not np.array_equal(keep1, keep2) and abs((keep1 == keep2).mean() - 0.5) < 0.06      # 1536 fair coins: 0.06 is 4.7 sigma
    assert np.abs(q - O.forward(spec, flat, obs, training=True, keep_masks=[ref1, ref2])[0]).max() == 0
