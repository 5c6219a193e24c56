"""Every variant of the wide union-find kernels where a dispatch or a stride mistake would show (csrc/uf_wide.h: ufw_with_mode, ufw_setup; csrc/uf_wide.hip:
wide_kernel; csrc/env_wide_uf.hip: env_wide_uf_kernel_of).  No reference runs on the device: the assertions are identities that include/deepq_hip.h promises
between the launches -- weights (1, 1) are the unit weights, w_corr = w_space is the weighted decode, decoding the syndromes a run wrote is the run, a teacher
that everybody follows is the policy, a per-row array is the uniform launch of each row -- at the shapes that ask every variant for its LDS maximum, and
with rows that differ enough for a wrong stride to change a frame (chosen on the CPU with tests/weighted_uf_ref.py and tests/correlated_uf_ref.py)."""
import pytest

import correlated_env_uf_ref as R
from test_wide_env_uf_cpu import SEED

pytestmark = pytest.mark.gpu

PAIRS = [(1, 1), (7, 4), (1, 3), (15, 2)]
TRIPLES = [(7, 4, 1), (7, 4, 7), (4, 4, 2), (15, 2, 3)]


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return torch


def _fields(torch, ev, n, T, commit, syn=None, run=None, **kw):
    """(frame, weight, n_defects, rounds) of n streams: decode_into on syn, or run_into with run = (lattice_id, seed, p_phys, p_meas, syndromes or None)."""
    dev, d = ev.device, ev.d
    frame = torch.full((n, d, d), 7, dtype=torch.uint8, device=dev)
    w, nd, r = (torch.full((n, 2), -7, dtype=torch.int32, device=dev) for _ in range(3))
    if run is None:
        ev.decode_into(syn, n, T, commit, frame, w, nd, r, **kw)
    else:
        hid, triv = torch.empty((n, d * d), dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)
        ev.run_into(n, T, commit, run[0], run[1], run[2], run[3], hid, triv, frame, w, nd, r, syndromes=run[4], **kw)
    return frame, w, nd, r


def _kw(row):
    """A pair or a triple as VectorEnv.uf_select_wide / guided_select_wide take it."""
    return dict(weights=tuple(row[:2]), **({} if len(row) == 2 else dict(correlated=int(row[2]))))


def _same(torch, a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("final_round", ["faulty", "perfect"])
def test_every_stream_variant_at_the_lds_maximum(dq, torch_mod, final_round):
    """d = 15, DP, window 32, commit 16, T = 33 (two windows: the carry and the final window run), 4 streams at 0.01 / 0.01: the run and the decode kernel of
    all three modes, open and closed -- the twelve instantiations, each with the largest dynamic LDS it can ask for."""
    torch = torch_mod
    d, T, window, commit, n = 15, 33, 32, 16, 4
    ev = dq.WideEvaluator(d, "DP", window=window, chunk=n)
    try:
        got = {}
        for key, kw in (("unit", {}), ("w11", dict(weights=(1, 1))), ("w44", dict(weights=(4, 4))), ("c444", dict(weights=(4, 4, 4)))):
            syn = torch.full((n, T, d + 1, d + 1), 7, dtype=torch.uint8, device=ev.device)
            ran = _fields(torch, ev, n, T, commit, run=(40, (11, 12), 0.01, 0.01, syn), final_round=final_round, **kw)
            assert _same(torch, ran, _fields(torch, ev, n, T, commit, syn=syn, final_round=final_round, **kw)), (key, "decode_into is not run_into")
            got[key] = ran + (syn,)
        assert _same(torch, got["w11"], got["unit"]), "weights (1, 1) are not the unit weights"
        assert _same(torch, got["c444"], got["w44"]), "w_corr = w_space is not the weighted decode"
        assert torch.equal(got["w44"][4], got["unit"][4])                                # (the sampler does not depend on the weights)
        assert (got["unit"][0].reshape(n, -1) != 0).any(dim=1).any() and int(got["unit"][2].sum()) > 0
    finally:
        ev.close()


def test_every_environment_variant_at_its_lds_maximum(dq, torch_mod):
    """The d15deep lattice of test_correlated_env_uf_gpu.py (d = 15, volume_depth 16), along six steps of the unit-weight policy: the select and the guided
    kernel of all three modes -- the six instantiations at the largest dynamic LDS the environment can ask for."""
    torch = torch_mod
    kw, n, _, _ = R.CONFIGS["d15deep"]
    env = dq.VectorEnv(n_envs=n, seed=SEED, env_id_base=0, backend="wide", **kw)
    ev = dq.WideEvaluator(env.d, env.error_model, window=env.volume_depth, chunk=n, device=env.device)
    modes = ({}, dict(weights=(1, 1)), dict(weights=(4, 4)), dict(weights=(4, 4), correlated=4))
    try:
        env.reset(write_obs=False)
        acted = 0
        for t in range(6):
            unit, w11, w44, c444 = (env.uf_select_wide(ev, **m).clone() for m in modes)
            assert torch.equal(w11, unit), (t, "weights (1, 1) are not the unit weights")
            assert torch.equal(c444, w44), (t, "w_corr = w_space is not the weighted decode")
            for m, want in zip(modes, (unit, w11, w44, c444)):
                assert torch.equal(env.guided_select_wide(ev, t, eps=1.0, guide_share=1.0, **m), want), (t, m, "a teacher everybody follows is not the policy")
            acted += int((unit != env.identity_index).sum()) + int((w44 != env.identity_index).sum())
            env.step(unit, auto_reset=True, write_obs=False)
        assert acted >= 1
    finally:
        ev.close()
        env.close()


@pytest.mark.parametrize("rows", [PAIRS, TRIPLES], ids=["pairs", "triples"])
def test_a_stream_decodes_under_its_own_row(dq, torch_mod, rows):
    """d = 5, DP, window 10, commit 5, T = 12, lattices 100 .. 103 at 0.03 / 0.06 under seed (5, 6): a uint8 device tensor of four different rows gives
    stream i what a uniform launch of row i gives stream i alone, from the run and from the decode kernel.  With the reference decoders on the CPU every
    one of the four streams has another frame under its neighbour's row (i + 1) % 4 than under its own, for the pairs and for the triples, so a stride of
    the other width, or a row off by one, changes a frame; the device is asked for the same of streams 0 .. 3."""
    torch = torch_mod
    d, T, window, commit, n, base, seed, rates = 5, 12, 10, 5, 4, 100, (5, 6), (0.03, 0.06)
    ev = dq.WideEvaluator(d, "DP", window=window, chunk=n)
    try:
        each = torch.tensor(rows, dtype=torch.uint8, device=ev.device)
        syn = torch.empty((n, T, d + 1, d + 1), dtype=torch.uint8, device=ev.device)
        ran = _fields(torch, ev, n, T, commit, run=(base, seed) + rates + (syn,), weights=each)
        dec = _fields(torch, ev, n, T, commit, syn=syn, weights=each)
        assert _same(torch, ran, dec)
        for i, row in enumerate(rows):
            alone = _fields(torch, ev, 1, T, commit, syn=syn[i:i + 1], weights=row)
            assert _same(torch, [x[i:i + 1] for x in dec], alone), (i, row, "decode")
            assert _same(torch, alone, _fields(torch, ev, 1, T, commit, run=(base + i, seed) + rates + (None,), weights=row)), (i, row, "run")
            neighbour = _fields(torch, ev, 1, T, commit, syn=syn[i:i + 1], weights=rows[(i + 1) % n])
            assert not torch.equal(neighbour[0], alone[0]), (i, "the neighbour's row gives the same frame: a wrong row would not show")
    finally:
        ev.close()


@pytest.mark.parametrize("rows,shown_by", [(PAIRS, 1), (TRIPLES, 3)], ids=["pairs", "triples"])
def test_a_lattice_acts_under_its_own_row(dq, torch_mod, rows, shown_by):
    """Four d = 5 lattices (DP, volume_depth 5, 0.004 / 0.04) along ten steps of row 0's policy: a uint8 device tensor [4, 2] / [4, 3] gives lattice i the
    action of a uniform launch of row i, as a policy and as a teacher everybody follows.  On the C oracle environment played by the reference decoders
    lattice `shown_by` acts differently under its neighbour's row on 8 (pairs) and 6 (triples) of these ten records."""
    torch = torch_mod
    kw, n = R.CONFIGS["d5dp"][0], 4
    env = dq.VectorEnv(n_envs=n, seed=SEED, env_id_base=0, backend="wide", **kw)
    ev = dq.WideEvaluator(env.d, env.error_model, window=env.volume_depth, chunk=n, device=env.device)
    try:
        each = torch.tensor(rows, dtype=torch.uint8, device=env.device)
        env.reset(write_obs=False)
        shown = 0
        for t in range(10):
            uniform = torch.stack([env.uf_select_wide(ev, **_kw(row)).clone() for row in rows])       # [row, lattice]
            want = uniform.diagonal()
            assert torch.equal(env.uf_select_wide(ev, weights=each), want), t
            assert torch.equal(env.guided_select_wide(ev, t, eps=1.0, guide_share=1.0, weights=each), want), t
            shown += int(uniform[(shown_by + 1) % n, shown_by] != uniform[shown_by, shown_by])
            env.step(uniform[0].contiguous(), auto_reset=True, write_obs=False)
        assert shown >= 1
    finally:
        ev.close()
        env.close()
