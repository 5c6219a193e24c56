"""Union-find stream decoding with a perfect final round on the device (final_round="perfect" of decoder.stream_decode / memory_experiment and
decoder_wide.stream_decode_wide / memory_experiment_wide; the closed instantiations of csrc/uf_stream.hip and csrc/uf_wide.hip), bit
for bit in frame, weight, defect count and growth rounds against tests/closed_uf_ref.py, the wide kernel against the narrow one where both run, and
against properties that need no restatement.  No stream is left out of any comparison."""
import numpy as np
import pytest

import closed_uf_ref as R
import decode_eval_ref as V
import match_st_ref as M
import wide_uf_ref as W

pytestmark = pytest.mark.gpu

SEED = (1234, 5678)
KEYS = ("frame", "weight", "n_defects", "rounds")
PERFECT = dict(final_round="perfect")


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return torch


_envs, _streams, _refs = {}, {}, {}


def _env(dq, d, model="DP", ref=None):
    """One narrow environment per lattice for the module: it supplies the lattice tables (and the referee memory_experiment asks)."""
    key = (d, model, ref)
    if key not in _envs:
        _envs[key] = dq.VectorEnv(n_envs=1, p_phys=0.01, p_meas=0.01, seed=SEED, referee=ref, d=d, error_model=model, use_Y=False, volume_depth=5)
    return _envs[key]


def _sampled(d, T, n, p, closed=True, model="DP", base=0):
    """(syndromes, hidden, trivial) of n streams of T rounds, restated on the host once per shape."""
    key = (d, model, T, n, p, base, closed)
    if key not in _streams:
        _streams[key] = R.sample_streams(d, model, T, n, p, p, SEED, base, closed=closed)
    return _streams[key]


def _reference(d, syn, w, c, key, closed=True):
    """The restatement's (frame, weight, n_defects, rounds, windows), computed once per key and left unchanged."""
    key = (key, w, c, closed)
    if key not in _refs:
        _refs[key] = R.decode(d, syn, w, c, closed)[:5]
    return _refs[key]


def _assert_equal(res, want, windows, tag):
    n = len(want[0])
    for key, w in zip(KEYS, want):
        got = getattr(res, key)
        assert got.dtype == w.dtype and got.shape == w.shape, (tag, key, got.dtype, got.shape)
        bad = np.flatnonzero((got != w).reshape(n, -1).any(axis=1))
        assert bad.size == 0, (tag, key, bad[:8], got[bad[:2]], w[bad[:2]])
    assert res.windows == windows, tag


def _narrow(dq, d, syn, w, c, **kw):
    return dq.decoder.stream_decode(syn, _env(dq, d), window=w, commit=c, to_host=True, **kw)


def _wide(dq, d, syn, w, c, **kw):
    return dq.stream_decode_wide(syn, d, window=w, commit=c, to_host=True, **kw)


def _both_are_the_reference(dq, d, syn, w, c, key):
    """Narrow against the restatement, then wide against narrow."""
    want = _reference(d, syn, w, c, key)
    res = _narrow(dq, d, syn, w, c, **PERFECT)
    _assert_equal(res, want[:4], want[4], ("narrow", key, w, c))
    _assert_equal(_wide(dq, d, syn, w, c, **PERFECT), [getattr(res, k) for k in KEYS], res.windows, ("wide", key, w, c))
    return res


def _d3_patterns():
    if "d3" not in _streams:
        d, T, bits = 3, 3, 12
        n = 1 << bits
        idx = np.arange(n, dtype=np.int64)
        rev = np.zeros_like(idx)
        for b in range(bits):
            rev |= ((idx >> b) & 1) << (bits - 1 - b)
        syn = np.zeros((n, T, d + 1, d + 1), dtype=np.uint8)
        for comp, pat in ((0, idx), (1, rev)):                                   # every pattern of both components appears
            cells = M.Component(d, comp).cells
            assert len(cells) * T == bits
            for t in range(T):
                for j, (a, b) in enumerate(cells):
                    syn[:, t, a, b] = (pat >> (t * len(cells) + j)) & 1
        _streams["d3"] = syn
    return _streams["d3"]


# ---- 1. narrow against the restatement, wide against narrow ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,c", [(2, 1), (3, 3)])
def test_every_pattern_of_d3_three_rounds(dq, torch_mod, w, c):
    syn = _d3_patterns()
    res = _both_are_the_reference(dq, 3, syn, w, c, "d3")
    open_ = _narrow(dq, 3, syn, w, c)
    assert len(np.unique(res.frame.reshape(len(syn), -1), axis=0)) > 50 and res.rounds.max() >= 2           # (not vacuous)
    # at d = 3 every node has a space edge to B, whose id is below its time edge's: the restatement gives the open result for all 4096 patterns, so must the device
    _assert_equal(open_, [getattr(res, k) for k in KEYS], res.windows, ("d3 open", w, c))


@pytest.mark.parametrize("w,c", [(10, 5), (16, 16), (1, 1)])
def test_d5_streams_are_the_reference(dq, torch_mod, w, c):
    syn = _sampled(5, 33, 128, 0.011)[0]
    res = _both_are_the_reference(dq, 5, syn, w, c, "d5")
    assert (res.n_defects.sum(axis=1) > 0).sum() > 64 and res.frame.any()


def test_d7_streams_are_the_reference(dq, torch_mod):
    syn = _sampled(7, 33, 32, 0.02)[0]
    res = _both_are_the_reference(dq, 7, syn, 14, 7, "d7")
    assert (res.n_defects.sum(axis=1) > 0).all() and res.rounds.max() >= 3


@pytest.mark.parametrize("T", [1, 11])
def test_d5_one_round_and_one_round_more_than_the_window(dq, torch_mod, T):
    syn = _sampled(5, T, 128, 0.03)[0]
    res = _both_are_the_reference(dq, 5, syn, 10, 5, ("d5", T))
    assert res.windows == (1 if T == 1 else 2) and res.frame.any()
    if T == 1:                                                                   # code-capacity decoding: every committed edge is a qubit of the frame
        assert np.array_equal(res.weight.sum(axis=1), (res.frame != 0).reshape(128, -1).sum(axis=1) + (res.frame == 2).reshape(128, -1).sum(axis=1))


# ---- 2. wide against the restatement ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,n,T,p,w,c", [(9, 32, 40, 0.01, 18, 9), (9, 32, 40, 0.01, 2, 1), (9, 32, 40, 0.01, 32, 32), (13, 8, 40, 0.01, 26, 13),
                                         (15, 8, 64, 0.01, 30, 15), (15, 4, 32, 0.04, 32, 16)])
def test_wide_lattices_are_the_restatement(dq, torch_mod, d, n, T, p, w, c):
    syn = _sampled(d, T, n, p)[0]
    want = _reference(d, syn, w, c, (d, n, T, p))
    res = _wide(dq, d, syn, w, c, **PERFECT)
    _assert_equal(res, want[:4], want[4], (d, n, T, p, w, c))
    assert (res.n_defects.sum(axis=1) > 0).all() and res.frame.any()
    if p == 0.04:                                                                # the dense case at the LDS maximum
        assert res.n_defects.max() > 500 and res.rounds.max() >= 4
    for comp in range(2):                                                        # sigma(frame) = the last syndrome, on the device's own output
        C = M.Component(d, comp)
        assert np.array_equal((C.plane(res.frame) @ C.H) & 1, C.syndromes(syn)[:, -1]), (d, comp)


# ---- 3. hand cases ---------------------------------------------------------------------------------------------------------------------------------------
def _beside_boundary(C):
    """bool [n]: the node has a space edge to B (a qubit with no other plaquette of the component)."""
    single = C.H.sum(axis=1) == 1
    return C.H[single].sum(axis=0) > 0


def _hand_cases(d):
    """Streams of window + 2 rounds under the default schedule as node bits [K, T, n], the same for both components: nothing; for each of the nodes 0, n - 1,
    32, 64 that exist a lone last-round defect (a syndrome bit set in round T - 1 only) and a same-site pair in rounds T - 2 and T - 1 (a bit set in round
    T - 2 only); then a lone last-round defect on the first bulk node and on the first node beside the boundary."""
    n, w = (d * d - 1) // 2, min(2 * d, 32)
    c, T = (w + 1) // 2, w + 2
    nodes = [u for u in (0, n - 1, 32, 64) if u < n]
    cases, kinds = [np.zeros((T, n), dtype=np.uint8)], [("none", -1)]
    for u in nodes:
        for t, kind in ((T - 1, "lone"), (T - 2, "pair")):
            b = np.zeros((T, n), dtype=np.uint8)
            b[t, u] = 1
            cases.append(b)
            kinds.append((kind, u))
    return np.stack(cases), kinds, T, w, c


@pytest.mark.parametrize("d", [5, 9, 15])
def test_hand_cases(dq, torch_mod, d):
    bits, kinds, T, w, c = _hand_cases(d)
    K = len(bits)
    for comp in range(2):
        C = M.Component(d, comp)
        beside = _beside_boundary(C)
        extra = []
        for want_beside in (False, True):                                        # one node of each kind, whatever the four fixed nodes are
            u = int(np.flatnonzero(beside == want_beside)[0])
            b = np.zeros((T, C.n), dtype=np.uint8)
            b[T - 1, u] = 1
            extra.append(b)
        all_bits = np.concatenate([bits, np.stack(extra)])
        all_kinds = kinds + [("lone", int(np.flatnonzero(~beside)[0])), ("lone", int(np.flatnonzero(beside)[0]))]
        syn = W.node_syndromes(d, comp, all_bits)
        want = _reference(d, syn, w, c, ("hand", d, comp))
        res = _wide(dq, d, syn, w, c, **PERFECT)
        _assert_equal(res, want[:4], want[4], ("hand", d, comp))
        open_ = _wide(dq, d, syn, w, c)
        if d <= 7:
            _assert_equal(_narrow(dq, d, syn, w, c, **PERFECT), want[:4], want[4], ("hand narrow", d, comp))
        plane = C.plane(res.frame)
        assert not res.frame[0].any() and not res.weight[0].any() and not res.rounds[0].any() and K + 2 == len(all_kinds)
        assert not res.weight[:, 1 - comp].any() and not res.n_defects[:, 1 - comp].any()
        seen = set()
        for k, (kind, u) in enumerate(all_kinds):
            if kind == "pair":                                                   # one time edge between the two, no qubit, in both forms
                assert res.weight[k, comp] == 1 and res.n_defects[k, comp] == 2 and not res.frame[k].any() and not open_.frame[k].any(), (d, comp, u)
            elif kind == "lone":
                assert res.n_defects[k, comp] == 1 and np.array_equal((plane[k] @ C.H) & 1, np.eye(C.n, dtype=np.int64)[u]), (d, comp, u)
                assert res.weight[k, comp] == plane[k].sum() >= 1                # space edges only, as many as the frame has qubits
                assert open_.weight[k, comp] == 1
                if beside[u]:                                                    # one space edge to B, in both forms (its id is below the time edge's)
                    assert plane[k].sum() == 1 and np.array_equal(open_.frame[k], res.frame[k]), (d, comp, u)
                else:                                                            # open: the time edge to B and no qubit; closed: a path of space edges to B
                    assert not open_.frame[k].any() and plane[k].sum() >= 2, (d, comp, u)
                seen.add(bool(beside[u]))
        assert seen == {False, True}


# ---- 4. the samplers -------------------------------------------------------------------------------------------------------------------------------------
def _check_run(torch, dq, d, model, T, n, run, decode):
    """run(final_round, ph, pm, hid, triv, frame, outs, syn) launches; decode(syn) is the closed decode of syndromes on the host."""
    base = 4_294_967_290                                                         # the lattice ids wrap
    for each in (False, True):
        ph = np.linspace(0.004, 0.03, n) if each else 0.02
        pm = ph[::-1].copy() if each else 0.01
        want_syn, want_hid, want_triv = R.sample_streams(d, model, T, n, ph, pm, SEED, base, closed=True)
        got = {}
        for mode, with_syn in (("perfect", True), ("perfect", False), ("faulty", True)):
            hid = torch.zeros((n, d, d), dtype=torch.uint8, device="cuda")
            frame = torch.full((n, d, d), 9, dtype=torch.uint8, device="cuda")
            triv = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
            outs = [torch.zeros((n, 2), dtype=torch.int32, device="cuda") for _ in range(3)]
            syn = torch.full((n, T, d + 1, d + 1), 9, dtype=torch.uint8, device="cuda") if with_syn else None
            run(mode, ph, pm, hid, triv, frame, outs, syn)
            torch.cuda.synchronize()
            got[(mode, with_syn)] = [x.cpu().numpy() for x in [hid, triv, frame] + outs] + [None if syn is None else syn.cpu().numpy()]
        tag = (d, model, each)
        for with_syn in (True, False):
            hid, triv = got[("perfect", with_syn)][:2]
            assert np.array_equal(hid, want_hid) and np.array_equal(triv, want_triv), tag
        closed_syn, open_run = got[("perfect", True)][6], got[("faulty", True)]
        assert np.array_equal(closed_syn, want_syn), tag
        assert np.array_equal(open_run[0], want_hid) and np.array_equal(open_run[6][:, :-1], want_syn[:, :-1]), tag
        assert (open_run[6][:, -1] != want_syn[:, -1]).any(), tag               # (the open run does flip its last round)
        dec = decode(closed_syn)
        for with_syn in (True, False):
            for key, x in zip(KEYS, got[("perfect", with_syn)][2:6]):
                assert np.array_equal(x, getattr(dec, key)), (tag, with_syn, key)
        assert want_hid.any() and dec.frame.any(), tag


@pytest.mark.parametrize("model", ["X", "DP", "IIDXZ"])
def test_narrow_closed_run_samples_the_restated_rounds_and_decodes_them(dq, torch_mod, model):
    D = dq.decoder
    d, T, n, w, c = 5, 12, 48, 10, 5
    env = _env(dq, d, model)
    ev = D.Evaluator(d, model, False, w, chunk=n, device=env.device)
    try:
        def run(mode, ph, pm, hid, triv, frame, outs, syn):
            ev.stream_run_into(env, n, T, c, 4_294_967_290, SEED, ph, pm, hid, triv, frame, *outs, syndromes=syn, final_round=mode)
        _check_run(torch_mod, dq, d, model, T, n, run, lambda syn: D.stream_decode(syn, env, window=w, commit=c, evaluator=ev, to_host=True, **PERFECT))
    finally:
        ev.close()


@pytest.mark.parametrize("d,T,n", [(5, 12, 48), (9, 12, 48), (15, 6, 24)])
@pytest.mark.parametrize("model", ["X", "DP", "IIDXZ"])
def test_wide_closed_run_samples_the_restated_rounds_and_decodes_them(dq, torch_mod, d, T, n, model):
    w = min(2 * d, 32)
    c = (w + 1) // 2
    ev = dq.WideEvaluator(d, model, w, chunk=n)
    try:
        def run(mode, ph, pm, hid, triv, frame, outs, syn):
            ev.run_into(n, T, c, 4_294_967_290, SEED, ph, pm, hid, triv, frame, *outs, syndromes=syn, final_round=mode)
        _check_run(torch_mod, dq, d, model, T, n, run, lambda syn: dq.stream_decode_wide(syn, d, window=w, commit=c, evaluator=ev, to_host=True, **PERFECT))
    finally:
        ev.close()


# ---- 5. invariants that are not taken from the restatement ---------------------------------------------------------------------------------------------
def _experiment(dq, d, n, T, p, **kw):
    if d <= 7:
        return dq.decoder.memory_experiment(_env(dq, d, "DP", ref="lut"), n, T, p_phys=p, seed=SEED, **kw)
    return dq.memory_experiment_wide((d, "DP"), n, T, p_phys=p, seed=SEED, **kw)


@pytest.mark.parametrize("d", [5, 9])
def test_every_closed_residual_is_in_the_code_space(dq, torch_mod, d):
    n, T, p = 2048, 24, 0.012
    closed = _experiment(dq, d, n, T, p, **PERFECT)
    open_ = _experiment(dq, d, n, T, p)
    assert closed.counters["volumes"] == n and closed.counters["in_codespace"] == n
    assert open_.counters["volumes"] == n and open_.counters["in_codespace"] < n


def _single_faults(d, T):
    """Every X / Y / Z data error per round and qubit and every misreading of rounds 0 .. T - 2, one per stream, as (syndromes, hidden)."""
    from oracle import lattice
    d2, ns = d * d, lattice.Masks(d).n_stab
    xs, zs, flips = [], [], []
    for j in range(T):
        for q in range(d2):
            for code in (1, 2, 3):
                x, z = np.zeros((T, d2), dtype=np.int64), np.zeros((T, d2), dtype=np.int64)
                if code in (1, 2):
                    x[j:, q] = 1
                if code in (2, 3):
                    z[j:, q] = 1
                xs.append(x), zs.append(z), flips.append(np.zeros((T, ns), dtype=np.int64))
    for j in range(T - 1):
        for s in range(ns):
            f = np.zeros((T, ns), dtype=np.int64)
            f[j, s] = 1
            xs.append(np.zeros((T, d2), dtype=np.int64)), zs.append(np.zeros((T, d2), dtype=np.int64)), flips.append(f)
    x, z, f = np.stack(xs), np.stack(zs), np.stack(flips)
    N = len(x)
    bits = V.syndrome_bits(d, x.reshape(N * T, d2), z.reshape(N * T, d2)).reshape(N, T, ns) ^ f
    return V.bits_to_grids(d, bits), V.xz_to_codes(d, x[:, -1], z[:, -1])


def test_no_single_fault_defeats_the_closed_decoder_at_d5(dq, torch_mod):
    d, T = 5, 4
    syn, hidden = _single_faults(d, T)
    assert len(syn) == 372
    for w, c in ((4, 4), (2, 1)):
        for name, res in (("narrow", _narrow(dq, d, syn, w, c, **PERFECT)), ("wide", _wide(dq, d, syn, w, c, **PERFECT))):
            v = V.verdict(d, hidden, res.frame, W.classify_none)
            bad = np.flatnonzero((v & V.SUCCESS) == 0)
            assert bad.size == 0, (name, w, c, bad[:8])


# ---- 6. one sanity row -----------------------------------------------------------------------------------------------------------------------------------
def test_closed_failure_falls_with_the_distance(dq, torch_mod):
    """8192 DP streams of 24 rounds at p = 0.012 under the default windows.  The CPU restatement on component-wise sampled streams gave 0.039 at d = 5 and
    0.0023 at d = 9, a factor of 17; a quarter leaves room for that sampling and for the noise of 8192 streams."""
    n, T, p = 8192, 24, 0.012
    rate = {}
    for d in (5, 9):
        for mode in ("perfect", "faulty"):
            r = _experiment(dq, d, n, T, p, final_round=mode)
            assert r.counters["volumes"] == n
            rate[(d, mode)] = r.failure_rate
            print(f"d = {d}, final round {mode}: failure {r.failure_rate:.5f} {r.failure_interval}")
    assert rate[(9, "perfect")] < rate[(5, "perfect")] / 4
    assert rate[(5, "perfect")] < rate[(5, "faulty")] and rate[(9, "perfect")] < rate[(9, "faulty")]


# ---- 7. the open forms are untouched by closed calls on the same handle ------------------------------------------------------------------------------
def test_open_forms_return_the_same_bits_around_closed_calls(dq, torch_mod):
    D = dq.decoder
    d5, n = _sampled(5, 33, 128, 0.011)[0], 128
    d9 = _sampled(9, 40, 32, 0.01)[0]
    env = _env(dq, 5)
    nv = D.Evaluator(5, "DP", False, 10, chunk=n, device=env.device)
    wv = dq.WideEvaluator(9, "DP", 18, chunk=32)
    try:
        before = (D.stream_decode(d5, env, window=10, commit=5, evaluator=nv, to_host=True), _wide(dq, 9, d9, 18, 9, evaluator=wv))
        for chunk in (1, 7, n):
            _assert_equal(_narrow(dq, 5, d5, 10, 5, chunk=chunk, **PERFECT), _reference(5, d5, 10, 5, "d5")[:4], 6, ("narrow chunk", chunk))
            _assert_equal(_wide(dq, 9, d9, 18, 9, chunk=chunk, **PERFECT), _reference(9, d9, 18, 9, (9, 32, 40, 0.01))[:4], 4, ("wide chunk", chunk))
        closed = (D.stream_decode(d5, env, window=10, commit=5, evaluator=nv, to_host=True, **PERFECT), _wide(dq, 9, d9, 18, 9, evaluator=wv, **PERFECT))
        after = (D.stream_decode(d5, env, window=10, commit=5, evaluator=nv, to_host=True), _wide(dq, 9, d9, 18, 9, evaluator=wv))
        for b, cl, a, name in zip(before, closed, after, ("narrow", "wide")):
            for k in KEYS:
                assert np.array_equal(getattr(b, k), getattr(a, k)), (name, k)
            assert (cl.frame != b.frame).any(), name
        for res, d, syn, w, c in ((before[0], 5, d5, 10, 5), (before[1], 9, d9, 18, 9)):      # and those bits are the open restatement's
            want = W.decode(d, syn, w, c)
            _assert_equal(res, want[:4], want[4], ("open", d))
    finally:
        nv.close()
        wv.close()


def test_a_small_handle_does_not_lower_a_large_ones_lds_for_the_closed_kernels(dq, torch_mod):
    d, n, T, p, w, c = 15, 4, 32, 0.04, 32, 16
    syn = _sampled(d, T, n, p)[0]
    want = _reference(d, syn, w, c, (d, n, T, p))
    small = dq.WideEvaluator(3, "DP", 2, chunk=n)
    large = dq.WideEvaluator(d, "DP", w, chunk=n)
    try:
        tiny = dq.stream_decode_wide(np.zeros((n, 4, 4, 4), dtype=np.uint8), 3, window=2, commit=1, evaluator=small, to_host=True, **PERFECT)
        assert not tiny.frame.any()
        _assert_equal(_wide(dq, d, syn, w, c, evaluator=large, **PERFECT), want[:4], want[4], "large after small")
        _assert_equal(_wide(dq, d, syn, w, c, evaluator=large), W.decode(d, syn, w, c)[:4], 1, "large, open")
    finally:
        small.close()
        large.close()
