"""Weighted union-find on the device (decoder_wide weights=; dq_wide_uf_decode_weighted / dq_wide_uf_run_weighted; the Weighted instantiations of
csrc/uf_wide.hip), bit for bit in frame, weight, defect count and growth rounds against tests/weighted_uf_ref.py, whose growth is
stepwise while the device jumps from event to event; against the unweighted entry points at (1, 1); and the per-stream array, the fused run and the
experiment against the plain launches they must equal.  No stream is left out of any comparison."""
import numpy as np
import pytest

import match_st_ref as M
import weighted_uf_ref as WR

pytestmark = pytest.mark.gpu

SEED = (1234, 5678)
KEYS = ("frame", "weight", "n_defects", "rounds")


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return torch


_streams, _refs = {}, {}


def _sampled(d, T, n, p, pm=None, model="DP", base=0, closed=False):
    """Syndromes of n streams of T rounds, restated on the host once per shape."""
    key = (d, model, T, n, p, pm, base, closed)
    if key not in _streams:
        _streams[key] = WR.sample_streams(d, model, T, n, p, p if pm is None else pm, SEED, base, closed=closed)[0]
    return _streams[key]


def _reference(d, syn, w, c, closed, weights, key):
    """The restatement's (frame, weight, n_defects, rounds, windows), computed once per key and left unchanged."""
    key = (key, w, c, closed, tuple(np.asarray(weights).reshape(-1).tolist()))
    if key not in _refs:
        _refs[key] = WR.decode(d, syn, w, c, closed, weights)
    return _refs[key]


def _assert_equal(res, want, windows, tag):
    n = len(want[0])
    for key, w in zip(KEYS, want):
        got = getattr(res, key)
        assert got.dtype == w.dtype and got.shape == w.shape, (tag, key, got.dtype, got.shape)
        bad = np.flatnonzero((got != w).reshape(n, -1).any(axis=1))
        assert bad.size == 0, (tag, key, bad[:8], got[bad[:2]], w[bad[:2]])
    assert res.windows == windows, tag


def _same_results(a, b, tag):
    _assert_equal(a, [getattr(b, k) for k in KEYS], b.windows, tag)


def _wide(dq, d, syn, w, c, closed=False, **kw):
    return dq.stream_decode_wide(syn, d, window=w, commit=c, to_host=True, final_round="perfect" if closed else "faulty", **kw)


def _d3_patterns():
    """Every 12-bit pattern of three rounds of d = 3, in both components (tests/test_closed_uf_gpu.py enumerates them the same way)."""
    if "d3" not in _streams:
        d, T, bits = 3, 3, 12
        n = 1 << bits
        idx = np.arange(n, dtype=np.int64)
        rev = np.zeros_like(idx)
        for b in range(bits):
            rev |= ((idx >> b) & 1) << (bits - 1 - b)
        syn = np.zeros((n, T, d + 1, d + 1), dtype=np.uint8)
        for comp, pat in ((0, idx), (1, rev)):
            cells = M.Component(d, comp).cells
            assert len(cells) * T == bits
            for t in range(T):
                for j, (a, b) in enumerate(cells):
                    syn[:, t, a, b] = (pat >> (t * len(cells) + j)) & 1
        _streams["d3"] = syn
    return _streams["d3"]


# ---- 1. the device against the stepwise restatement ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("closed", [False, True])
@pytest.mark.parametrize("pair", [(1, 1), (1, 2), (2, 1), (3, 2), (15, 1), (1, 15)])
def test_every_pattern_of_d3_three_rounds(dq, torch_mod, pair, closed):
    syn = _d3_patterns()
    for w, c in ((3, 3), (2, 1)):
        want = _reference(3, syn, w, c, closed, pair, "d3")
        res = _wide(dq, 3, syn, w, c, closed, weights=pair)
        _assert_equal(res, want[:4], want[4], ("d3", pair, closed, w, c))
    assert res.rounds.max() >= 2 * min(pair)                                                                           # (not vacuous)
    if pair != (15, 1):                                      # (there a time edge to the open boundary is always the cheapest way out: no qubit is corrected)
        assert len(np.unique(res.frame.reshape(len(syn), -1), axis=0)) > 50
    assert (res.weight.sum(axis=1) > 0).sum() > 4000


@pytest.mark.parametrize("d,p", [(5, 0.02), (7, 0.015), (9, 0.01)])
@pytest.mark.parametrize("w,c", [(2, 1), (10, 5), (32, 32)])
@pytest.mark.parametrize("pair", [(2, 1), (3, 2), (5, 8)])
def test_sampled_streams_are_the_restatement(dq, torch_mod, d, p, w, c, pair):
    """32 streams of 40 rounds (24 under window 2, where every round is a window); the closed form on streams drawn with a perfect last round."""
    T = 24 if w == 2 else 40
    for closed in (False, True):
        syn = _sampled(d, T, 32, p, closed=closed)
        want = _reference(d, syn, w, c, closed, pair, (d, T, closed))
        res = _wide(dq, d, syn, w, c, closed, weights=pair)
        _assert_equal(res, want[:4], want[4], (d, w, c, pair, closed))
        assert (res.n_defects.sum(axis=1) > 0).sum() >= 28 and res.frame.any() and res.rounds.max() >= 2 * min(pair)


@pytest.mark.parametrize("d,n,T,p,w,c", [(13, 8, 40, 0.01, 32, 16), (15, 4, 32, 0.04, 32, 16), (15, 4, 40, 0.01, 32, 8)])
@pytest.mark.parametrize("pair", [(3, 2), (1, 4)])
def test_large_lattices_at_the_lds_maximum_are_the_restatement(dq, torch_mod, d, n, T, p, w, c, pair):
    syn = _sampled(d, T, n, p)
    for closed in (False, True):
        want = _reference(d, syn, w, c, closed, pair, (d, n, T, p))
        res = _wide(dq, d, syn, w, c, closed, weights=pair)
        _assert_equal(res, want[:4], want[4], (d, n, T, p, w, c, pair, closed))
        assert (res.n_defects.sum(axis=1) > 0).all() and res.frame.any()
        if p == 0.04:                                                            # the dense case: 32 rounds of d = 15 in one window
            assert res.n_defects.max() > 500 and res.rounds.max() >= 4
        if closed:                                                               # sigma(frame) = the last syndrome, on the device's own output
            for comp in range(2):
                C = M.Component(d, comp)
                assert np.array_equal((C.plane(res.frame) @ C.H) & 1, C.syndromes(syn)[:, -1]), (d, comp)


# ---- 2. unit weights are the unweighted kernels -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,n,T,p,w,c", [(5, 64, 33, 0.02, 10, 5), (9, 32, 40, 0.01, 18, 9), (15, 4, 32, 0.04, 32, 16), (3, 64, 9, 0.05, 1, 1)])
def test_unit_weights_equal_the_unweighted_entry_points(dq, torch_mod, d, n, T, p, w, c):
    syn = _sampled(d, T, n, p)
    for closed in (False, True):
        plain = _wide(dq, d, syn, w, c, closed)
        _same_results(_wide(dq, d, syn, w, c, closed, weights=(1, 1)), plain, (d, closed, "pair"))
        _same_results(_wide(dq, d, syn, w, c, closed, weights=np.ones((n, 2), dtype=np.int64)), plain, (d, closed, "array"))
        assert plain.frame.any() and plain.rounds.max() >= 2


# ---- 3. a pair per stream -------------------------------------------------------------------------------------------------------------------------------------
def test_a_pair_per_stream_equals_the_uniform_launches(dq, torch_mod):
    d, n, T, w, c = 9, 48, 24, 18, 9
    syn = _sampled(d, T, n, 0.012)
    kinds = [(1, 1), (2, 1), (3, 2), (1, 4), (15, 15), (8, 5)]
    rng = np.random.default_rng(5)
    for closed in (False, True):
        uniform = {pr: _wide(dq, d, syn, w, c, closed, weights=pr) for pr in kinds}
        assert any((uniform[kinds[0]].frame != uniform[pr].frame).any() for pr in kinds[1:])        # (the weights do change corrections)
        which = np.arange(n) % len(kinds)
        for trial in range(2):
            pairs = np.array([kinds[k] for k in which])
            for chunk in (1, 7, n):
                res = _wide(dq, d, syn, w, c, closed, weights=pairs, chunk=chunk)
                for key in KEYS:
                    want = np.stack([getattr(uniform[kinds[k]], key)[i] for i, k in enumerate(which)])
                    assert np.array_equal(getattr(res, key), want), (closed, trial, chunk, key)
            order = rng.permutation(n)                                           # the same streams and pairs in another batch order
            res = _wide(dq, d, syn[order], w, c, closed, weights=pairs[order], chunk=7)
            for key in KEYS:
                want = np.stack([getattr(uniform[kinds[which[i]]], key)[i] for i in order])
                assert np.array_equal(getattr(res, key), want), (closed, trial, "permuted", key)
            which = rng.integers(0, len(kinds), n)


# ---- 4. the fused run ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,T,n,model", [(5, 12, 48, "DP"), (9, 12, 48, "X"), (15, 6, 24, "IIDXZ")])
def test_weighted_run_samples_what_the_plain_run_samples_and_decodes_it(dq, torch_mod, d, T, n, model):
    torch = torch_mod
    w = min(2 * d, 32)
    c = (w + 1) // 2
    base = 4_294_967_290                                                         # the lattice ids wrap
    ev = dq.WideEvaluator(d, model, w, chunk=n)
    try:
        for each in (False, True):
            ph = np.linspace(0.004, 0.03, n) if each else 0.02
            pm = ph[::-1].copy() if each else 0.05
            pairs = np.array([(1 + i % 3, 1 + i % 4) for i in range(n)], dtype=np.uint8)
            for mode in ("faulty", "perfect"):
                def run(weights):
                    hid = torch.zeros((n, d, d), dtype=torch.uint8, device="cuda")
                    frame = torch.full((n, d, d), 9, dtype=torch.uint8, device="cuda")
                    triv = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
                    outs = [torch.zeros((n, 2), dtype=torch.int32, device="cuda") for _ in range(3)]
                    syn = torch.full((n, T, d + 1, d + 1), 9, dtype=torch.uint8, device="cuda")
                    kw = {} if weights is None else dict(weights=weights)
                    ev.run_into(n, T, c, base, SEED, ph, pm, hid, triv, frame, *outs, syndromes=syn, final_round=mode, **kw)
                    torch.cuda.synchronize()
                    return [x.cpu().numpy() for x in [hid, triv, syn, frame] + outs]
                plain = run(None)
                for weights in ((3, 2), torch.from_numpy(pairs).cuda()):
                    got = run(weights)
                    for k in range(3):                                           # hidden, trivial and the syndromes are the unweighted run's
                        assert np.array_equal(got[k], plain[k]), (d, model, each, mode, k)
                    host = (3, 2) if isinstance(weights, tuple) else pairs
                    dec = dq.stream_decode_wide(got[2], d, window=w, commit=c, evaluator=ev, to_host=True, final_round=mode, weights=host)
                    for key, x in zip(KEYS, got[3:]):
                        assert np.array_equal(x, getattr(dec, key)), (d, model, each, mode, key)
                    assert dec.frame.any() and plain[0].any()
                one = run((1, 1))
                for k in range(7):
                    assert np.array_equal(one[k], plain[k]), (d, model, each, mode, k)
    finally:
        ev.close()


# ---- 5. the experiment ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(), dict(final_round="perfect", referee="matching", no_decoder=True)])
def test_experiment_with_weights_from_the_rates_equals_one_call_per_rate(dq, torch_mod, kw):
    DW = dq.decoder_wide
    d, n, T = 9, 512, 12
    rates, meas = [0.004, 0.008, 0.02], [0.04, 0.008, 0.001]
    both = DW.memory_experiment_wide((d, "DP"), n, T, rates=rates, p_meas=meas, seed=SEED, weights="rates", chunk=700, **kw)
    assert list(both) == rates
    pairs = [DW.uf_weights(a, b, "DP") for a, b in zip(rates, meas)]
    assert len(set(pairs)) == 3
    differs = []
    for k, (a, b) in enumerate(zip(rates, meas)):
        one = DW.memory_experiment_wide((d, "DP"), n, T, p_phys=a, p_meas=b, seed=SEED, env_id_base=k * n, weights=pairs[k], **kw)
        by_rate = DW.memory_experiment_wide((d, "DP"), n, T, p_phys=a, p_meas=b, seed=SEED, env_id_base=k * n, weights="rates", **kw)
        unit = DW.memory_experiment_wide((d, "DP"), n, T, p_phys=a, p_meas=b, seed=SEED, env_id_base=k * n, **kw)
        assert both[a].counters == one.counters == by_rate.counters and both[a].inexact == one.inexact, (a, both[a].counters, one.counters)
        assert both[a].weights == one.weights == by_rate.weights == pairs[k] and unit.weights is None
        assert one.counters["volumes"] == n and 0 < one.counters["success"]
        if "no_decoder" in kw:
            assert both[a].no_decoder.counters == one.no_decoder.counters == unit.no_decoder.counters
        differs.append(one.counters != unit.counters)
    assert any(differs)                                                          # (the pairs do decode differently from unit weights)


# ---- 6. the unweighted forms are untouched by weighted calls on the same handle ------------------------------------------------------------------------------
def test_unweighted_results_are_the_same_around_weighted_calls(dq, torch_mod):
    d, n, T, w, c = 9, 32, 40, 18, 9
    syn = _sampled(d, T, n, 0.01)
    ev = dq.WideEvaluator(d, "DP", w, chunk=n)
    try:
        before = [_wide(dq, d, syn, w, c, closed, evaluator=ev) for closed in (False, True)]
        weighted = [_wide(dq, d, syn, w, c, closed, evaluator=ev, weights=(3, 2)) for closed in (False, True)]
        after = [_wide(dq, d, syn, w, c, closed, evaluator=ev) for closed in (False, True)]
        for b, wt, a, closed in zip(before, weighted, after, (False, True)):
            _same_results(a, b, ("around", closed))
            assert (wt.frame != b.frame).any() and (wt.rounds != b.rounds).any(), closed
            want = _reference(d, syn, w, c, closed, (3, 2), (d, n, T, 0.01))
            _assert_equal(wt, want[:4], want[4], ("weighted on the handle", closed))
    finally:
        ev.close()
