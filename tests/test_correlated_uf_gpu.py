"""Correlated union-find on the device (decoder_wide correlated=; dq_wide_uf_decode_correlated / dq_wide_uf_run_correlated; the Corr instantiations of
csrc/uf_wide.hip), bit for bit in frame, weight, defect count and growth rounds against tests/correlated_uf_ref.py, whose growth is
stepwise and whose weights are an array per edge; against the weighted entry points at w_corr = w_space; and the per-stream array, the fused run and the
experiment against the plain launches they must equal.  Sampled streams are DP at p = p_meas = 0.03, so that the masks are not empty: every sampled set
holds a stream whose frame differs from the weighted launch's.  No stream is left out of any comparison."""
import numpy as np
import pytest

import correlated_uf_ref as CR
import match_st_ref as M

pytestmark = pytest.mark.gpu

SEED = (1234, 5678)
KEYS = ("frame", "weight", "n_defects", "rounds")
P = 0.03


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return torch


_streams, _refs = {}, {}


def _sampled(d, T, n, model="DP", closed=False):
    """Syndromes of n streams of T rounds, restated on the host once per shape."""
    key = (d, model, T, n, closed)
    if key not in _streams:
        _streams[key] = CR.sample_streams(d, model, T, n, P, P, SEED, 0, closed=closed)[0]
    return _streams[key]


def _reference(d, syn, w, c, closed, triple, key):
    """The restatement's (frame, weight, n_defects, rounds, windows), computed once per key and left unchanged."""
    key = (key, w, c, closed, tuple(np.asarray(triple).reshape(-1).tolist()))
    if key not in _refs:
        _refs[key] = CR.decode(d, syn, w, c, closed, triple)
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


def _wide(dq, d, syn, w, c, closed=False, triple=None, **kw):
    if triple is not None:
        kw.update(weights=tuple(triple[:2]), correlated=int(triple[2]))
    return dq.stream_decode_wide(syn, d, window=w, commit=c, to_host=True, final_round="perfect" if closed else "faulty", **kw)


def _differs(a, b):
    """The number of streams whose frames differ."""
    return int((a.frame != b.frame).reshape(len(a.frame), -1).any(axis=1).sum())


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
@pytest.mark.parametrize("triple", [(4, 4, 1), (2, 1, 1), (3, 2, 2), (15, 1, 1), (15, 15, 1)])
def test_every_pattern_of_d3_three_rounds(dq, torch_mod, triple, closed):
    syn = _d3_patterns()
    # (the sliding schedule with the small weights only: the restatement walks 30 unit steps per filled edge of weight 15)
    for w, c in ((3, 3), (2, 1)) if max(triple) <= 4 else ((3, 3),):
        want = _reference(3, syn, w, c, closed, triple, "d3")
        res = _wide(dq, 3, syn, w, c, closed, triple)
        _assert_equal(res, want[:4], want[4], ("d3", triple, closed, w, c))
        assert res.rounds.max() >= 2 * min(triple[:2]) and (res.weight.sum(axis=1) > 0).sum() > 4000                        # (not vacuous)
        if triple[2] < triple[0] and triple[:2] != (15, 1):     # (at (15, 1) a time edge is always the cheapest way out: no qubit is corrected)
            assert _differs(res, _wide(dq, 3, syn, w, c, closed, weights=triple[:2])) > 0


@pytest.mark.parametrize("d", [5, 7, 9])
@pytest.mark.parametrize("w,c", [(2, 1), (10, 5), (32, 32)])
@pytest.mark.parametrize("triple", [(4, 4, 1), (7, 4, 1), (8, 7, 2)])
def test_sampled_streams_are_the_restatement(dq, torch_mod, d, w, c, triple):
    """32 streams: 12 rounds under window 2 (every round a window), 20 under (10, 5) (three windows), 36 under (32, 32) (two windows); the closed form on
    streams drawn with a perfect last round."""
    T = {2: 12, 10: 20, 32: 36}[w]
    for closed in (False, True):
        syn = _sampled(d, T, 32, closed=closed)
        want = _reference(d, syn, w, c, closed, triple, (d, T, closed))
        res = _wide(dq, d, syn, w, c, closed, triple)
        _assert_equal(res, want[:4], want[4], (d, w, c, triple, closed))
        assert (res.n_defects.sum(axis=1) > 0).sum() >= 28 and res.frame.any() and res.rounds.max() >= 2 * min(triple[:2])
        # not vacuous: the masks changed some stream's correction (on the restatement's own frames too)
        weighted = _wide(dq, d, syn, w, c, closed, weights=triple[:2])
        assert _differs(res, weighted) >= 1 and (want[0] != weighted.frame).any(), (d, w, c, triple, closed)


@pytest.mark.parametrize("d,n,T,w,c", [(13, 8, 36, 32, 16), (15, 4, 32, 32, 32), (15, 4, 36, 32, 8)])
def test_large_lattices_at_the_lds_maximum_are_the_restatement(dq, torch_mod, d, n, T, w, c):
    """d = 15 with window 32 is the LDS maximum: 63 152 bytes of the layout and 2 048 of the two masks."""
    syn = _sampled(d, T, n)
    triple = (4, 4, 1)
    for closed in (False, True):
        want = _reference(d, syn, w, c, closed, triple, (d, n, T))
        res = _wide(dq, d, syn, w, c, closed, triple)
        _assert_equal(res, want[:4], want[4], (d, n, T, w, c, closed))
        assert (res.n_defects.sum(axis=1) > 0).all() and res.frame.any()
        assert _differs(res, _wide(dq, d, syn, w, c, closed, weights=triple[:2])) >= 1


# ---- 2. w_corr = w_space is the weighted launch ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,n,T,w,c", [(5, 64, 33, 10, 5), (9, 32, 40, 18, 9), (15, 4, 32, 32, 16), (3, 64, 9, 1, 1)])
def test_w_corr_equal_to_w_space_is_the_weighted_launch(dq, torch_mod, d, n, T, w, c):
    syn = _sampled(d, T, n)
    for closed in (False, True):
        for pair in ((4, 4), (3, 2), (1, 1)):
            weighted = _wide(dq, d, syn, w, c, closed, weights=pair)
            _same_results(_wide(dq, d, syn, w, c, closed, pair + (pair[0],)), weighted, (d, closed, pair, "triple"))
            each = np.tile(np.array(pair, dtype=np.int64), (n, 1))
            _same_results(_wide(dq, d, syn, w, c, closed, weights=each, correlated=pair[0]), weighted, (d, closed, pair, "array"))
            assert weighted.frame.any() and weighted.rounds.max() >= 2


# ---- 3. a triple per stream -----------------------------------------------------------------------------------------------------------------------------------
def test_a_triple_per_stream_equals_the_uniform_launches(dq, torch_mod):
    """Through the evaluator, whose decode_into takes a uint8 device tensor [m, 3]: permuted, in chunks of 1, 7 and n."""
    torch = torch_mod
    d, n, T, w, c = 9, 48, 24, 18, 9
    syn = _sampled(d, T, n)
    kinds = [(4, 4, 1), (4, 4, 4), (7, 4, 1), (8, 7, 2), (15, 15, 1), (1, 1, 1)]
    rng = np.random.default_rng(5)
    ev = dq.WideEvaluator(d, "DP", w, chunk=n)

    def run(s, triples, chunk, closed):
        dev = torch.from_numpy(np.ascontiguousarray(s)).cuda()
        tri = torch.from_numpy(np.ascontiguousarray(triples.astype(np.uint8))).cuda()
        frame = torch.full((n, d, d), 9, dtype=torch.uint8, device="cuda")
        outs = [torch.full((n, 2), -1, dtype=torch.int32, device="cuda") for _ in range(3)]
        for a in range(0, n, chunk):
            m = min(chunk, n - a)
            ev.decode_into(dev[a:a + m], m, T, c, frame[a:a + m], *(x[a:a + m] for x in outs), final_round="perfect" if closed else "faulty",
                           weights=tri[a:a + m])
        torch.cuda.synchronize()
        return [x.cpu().numpy() for x in [frame] + outs]

    try:
        for closed in (False, True):
            uniform = {tr: _wide(dq, d, syn, w, c, closed, tr, evaluator=ev) for tr in kinds}
            assert _differs(uniform[(4, 4, 1)], uniform[(4, 4, 4)]) >= 1                  # (w_corr does change corrections)
            which = np.arange(n) % len(kinds)
            for trial in range(2):
                triples = np.array([kinds[k] for k in which])
                for chunk in (1, 7, n):
                    got = run(syn, triples, chunk, closed)
                    for key, x in zip(KEYS, got):
                        want = np.stack([getattr(uniform[kinds[k]], key)[i] for i, k in enumerate(which)])
                        assert np.array_equal(x, want), (closed, trial, chunk, key)
                order = rng.permutation(n)                                        # the same streams and triples in another batch order
                got = run(syn[order], triples[order], 7, closed)
                for key, x in zip(KEYS, got):
                    want = np.stack([getattr(uniform[kinds[which[i]]], key)[i] for i in order])
                    assert np.array_equal(x, want), (closed, trial, "permuted", key)
                which = rng.integers(0, len(kinds), n)
    finally:
        ev.close()


# ---- 4. the fused run -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,T,n,model", [(5, 12, 48, "DP"), (9, 12, 48, "X"), (15, 6, 24, "IIDXZ")])
def test_correlated_run_samples_what_the_weighted_run_samples_and_decodes_it(dq, torch_mod, d, T, n, model):
    torch = torch_mod
    w = min(2 * d, 32)
    c = (w + 1) // 2
    base = 4_294_967_290                                                         # the lattice ids wrap
    ev = dq.WideEvaluator(d, model, w, chunk=n)
    try:
        for each in (False, True):
            ph = np.linspace(0.01, 0.04, n) if each else P
            pm = ph[::-1].copy() if each else P
            triples = np.array([(3 + i % 3, 1 + i % 4, 1 + i % 3) for i in range(n)], dtype=np.uint8)
            for mode in ("faulty", "perfect"):
                def run(weights):
                    hid = torch.zeros((n, d, d), dtype=torch.uint8, device="cuda")
                    frame = torch.full((n, d, d), 9, dtype=torch.uint8, device="cuda")
                    triv = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
                    outs = [torch.zeros((n, 2), dtype=torch.int32, device="cuda") for _ in range(3)]
                    syn = torch.full((n, T, d + 1, d + 1), 9, dtype=torch.uint8, device="cuda")
                    ev.run_into(n, T, c, base, SEED, ph, pm, hid, triv, frame, *outs, syndromes=syn, final_round=mode, weights=weights)
                    torch.cuda.synchronize()
                    return [x.cpu().numpy() for x in [hid, triv, syn, frame] + outs]
                weighted = run((4, 4))
                for weights in ((4, 4, 1), torch.from_numpy(triples).cuda()):
                    got = run(weights)
                    for k in range(3):                                           # hidden, trivial and the syndromes are the weighted run's
                        assert np.array_equal(got[k], weighted[k]), (d, model, each, mode, k)
                    sdev = torch.from_numpy(got[2]).cuda()
                    frame = torch.full((n, d, d), 9, dtype=torch.uint8, device="cuda")
                    outs = [torch.zeros((n, 2), dtype=torch.int32, device="cuda") for _ in range(3)]
                    ev.decode_into(sdev, n, T, c, frame, *outs, final_round=mode, weights=weights)
                    torch.cuda.synchronize()
                    for key, x, y in zip(KEYS, got[3:], [frame] + outs):
                        assert np.array_equal(x, y.cpu().numpy()), (d, model, each, mode, key)
                    assert got[3].any() and weighted[0].any()
                if model == "DP":
                    assert (run((4, 4, 1))[3] != weighted[3]).any(), (d, each, mode)
                one = run((4, 4, 4))
                for k in range(7):
                    assert np.array_equal(one[k], weighted[k]), (d, model, each, mode, k)
    finally:
        ev.close()


# ---- 5. the experiment ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(), dict(final_round="perfect", referee="matching", no_decoder=True)])
def test_experiment_correlated_from_the_rates_equals_one_call_per_rate(dq, torch_mod, kw):
    DW = dq.decoder_wide
    d, n, T = 9, 512, 12
    rates, meas = [0.004, 0.008, 0.02], [0.04, 0.008, 0.001]
    both = DW.memory_experiment_wide((d, "DP"), n, T, rates=rates, p_meas=meas, seed=SEED, weights="rates", correlated="rates", chunk=700, **kw)
    assert list(both) == rates
    triples = [DW.uf_weights_correlated(a, b, "DP") for a, b in zip(rates, meas)]
    assert len(set(triples)) == 3
    differs = []
    for k, (a, b) in enumerate(zip(rates, meas)):
        tr = triples[k]
        one = DW.memory_experiment_wide((d, "DP"), n, T, p_phys=a, p_meas=b, seed=SEED, env_id_base=k * n, weights=tr[:2], correlated=tr[2], **kw)
        by_rate = DW.memory_experiment_wide((d, "DP"), n, T, p_phys=a, p_meas=b, seed=SEED, env_id_base=k * n, correlated="rates", **kw)
        plain = DW.memory_experiment_wide((d, "DP"), n, T, p_phys=a, p_meas=b, seed=SEED, env_id_base=k * n, weights=tr[:2], **kw)
        assert both[a].counters == one.counters == by_rate.counters and both[a].inexact == one.inexact, (a, both[a].counters, one.counters)
        assert both[a].weights == one.weights == by_rate.weights == tr and plain.weights == tr[:2]
        assert one.counters["volumes"] == n and 0 < one.counters["success"]
        if "no_decoder" in kw:
            assert both[a].no_decoder.counters == one.no_decoder.counters == plain.no_decoder.counters
        differs.append(one.counters != plain.counters)
    assert any(differs)                                                          # (the triples do decode differently from the pairs)


# ---- 6. the other forms are untouched by correlated calls on the same handle ------------------------------------------------------------------------------------
def test_unweighted_and_weighted_results_are_the_same_around_correlated_calls(dq, torch_mod):
    d, n, T, w, c = 9, 32, 36, 18, 9
    triple = (4, 4, 1)
    ev = dq.WideEvaluator(d, "DP", w, chunk=n)
    try:
        for closed in (False, True):
            syn = _sampled(d, T, n, closed=closed)
            forms = (dict(), dict(weights=(4, 4)), dict(weights=(3, 2)))
            before = [_wide(dq, d, syn, w, c, closed, evaluator=ev, **kw) for kw in forms]
            corr = _wide(dq, d, syn, w, c, closed, triple, evaluator=ev)
            after = [_wide(dq, d, syn, w, c, closed, evaluator=ev, **kw) for kw in forms]
            for b, a, kw in zip(before, after, forms):
                _same_results(a, b, ("around", closed, kw))
            assert _differs(corr, before[1]) >= 1, closed
            want = _reference(d, syn, w, c, closed, triple, (d, T, closed))
            _assert_equal(corr, want[:4], want[4], ("correlated on the handle", closed))
    finally:
        ev.close()
