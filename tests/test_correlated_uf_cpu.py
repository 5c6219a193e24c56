"""Correlated union-find without a GPU (decoder_wide correlated=; include/deepq_hip.h dq_wide_uf_decode_correlated / dq_wide_uf_run_correlated; DESIGN.md
section 25): the three-pass restatement of tests/correlated_uf_ref.py against the weighted restatement where the two must agree, the exhaustive scan of Y
errors at d = 5, the gain it is there for, uf_weights_correlated, validation before any library call, and the C ABI."""
import ctypes
import importlib
import itertools
import os
import types

import numpy as np
import pytest

import correlated_uf_ref as CR
import match_st_ref as M
import weighted_uf_ref as WR


def _same(got, want, tag):
    for k, (a, b) in enumerate(zip(got[:4], want[:4])):
        assert a.dtype == b.dtype and np.array_equal(a, b), (tag, k)
    assert got[4] == want[4], tag


# ---- 1. w_corr = w_space is the weighted restatement -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,T", [(5, 12), (7, 8)])
def test_w_corr_equal_to_w_space_is_the_weighted_restatement(d, T):
    for closed in (False, True):
        syn = CR.sample_streams(d, "DP", T, 4, 0.03, 0.03, (100 + d, 3), closed=closed)[0]
        for w, c in ((2, 1), (6, 3), (T, T)):
            for pair in ((4, 4), (3, 2)):
                want = WR.decode(d, syn, w, c, closed, pair)
                _same(CR.decode(d, syn, w, c, closed, pair + (pair[0],)), want, (d, closed, w, c, pair))
                assert want[2].sum() > 0 and want[0].any() and want[3].max() >= 2          # (not vacuous)
        # ... and a smaller w_corr is another decoder on these streams
        assert (CR.decode(d, syn, T, T, closed, (4, 4, 1))[0] != WR.decode(d, syn, T, T, closed, (4, 4))[0]).any()


def test_x_model_streams_are_the_weighted_result_for_any_w_corr():
    """Only component 0 has defects: pass 1 leaves an empty mask B, so pass 2 is the weighted decode.  (The stabilizers are read without error here: a
    misread stabilizer of component 1 is a defect pair of that component, and what its correction leaves in B is the rule's to use.)"""
    d, T = 5, 10
    syn = CR.sample_streams(d, "X", T, 6, 0.04, 0.0, (5, 9))[0]
    assert M.Component(d, 0).defects(syn).any() and not M.Component(d, 1).defects(syn).any()
    for w, c, closed in ((6, 3, False), (T, T, True), (2, 1, False)):
        want = WR.decode(d, syn, w, c, closed, (4, 3))
        for w_corr in (1, 2, 4):
            _same(CR.decode(d, syn, w, c, closed, (4, 3, w_corr)), want, (w, c, closed, w_corr))
        assert want[0].any()
    per_stream = np.array([(4, 3, 1 + i % 4) for i in range(6)])
    _same(CR.decode(d, syn, 6, 3, False, per_stream), WR.decode(d, syn, 6, 3, False, (4, 3)), "per stream")
    for bad in ((4, 4, 5), (4, 4, 0), (16, 1, 1), (4, 0, 1), (4, 4, 1.5)):
        with pytest.raises(ValueError):
            CR.decode(d, syn[:1], 6, 3, False, bad)


# ---- 2. the exhaustive scan of Y errors at d = 5, one perfect round ------------------------------------------------------------------------------------------
_scan = {}


def _y_fails(qs, triple):
    """Whether each component fails on Y errors at the qubits qs: d = 5, T = 1, closed, one window."""
    key = (tuple(qs), triple)
    if key not in _scan:
        d = 5
        err = np.zeros(d * d, dtype=np.int64)
        err[list(qs)] = 1
        C = [M.Component(d, 0), M.Component(d, 1)]
        rows = [((err @ c.H) & 1).reshape(1, -1) for c in C]
        res = CR.stream(d, rows[0], rows[1], 1, 1, True, *triple)
        out = []
        for k in range(2):
            r = err ^ np.array([(res[k]["M"] >> q) & 1 for q in range(d * d)], dtype=np.int64)
            assert not ((r @ C[k].H) & 1).any()
            out.append(bool((r @ C[k].logical) & 1))
        _scan[key] = tuple(out)
    return _scan[key]


def test_exhaustive_y_errors_at_d5():
    """(4, 4, 1) against the plain decoder (4, 4, 4) on every set of one, two and three Y errors.  The prototype of the rule gave: no single fails; 2 of
    the 300 pairs fail (in component 1; plain: none) -- the rule trades a few low-weight cases for many above them, which is documented, not a defect;
    triples 176 / 174 per component against 390 / 390."""
    corr, plain = (4, 4, 1), (4, 4, 4)
    assert not any(any(_y_fails((q,), corr)) for q in range(25))
    pairs = list(itertools.combinations(range(25), 2))
    assert len(pairs) == 300
    assert sum(any(_y_fails(qs, corr)) for qs in pairs) <= 2
    triples = list(itertools.combinations(range(25), 3))
    assert len(triples) == 2300
    got = np.array([_y_fails(qs, corr) for qs in triples]).sum(axis=0)
    ref = np.array([_y_fails(qs, plain) for qs in triples]).sum(axis=0)
    print(f"triples failing per component: correlated {got.tolist()}, plain {ref.tolist()}")
    assert ref.min() >= 300                                                            # (the plain decoder does fail here: the ratio means something)
    assert (got <= 0.6 * ref).all(), (got, ref)


PINNED_TRIPLE = (3, 12, 16)


def test_a_pinned_triple_that_only_the_correlated_decoder_corrects():
    """Y errors on qubits 3, 12 and 16: the plain decoder fails in both components, three passes correct both; with w_corr = 3 the scan still gains
    (307 / 310 triples against 390) and loses no pair."""
    assert not any(any(_y_fails(qs, (4, 4, 3))) for qs in itertools.combinations(range(25), 2))
    assert _y_fails(PINNED_TRIPLE, (4, 4, 4)) == (True, True) and _y_fails(PINNED_TRIPLE, (4, 4, 1)) == (False, False)


# ---- 3. the purpose -------------------------------------------------------------------------------------------------------------------------------------------
def test_correlated_decoding_fails_less_under_depolarising_noise():
    """d = 5, T = 6 in one closed window, 1500 DP streams at p = p_meas = 0.025, seed (7, 11), ids from 0, weights (4, 4): streams with a logical failure
    under w_corr = 1 are at most 0.8 of those under the plain weighted decode (the prototype: 63 against 98; per component 45 / 54 -> 34 / 31)."""
    d, T, n = 5, 6, 1500
    syn, hidden, _ = CR.sample_streams(d, "DP", T, n, 0.025, 0.025, (7, 11), 0, closed=True)
    plain = CR.failures(d, hidden, WR.decode(d, syn, 6, 6, True, (4, 4))[0])
    corr = CR.failures(d, hidden, CR.decode(d, syn, 6, 6, True, (4, 4, 1))[0])
    a, b = int(plain.any(axis=1).sum()), int(corr.any(axis=1).sum())
    print(f"failures of {n}: plain {a} {plain.sum(axis=0).tolist()}, correlated {b} {corr.sum(axis=0).tolist()}, ratio {b / max(1, a):.3f}")
    assert a >= 60                                                                     # (the plain decoder does fail here: the ratio means something)
    assert b <= 0.8 * a, (a, b)


# ---- 4. uf_weights_correlated ---------------------------------------------------------------------------------------------------------------------------------
def test_uf_weights_correlated(dq):
    DW = dq.decoder_wide
    assert dq.uf_weights_correlated is DW.uf_weights_correlated
    # X and IIDXZ: the components are independent, w_corr = w_space
    for model in ("X", "IIDXZ"):
        for a, b in ((0.01, 0.01), (0.01, 0.08), (0.03, 0.002), (0.001, 0.2)):
            ws, wt = DW.uf_weights(a, b, model)
            assert DW.uf_weights_correlated(a, b, model) == (ws, wt, ws)
    # DP: w_corr = 1, the pair scaled so that w_space >= 4 where 15 allows it
    assert DW.uf_weights_correlated(0.004, 0.004, "DP") == DW.uf_weights(0.004, 0.004, "DP") + (1,) == (8, 7, 1)
    assert DW.uf_weights_correlated(0.004, 0.04, "DP") == (7, 4, 1)
    assert DW.uf_weights(0.006, 0.004, "DP") == (1, 1) and DW.uf_weights_correlated(0.006, 0.004, "DP") == (4, 4, 1)
    for a, b in ((0.004, 0.016), (0.03, 0.01), (0.006, 0.004), (0.001, 0.2), (0.03, 0.002), (0.05, 0.0001), (0.2, 0.001)):
        for mw in (1, 2, 3, 8, 15):
            ws, wt = DW.uf_weights(a, b, "DP", max_weight=mw)
            t = DW.uf_weights_correlated(a, b, "DP", max_weight=mw)
            k = t[0] // ws
            assert t == (k * ws, k * wt, 1) and 1 <= t[2] <= t[0] <= 15 and 1 <= t[1] <= 15, (a, b, mw, t)
            assert k == max(1, min(-(-4 // ws), 15 // max(ws, wt))), (a, b, mw, t)
    assert DW.uf_weights_correlated(0.006, 0.004, "DP", max_weight=1) == (4, 4, 1)
    assert DW.uf_weights(0.75, 0.01, "DP") == (1, 8) and DW.uf_weights_correlated(0.75, 0.01, "DP") == (1, 8, 1)      # (15 leaves no room to scale)
    assert DW.uf_weights(0.2, 0.001, "DP") == (2, 7) and DW.uf_weights_correlated(0.2, 0.001, "DP") == (4, 14, 1)
    assert DW.uf_weights_correlated(0.2, 0.01, "DP", max_weight=3) == (4, 12, 1)
    assert DW.uf_weights_correlated(0.3, 0.0001, "DP", max_weight=4) == (3, 12, 1)                                    # (1, 4): 3 is the most 15 allows
    for bad in (dict(error_model="Y"), dict(max_weight=0), dict(max_weight=16), dict(p_phys=-0.1), dict(p_meas=1.5), dict(p_phys=None)):
        with pytest.raises(ValueError):
            DW.uf_weights_correlated(**dict(dict(p_phys=0.01, p_meas=0.01, error_model="DP"), **bad))
    # "rates": one triple per stream from the stream's own rates, scalars give one triple
    assert DW.rate_weights_correlated(0.004, 0.04, "DP", 4) == (7, 4, 1)
    each = DW.rate_weights_correlated(np.array([0.004] * 2 + [0.006] * 2), np.array([0.04, 0.04, 0.004, 0.004]), "DP", 4)
    assert each.dtype == np.uint8 and each.tolist() == [[7, 4, 1]] * 2 + [[4, 4, 1]] * 2


# ---- 5. validation before any library call -------------------------------------------------------------------------------------------------------------------
def _no_library(monkeypatch):
    _lib = importlib.import_module("deepq-decoding_amd._lib")

    def no_library(*a, **k):
        raise AssertionError("a library call was made before the arguments were validated")
    monkeypatch.setattr(_lib, "lib", no_library)
    monkeypatch.setattr(_lib, "require_gpu", no_library)
    monkeypatch.setattr(_lib, "check", no_library)


def test_correlated_is_validated_before_the_library_is_touched(dq, monkeypatch):
    _no_library(monkeypatch)
    DW = dq.decoder_wide
    syn = np.zeros((3, 12, 10, 10), dtype=np.uint8)
    env = types.SimpleNamespace(d=9, error_model="DP", use_Y=False, volume_depth=5, wide=True, n_envs=8, p_phys=0.01, p_meas=0.04, seed=(1, 2))
    each = np.array([[4, 4], [3, 2], [15, 1]])
    # (weights, correlated) that are refused
    bad = [(None, 1), ("rates", 1), ((4, 4), 5), ((4, 4), 0), ((4, 4), 16), ((4, 4), -1), ((4, 4), 1.0), ((4, 4), True), ((4, 4), "rate"), ((4, 4), (1,)),
           ((4, 4), [1]), (each, 4), (each, 0), ((4, 4), {}), ((4, 4), np.array([1, 1, 1]))]
    for weights, corr in bad + [((4, 4), "rates"), (None, "rates")]:
        with pytest.raises(ValueError):
            DW.stream_decode_wide(syn, 9, weights=weights, correlated=corr)
    for weights, corr in [b for b in bad if b[0] is not each] + [((4, 4), "rates"), ([4, 4], "rates"), (None, "RATES")]:
        with pytest.raises(ValueError):
            DW.memory_experiment_wide(env, 8, 12, weights=weights, correlated=corr)
    # what passes: the next thing touched is the library
    for weights, corr in (((4, 4), 1), ((4, 4), 4), ([15, 1], 15), (each, 3), (each, 1), ((4, 4), np.int64(2))):
        with pytest.raises(AssertionError, match="library call"):
            DW.stream_decode_wide(syn, 9, weights=weights, correlated=corr)
    for weights, corr in (((4, 4), 1), (None, "rates"), ("rates", "rates"), ([7, 4], 7)):
        with pytest.raises(AssertionError, match="library call"):
            DW.memory_experiment_wide(env, 8, 12, weights=weights, correlated=corr)
        with pytest.raises(AssertionError, match="library call"):
            DW.memory_experiment_wide((9, "DP"), 8, 12, rates=[0.004, 0.01], p_meas=0.04, seed=(1, 2), weights=weights, correlated=corr,
                                      final_round="perfect", referee="matching")
    # None changes nothing: the weighted and the unweighted requests reach the library as before
    for weights in (None, (2, 1)):
        with pytest.raises(AssertionError, match="library call"):
            DW.stream_decode_wide(syn, 9, weights=weights, correlated=None)
    assert DW.check_correlated(None, None) is None and DW.check_correlated(2, (4, 4)) == 2 and DW.check_correlated("rates", None, rates=True) == "rates"
    assert DW.with_correlated((4, 3), 2) == (4, 3, 2) and DW.with_correlated((4, 3), None) == (4, 3) and DW.with_correlated(None, None) is None
    got = DW.with_correlated(DW.check_weights(each, 3), 1)
    assert got.dtype == np.uint8 and got.tolist() == [[4, 4, 1], [3, 2, 1], [15, 1, 1]] and got.flags["C_CONTIGUOUS"]
    # decode_benchmark_wide: the union-find row's, so a baseline is needed
    agent = types.SimpleNamespace()
    DQNAgent = dq.DQNAgent
    for kw in (dict(correlated="rates"), dict(weights=(4, 4), correlated=1)):
        with pytest.raises(ValueError, match="baseline"):
            DQNAgent.decode_benchmark_wide(agent, env, 8, **kw)
    with pytest.raises(ValueError):
        DQNAgent.decode_benchmark_wide(agent, env, 8, baseline="union_find", weights=(4, 4), correlated=5)


class _Ptr:
    def __init__(self, p, shape=None):
        self.p = p
        if shape is not None:
            self.shape = shape

    def data_ptr(self):
        return self.p


def test_evaluator_methods_hand_the_triple_to_the_library(dq, monkeypatch):
    DW = dq.decoder_wide
    L = importlib.import_module("deepq-decoding_amd._lib")
    monkeypatch.setattr(L, "check", lambda status: None)
    calls = []
    ev = object.__new__(DW.WideEvaluator)
    ev._h, ev._stream = "handle", lambda: "stream"
    names = ("dq_wide_uf_decode", "dq_wide_uf_decode_closed", "dq_wide_uf_decode_weighted", "dq_wide_uf_decode_correlated", "dq_wide_uf_run",
             "dq_wide_uf_run_weighted", "dq_wide_uf_run_correlated")
    ev.L = types.SimpleNamespace(dq_wide_uf_destroy=lambda h: None,
                                 **{name: (lambda *a, _n=name: calls.append((_n[len("dq_wide_uf_"):],) + a)) for name in names})
    ev.decode_into(_Ptr(10), 3, 40, 5, _Ptr(11), weights=None)
    assert calls.pop() == ("decode", "handle", 10, 3, 40, 5, 11, None, None, None, "stream")
    ev.decode_into(_Ptr(10), 3, 40, 5, _Ptr(11), weights=(3, 2))
    assert calls.pop() == ("decode_weighted", "handle", 10, 3, 40, 5, 0, 3, 2, None, 11, None, None, None, "stream")
    ev.decode_into(_Ptr(10), 3, 40, 5, _Ptr(11), weights=_Ptr(77, (3, 2)))
    assert calls.pop() == ("decode_weighted", "handle", 10, 3, 40, 5, 0, 1, 1, 77, 11, None, None, None, "stream")
    ev.decode_into(_Ptr(10), 3, 40, 5, _Ptr(11), _Ptr(12), _Ptr(13), _Ptr(14), weights=(4, 3, 2))
    assert calls.pop() == ("decode_correlated", "handle", 10, 3, 40, 5, 0, 4, 3, 2, None, 11, 12, 13, 14, "stream")
    ev.decode_into(_Ptr(10), 3, 40, 5, _Ptr(11), final_round="perfect", weights=_Ptr(77, (3, 3)))
    assert calls.pop() == ("decode_correlated", "handle", 10, 3, 40, 5, 1, 1, 1, 1, 77, 11, None, None, None, "stream")
    ev.run_into(3, 40, 5, (1 << 32) + 9, (7, 8), 0.01, 0.02, _Ptr(20), _Ptr(21), _Ptr(22), final_round="perfect", weights=(4, 3, 1))
    got = calls.pop()
    assert got[:6] == ("run_correlated", "handle", 3, 40, 5, 9) and list(got[6]) == [7, 8]
    assert got[7:] == (0.01, 0.02, None, None, 1, 4, 3, 1, None, 20, 21, 22, None, None, None, None, "stream")
    ph, pm = np.array([0.01, 0.02, 0.03]), np.array([0.0, 0.0, 0.1])
    ev.run_into(3, 40, 5, 0, (7, 8), ph, pm, _Ptr(20), _Ptr(21), _Ptr(22), _Ptr(23), _Ptr(24), _Ptr(25), _Ptr(26), weights=_Ptr(77, (3, 3)))
    assert calls.pop()[7:] == (0.0, 0.0, ph.ctypes.data, pm.ctypes.data, 0, 1, 1, 1, 77, 20, 21, 22, 23, 24, 25, 26, "stream")
    ev.run_into(3, 40, 5, 0, (7, 8), 0.01, 0.02, _Ptr(20), _Ptr(21), _Ptr(22), weights=(2, 1))
    assert calls.pop()[0] == "run_weighted"
    ev.run_into(3, 40, 5, 0, (7, 8), 0.01, 0.02, _Ptr(20), _Ptr(21), _Ptr(22))
    assert calls.pop()[0] == "run"
    ev._h = None


# ---- 6. the C ABI --------------------------------------------------------------------------------------------------------------------------------------------
def test_correlated_abi_is_declared_and_bound():
    L = importlib.import_module("deepq-decoding_amd._lib")
    lib = L.lib()
    assert lib.dq_version() == 8                                                       # new capability = the presence of the new symbols
    header = open(os.path.join(os.path.dirname(L.__file__), "..", "include", "deepq_hip.h")).read()
    vp, i, dbl, u32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_uint32
    want = {"dq_wide_uf_decode_correlated": (i, [vp, vp, i, i, i, i, i, i, i, vp, vp, vp, vp, vp, vp]),
            "dq_wide_uf_run_correlated": (i, [vp, i, i, i, u32, ctypes.POINTER(u32), dbl, dbl, vp, vp, i, i, i, i, vp, vp, vp, vp, vp, vp, vp, vp, vp])}
    for name, sig in want.items():
        assert name + "(" in header and hasattr(lib, name) and L.SIGNATURES[name] == sig, name
    # the weighted forms' arguments with w_corr behind w_time
    for name in ("decode", "run"):
        a, b = L.SIGNATURES[f"dq_wide_uf_{name}_weighted"][1], L.SIGNATURES[f"dq_wide_uf_{name}_correlated"][1]
        k = 8 if name == "decode" else 13
        assert b == a[:k] + [i] + a[k:], name
    seed = (u32 * 2)(1, 2)
    one = ctypes.c_void_p(1)                                                           # (never read: every call below is refused before any device work)
    assert lib.dq_wide_uf_decode_correlated(None, None, 1, 1, 1, 0, 4, 4, 1, None, None, None, None, None, None) == -1
    assert lib.dq_wide_uf_run_correlated(None, 1, 1, 1, 0, seed, 0.01, 0.01, None, None, 0, 4, 4, 1, None, None, None, None, None, None, None, None, None) == -1
    for closed, ws, wt, wc in ((2, 4, 4, 1), (0, 0, 1, 1), (0, 4, 0, 1), (1, 16, 1, 1), (0, 4, 4, 0), (0, 4, 4, 5), (1, 4, 15, 5), (0, 1, 1, 2), (0, 4, 4, -1)):
        assert lib.dq_wide_uf_decode_correlated(one, one, 1, 1, 1, closed, ws, wt, wc, None, one, None, None, None, None) == -1, (closed, ws, wt, wc)
        assert lib.dq_wide_uf_run_correlated(one, 1, 1, 1, 0, seed, 0.01, 0.01, None, None, closed, ws, wt, wc, None, one, one, one, None, None, None, None,
                                             None) == -1, (closed, ws, wt, wc)
        assert b"dq_wide_uf_run_correlated" in lib.dq_last_error()
    assert b"w_corr" in lib.dq_last_error()
    # the weighted entry points keep their signatures
    assert L.SIGNATURES["dq_wide_uf_decode_weighted"] == (i, [vp, vp, i, i, i, i, i, i, vp, vp, vp, vp, vp, vp])
