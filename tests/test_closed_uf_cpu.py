"""Union-find stream decoding with a perfect final round, host side: tests/closed_uf_ref.py -- the numpy statement the device is
compared with bit for bit in tests/test_closed_uf_gpu.py -- checked on its own (open: equal to stream_uf_ref / wide_uf_ref in every field; closed: the
frame's syndrome is the stream's last syndrome, and no fault set of weight <= (d - 1) / 2 defeats it); then the final_round keyword before any library
call, the C ABI and the Python plumbing."""
import contextlib
import ctypes
import importlib
import itertools
import os
import types

import numpy as np
import pytest

import closed_uf_ref as R
import match_st_ref as M
import stream_uf_ref as S
import wide_uf_ref as W

SCHEDULES = [(1, 1), (2, 1), (10, 5), (16, 16), (32, 16)]
SAMPLED = {3: (7, 0.05, 12), 5: (23, 0.011, 8), 7: (23, 0.02, 4), 9: (20, 0.012, 2)}          # d: rounds, rate, streams per component


def _plane(d, mask):
    return np.array([(mask >> q) & 1 for q in range(d * d)], dtype=np.int64)


def _streams(d):
    T, p, n = SAMPLED[d]
    for i in range(2 * n):
        comp = i & 1
        rows, s = S.sample_component_rows(d, comp, T, p, np.random.default_rng(7000 + 100 * d + i))
        yield comp, rows, s


# ---- 1. the restatement alone ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", sorted(SAMPLED))
def test_open_restatement_equals_the_existing_ones(d):
    """closed=False: every field of stream_uf_ref (window <= 16, d <= 7) and of wide_uf_ref."""
    seen = 0
    for comp, rows, _ in _streams(d):
        for w, c in SCHEDULES:
            got = R.stream_component(d, comp, rows, w, c, False)
            want = W.stream_component(d, comp, rows, w, c)
            assert {k: got[k] for k in ("M", "W", "ndef", "rounds", "windows")} == {k: want[k] for k in ("M", "W", "ndef", "rounds", "windows")}, (d, comp, w, c)
            assert np.array_equal(got["last"], want["last"])
            if w <= 16 and d <= 7:
                narrow = S.stream_component(d, comp, rows, w, c)
                assert (got["M"], got["W"], got["ndef"], got["rounds"], got["windows"]) == tuple(narrow[k] for k in ("M", "W", "ndef", "rounds", "windows"))
                assert np.array_equal(got["last"], narrow["last"])
            seen += got["W"]
    assert seen > 0


def test_open_grid_decode_equals_the_existing_ones():
    rng = np.random.default_rng(5)
    syn = (rng.random((4, 9, 6, 6)) < 0.06).astype(np.uint8)
    for w, c in ((10, 5), (2, 1), (4, 4)):
        got, want, narrow = R.decode(5, syn, w, c, False), W.decode(5, syn, w, c), S.decode(5, syn, w, c)
        for k in range(4):
            assert np.array_equal(got[k], want[k]) and np.array_equal(got[k], narrow[k]) and got[k].dtype == want[k].dtype
        assert got[4] == want[4] == narrow[4] and all(np.array_equal(a, b) for a, b in zip(got[5], want[5]))


@pytest.mark.parametrize("d", sorted(SAMPLED))
def test_closed_frame_syndrome_is_the_last_syndrome(d):
    """H M = S_{T-1} and last = 0 on every sampled stream under every schedule, whatever the last round holds (the streams end on a faulty round here: the
    closed decode is defined for any input)."""
    differs = 0
    for comp, rows, s in _streams(d):
        C = M.Component(d, comp)
        for w, c in SCHEDULES:
            r = R.stream_component(d, comp, rows, w, c, True)
            assert np.array_equal((_plane(d, r["M"]) @ C.H) & 1, s[-1]), (d, comp, w, c)
            assert not r["last"].any() and r["ndef"] == rows.sum() and r["windows"] == R.n_windows(len(rows), w, c)
            o = R.stream_component(d, comp, rows, w, c, False)
            assert np.array_equal(((_plane(d, o["M"]) @ C.H) & 1) ^ o["last"], s[-1])      # the open form's closing rule, for contrast
            differs += (o["M"], o["W"]) != (r["M"], r["W"])
    assert differs > 0 or d == 3              # (at d = 3 every node has a space edge to B, whose id is below its time edge's: both forms may take it)


def test_one_round_is_code_capacity_decoding_on_space_edges():
    for d in (3, 5, 7):
        for comp in (0, 1):
            C = M.Component(d, comp)
            rng = np.random.default_rng(d + comp)
            for _ in range(20):
                rows = (rng.random((1, C.n)) < 0.2).astype(np.int64)
                edges, _ = R.window_edges(d, comp, rows, 1, True)
                assert all(e < d * d for e in edges)                                   # space edges only
                m = np.zeros(d * d, dtype=np.int64)
                m[edges] = 1
                assert np.array_equal((m @ C.H) & 1, rows[0])
                assert R.stream_component(d, comp, rows, 16, 16, True)["W"] == len(edges)
    # a lone defect: the open form leaves by the one time edge to B, the closed form walks to the spatial boundary
    C = M.Component(5, 0)
    rows = np.zeros((1, C.n), dtype=np.int64)
    rows[0, 5] = 1
    assert R.window_edges(5, 0, rows, 1, False)[0] == [25 + 5]
    closed = R.window_edges(5, 0, rows, 1, True)[0]
    assert closed and all(e < 25 for e in closed)


# ---- 2. no fault set of weight <= (d - 1) / 2 defeats the closed decoder -------------------------------------------------------------------------------
def _faults(d, comp, T):
    n = M.Component(d, comp).n
    return [("d", j, q) for j in range(T) for q in range(d * d)] + [("m", j, u) for j in range(T - 1) for u in range(n)]


def _failures(d, comp, T, sets, schedules):
    C, stab = M.Component(d, comp), R.Stabilizers(d, comp)
    bad = []
    for fs in sets:
        rows, err, s_last = R.fault_rows(d, comp, T, [(j, x) for k, j, x in fs if k == "d"], [(j, x) for k, j, x in fs if k == "m"])
        for w, c in schedules:
            r = R.stream_component(d, comp, rows, w, c, True)
            res = err ^ _plane(d, r["M"])
            if ((res @ C.H) & 1).any() or not stab.trivial(res):
                bad.append((fs, w, c))
    return bad


@pytest.mark.parametrize("comp", [0, 1])
def test_d5_four_rounds_every_single_and_pair(comp):
    f = _faults(5, comp, 4)
    sets = [(a,) for a in f] + list(itertools.combinations(f, 2))
    assert len(f) == 136 and len(sets) == 9316
    assert _failures(5, comp, 4, sets, [(4, 4), (3, 2), (2, 1)]) == []


@pytest.mark.parametrize("d,schedules,count", [(3, [(3, 3), (2, 1), (1, 1)], 35), (7, [(3, 3), (2, 1)], 195)])
def test_three_rounds_every_single_fault(d, schedules, count):
    for comp in (0, 1):
        sets = [(a,) for a in _faults(d, comp, 3)]
        assert len(sets) == count
        assert _failures(d, comp, 3, sets, schedules) == []


@pytest.mark.parametrize("d,count", [(5, 325), (3, 9)])
def test_one_round_every_data_error_up_to_half_the_distance(d, count):
    for comp in (0, 1):
        f = [("d", 0, q) for q in range(d * d)]
        sets = [s for k in range(1, (d - 1) // 2 + 1) for s in itertools.combinations(f, k)]
        assert len(sets) == count
        assert _failures(d, comp, 1, sets, [(1, 1)]) == []


def test_gf2_rank_and_stabilizer_membership():
    assert R.gf2_rank(np.eye(4, dtype=np.int64)) == 4 and R.gf2_rank([[1, 1, 0], [0, 1, 1], [1, 0, 1]]) == 2 and R.gf2_rank(np.zeros((2, 3))) == 0
    for d in (3, 5):
        for comp in (0, 1):
            st, C, other = R.Stabilizers(d, comp), M.Component(d, comp), M.Component(d, 1 - comp)
            assert st.rank == other.n
            assert st.trivial(np.zeros(d * d, dtype=np.int64)) and st.trivial(other.H[:, 0]) and st.trivial(other.H[:, 0] ^ other.H[:, 1])
            logical = next(p for p in (np.eye(d, dtype=np.int64)[i][:, None] * np.ones(d, dtype=np.int64) for i in range(d))
                           for p in (p.reshape(-1), p.T.reshape(-1)) if not ((p @ C.H) & 1).any() and (p @ C.logical) & 1)
            assert not st.trivial(logical)                                             # a row or column that commutes with the checks and is no stabilizer


# ---- 3. the restated sampler ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["X", "DP", "IIDXZ"])
def test_closed_sampler_drops_only_the_last_flips(model):
    import decode_eval_ref as E
    d, T, n, seed = 5, 6, 64, (11, 12)
    p, pm = np.linspace(0.01, 0.08, n), np.linspace(0.08, 0.01, n)
    open_ = R.sample_streams(d, model, T, n, p, pm, seed, 9)
    assert all(np.array_equal(a, b) for a, b in zip(open_, E.sample_volumes(d, model, T, n, p, pm, seed, 9)))
    g, hid, triv = R.sample_streams(d, model, T, n, p, pm, seed, 9, closed=True)
    assert np.array_equal(hid, open_[1]) and np.array_equal(g[:, :-1], open_[0][:, :-1]) and (g[:, -1] != open_[0][:, -1]).any()
    x, z = E.codes_to_xz(hid)
    assert np.array_equal(g[:, -1], E.bits_to_grids(d, E.syndrome_bits(d, x, z)))      # the true syndrome of what accumulated
    assert np.array_equal(triv, (g.reshape(n, -1).max(axis=1) == 0).astype(np.uint8))


# ---- 4. final_round is validated before any library call --------------------------------------------------------------------------------------------
def _no_library(monkeypatch):
    _lib = importlib.import_module("deepq-decoding_amd._lib")

    def no_library(*a, **k):
        raise AssertionError("a library call was made before the arguments were validated")
    monkeypatch.setattr(_lib, "lib", no_library)
    monkeypatch.setattr(_lib, "require_gpu", no_library)
    monkeypatch.setattr(_lib, "check", no_library)


def _stub(**kw):
    return types.SimpleNamespace(**dict(dict(d=5, error_model="DP", use_Y=False, volume_depth=5, wide=False, n_envs=8, identity_index=50, p_phys=0.01, p_meas=0.01,
                                             seed=(1, 2)), **kw))


BAD = ("Perfect", "closed", "", None, True, 1, b"perfect", ("perfect",))


def test_final_round_is_validated_before_the_library_is_touched(dq, monkeypatch):
    _no_library(monkeypatch)
    D, DW = dq.decoder, dq.decoder_wide
    assert D.FINAL_ROUNDS == ("faulty", "perfect")
    assert D.check_final_round("faulty") is False and D.check_final_round("perfect") is True
    syn, syn9 = np.zeros((2, 40, 6, 6), dtype=np.uint8), np.zeros((2, 40, 10, 10), dtype=np.uint8)
    for bad in BAD:
        with pytest.raises(ValueError, match="final_round"):
            D.check_final_round(bad)
        with pytest.raises(ValueError, match="final_round"):
            D.stream_decode(syn, _stub(), final_round=bad)
        with pytest.raises(ValueError, match="final_round"):
            D.memory_experiment(_stub(), 16, 40, final_round=bad)
        with pytest.raises(ValueError, match="final_round"):
            DW.stream_decode_wide(syn9, 9, final_round=bad)
        with pytest.raises(ValueError, match="final_round"):
            DW.memory_experiment_wide((9, "DP"), 16, 40, p_phys=0.01, seed=(1, 2), final_round=bad)
        for ev, call in ((object.__new__(D.Evaluator), lambda e: e.stream_uf_into(None, 1, 1, 1, None, final_round=bad)),
                         (object.__new__(D.Evaluator), lambda e: e.stream_run_into(_stub(_h=1), 1, 1, 1, 0, (1, 2), 0.1, 0.1, None, None, None, final_round=bad)),
                         (object.__new__(DW.WideEvaluator), lambda e: e.decode_into(None, 1, 1, 1, None, final_round=bad)),
                         (object.__new__(DW.WideEvaluator), lambda e: e.run_into(1, 1, 1, 0, (1, 2), 0.1, 0.1, None, None, None, final_round=bad))):
            ev._h = None
            ev.L = types.SimpleNamespace()                                             # any attribute access would fail
            with pytest.raises(ValueError, match="final_round"):
                call(ev)
    # the other checks still hold with the keyword, and a valid request reaches the library
    with pytest.raises(NotImplementedError, match="committed rounds"):
        D.stream_decode(syn, _stub(), method="matching", final_round="perfect")
    with pytest.raises(NotImplementedError):
        D.stream_decode(syn9, _stub(d=9), final_round="perfect")
    with pytest.raises(ValueError):
        D.stream_decode(syn, _stub(), window=17, final_round="perfect")
    with pytest.raises(ValueError):
        DW.stream_decode_wide(syn9, 9, window=33, final_round="perfect")
    with pytest.raises(AssertionError, match="library call"):
        DW.memory_experiment_wide(_stub(d=9), 16, 40, final_round="perfect")
    with pytest.raises(AssertionError, match="library call"):
        DW.stream_decode_wide(syn9, 9, final_round="perfect")
    # the existing validators keep their signatures and their tuples
    assert D.check_stream_args(_stub(), syn, 16, 1) == (5, "DP", False, 2, False, 40, 16, 1)
    assert D.check_stream_schedule(5, 33, None, None) == (33, 10, 5)
    assert DW.check_wide_stream_args(syn9, 9) == (9, 2, False, 40, 18, 9, DW.DEFAULT_CHUNK)
    assert DW.check_wide_experiment_args((9, "DP"), 4, 40, p_phys=0.01, seed=(5, 6))[:6] == (9, "DP", 40, 18, 9, 4)


# ---- 5. the C ABI --------------------------------------------------------------------------------------------------------------------------------------
def test_closed_abi_is_declared_and_bound():
    L = importlib.import_module("deepq-decoding_amd._lib")
    lib = L.lib()
    assert lib.dq_version() == 8                                                       # new capability = the presence of the new symbols
    header = open(os.path.join(os.path.dirname(L.__file__), "..", "include", "deepq_hip.h")).read()
    vp, i, dbl, u32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_uint32
    pairs = {"dq_stream_decode_uf_closed": "dq_stream_decode_uf", "dq_stream_run_uf_closed": "dq_stream_run_uf",
             "dq_wide_uf_decode_closed": "dq_wide_uf_decode", "dq_wide_uf_run_closed": "dq_wide_uf_run"}
    want = {"dq_stream_decode_uf_closed": (i, [vp, vp, i, i, i, vp, vp, vp, vp, vp]),
            "dq_stream_run_uf_closed": (i, [vp, vp, i, i, i, u32, ctypes.POINTER(u32), dbl, dbl, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
            "dq_wide_uf_decode_closed": (i, [vp, vp, i, i, i, vp, vp, vp, vp, vp]),
            "dq_wide_uf_run_closed": (i, [vp, i, i, i, u32, ctypes.POINTER(u32), dbl, dbl, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp])}
    flat = " ".join(header.split())
    for name, sig in want.items():
        assert "dq_status " + name + "(" in header and hasattr(lib, name) and L.SIGNATURES[name] == sig == L.SIGNATURES[pairs[name]], name
        args = lambda f: flat.split("dq_status " + f + "(")[1].split(");")[0]
        assert args(name) == args(pairs[name]), name                                   # the argument list of the open counterpart, name for name
    seed = (u32 * 2)(1, 2)
    h = vp()
    # DQ_ERR_INVALID on null handles, no device touched
    assert lib.dq_stream_decode_uf_closed(None, None, 1, 1, 1, None, None, None, None, None) == -1
    assert b"dq_stream_decode_uf_closed" in lib.dq_last_error()
    assert lib.dq_stream_run_uf_closed(None, None, 1, 1, 1, 0, seed, 0.01, 0.01, None, None, None, None, None, None, None, None, None, None) == -1
    assert b"dq_stream_run_uf_closed" in lib.dq_last_error()
    assert lib.dq_wide_uf_decode_closed(None, None, 1, 1, 1, None, None, None, None, None) == -1
    assert b"dq_wide_uf_decode_closed" in lib.dq_last_error()
    assert lib.dq_wide_uf_run_closed(None, 1, 1, 1, 0, seed, 0.01, 0.01, None, None, None, None, None, None, None, None, None, None) == -1
    assert b"dq_wide_uf_run_closed" in lib.dq_last_error()
    # the open forms answer as before, under their own names
    assert lib.dq_stream_decode_uf(None, None, 1, 1, 1, None, None, None, None, None) == -1 and b"dq_stream_decode_uf:" in lib.dq_last_error()
    assert lib.dq_wide_uf_run(None, 1, 1, 1, 0, seed, 0.01, 0.01, None, None, None, None, None, None, None, None, None, None) == -1
    assert b"dq_wide_uf_run:" in lib.dq_last_error() and not h.value
    doc = header.split("Streams closed by a final round of perfect measurements")[1].split("dq_status dq_stream_decode_uf_closed")[0]
    assert "dq_version() stays 8" in doc and "one-host-thread" in doc and "never in the correction" in doc
    digest = importlib.import_module("deepq-decoding_amd._digest")
    assert lib.dq_build_digest().decode() == digest.csrc_digest()


# ---- 6. plumbing with stubs ------------------------------------------------------------------------------------------------------------------------------
class _Ptr:
    def __init__(self, p):
        self.p = p

    def data_ptr(self):
        return self.p


def test_evaluator_methods_pick_the_entry_point(dq, monkeypatch):
    D, DW = dq.decoder, dq.decoder_wide
    L = importlib.import_module("deepq-decoding_amd._lib")
    monkeypatch.setattr(L, "check", lambda status: None)
    calls = []
    rec = lambda name: (lambda *a: calls.append((name,) + a))
    ev = object.__new__(D.Evaluator)
    ev._h, ev._stream = "handle", lambda: "stream"
    ev.L = types.SimpleNamespace(dq_stream_decode_uf=rec("decode"), dq_stream_run_uf=rec("run"), dq_stream_decode_uf_closed=rec("decode_closed"),
                                 dq_stream_run_uf_closed=rec("run_closed"), dq_decode_eval_destroy=lambda h: None)
    venv = types.SimpleNamespace(_h="env")
    for kw, tag in (({}, ""), (dict(final_round="faulty"), ""), (dict(final_round="perfect"), "_closed")):
        ev.stream_uf_into(_Ptr(10), 3, 40, 5, _Ptr(11), _Ptr(12), _Ptr(13), _Ptr(14), **kw)
        assert calls.pop() == ("decode" + tag, "handle", 10, 3, 40, 5, 11, 12, 13, 14, "stream")
        ev.stream_run_into(venv, 3, 40, 5, (1 << 32) + 9, (7, 8), 0.01, 0.02, _Ptr(20), _Ptr(21), _Ptr(22), **kw)
        got = calls.pop()
        assert got[:7] == ("run" + tag, "handle", "env", 3, 40, 5, 9) and list(got[7]) == [7, 8]
        assert got[8:] == (0.01, 0.02, None, None, 20, 21, 22, None, None, None, None, "stream")
    ev._h = None
    wv = object.__new__(DW.WideEvaluator)
    wv._h, wv._stream = "handle", lambda: "stream"
    wv.L = types.SimpleNamespace(dq_wide_uf_decode=rec("decode"), dq_wide_uf_run=rec("run"), dq_wide_uf_decode_closed=rec("decode_closed"),
                                 dq_wide_uf_run_closed=rec("run_closed"), dq_wide_uf_destroy=lambda h: None)
    ph, pm = np.array([0.01, 0.02, 0.03]), np.array([0.0, 0.0, 0.1])
    for kw, tag in (({}, ""), (dict(final_round="faulty"), ""), (dict(final_round="perfect"), "_closed")):
        wv.decode_into(_Ptr(10), 3, 40, 5, _Ptr(11), **kw)
        assert calls.pop() == ("decode" + tag, "handle", 10, 3, 40, 5, 11, None, None, None, "stream")
        wv.run_into(3, 40, 5, 0, (7, 8), ph, pm, _Ptr(20), _Ptr(21), _Ptr(22), _Ptr(23), _Ptr(24), _Ptr(25), _Ptr(26), **kw)
        got = calls.pop()
        assert got[:6] == ("run" + tag, "handle", 3, 40, 5, 0) and got[7:] == (0.0, 0.0, ph.ctypes.data, pm.ctypes.data, 20, 21, 22, 23, 24, 25, 26, "stream")
    wv._h = None


class _OldEvaluator:
    """An evaluator with the argument lists of before the keyword: what the open entry points must still be able to drive."""

    def __init__(self, d, window, chunk, wide):
        self.d, self.error_model, self.use_Y, self.chunk, self.device = d, "DP", False, chunk, "cpu"
        self.window = self.volume_depth = window
        self.wide, self.calls = wide, []

    def _run(self, m, lattice_id, hidden, trivial, frame):
        hidden.zero_()
        frame.zero_()
        trivial.zero_()
        self.calls.append(("run", m, lattice_id))

    def stream_run_into(self, venv, m, T, commit, lattice_id, seed, p_phys, p_meas, hidden, trivial, frame, weight=None, n_defects=None, rounds=None,
                        syndromes=None):
        self._run(m, lattice_id, hidden, trivial, frame)

    def run_into(self, m, T, commit, lattice_id, seed, p_phys, p_meas, hidden, trivial, frame, weight=None, n_defects=None, rounds=None, syndromes=None):
        self._run(m, lattice_id, hidden, trivial, frame)

    def stream_uf_into(self, syndromes, m, T, commit, frame, weight=None, n_defects=None, rounds=None):
        self.calls.append(("decode", m))
        for x in (frame, weight, n_defects, rounds):
            x.zero_()

    decode_into = stream_uf_into

    def verdict_into(self, *a):
        a[-1].fill_(9)

    def count_into(self, verdict, trivial, status, n_corr, m, first, block, counters):
        counters[first // block, 0] += m


class _NewEvaluator(_OldEvaluator):
    def stream_run_into(self, *a, final_round="faulty", **kw):
        self.calls.append(("final_round", final_round))
        super().stream_run_into(*a, **kw)

    def run_into(self, *a, final_round="faulty", **kw):
        self.calls.append(("final_round", final_round))
        super().run_into(*a, **kw)

    def stream_uf_into(self, *a, final_round="faulty", **kw):
        self.calls.append(("final_round", final_round))
        super().stream_uf_into(*a, **kw)

    decode_into = stream_uf_into


def test_open_entry_points_keep_their_old_calls_and_closed_ones_pass_the_keyword(dq, monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "device", lambda dev: contextlib.nullcontext())
    monkeypatch.setattr(torch.cuda, "current_stream", lambda dev=None: types.SimpleNamespace(synchronize=lambda: None))
    D, DW = dq.decoder, dq.decoder_wide
    env = _stub(_h=1, device="cpu")
    syn, syn9 = np.zeros((5, 12, 6, 6), dtype=np.uint8), np.zeros((5, 12, 10, 10), dtype=np.uint8)
    # the old argument lists, positionally and by keyword, against evaluators that know nothing of final_round
    ev = _OldEvaluator(5, 10, 3, False)
    r = D.memory_experiment(env, 7, 40, None, None, None, 0.02, None, (3, 4), 100, 4, False, None, ev, False)
    assert r.counters["volumes"] == 7 and ev.calls == [("run", 3, 100), ("run", 3, 103), ("run", 1, 106)]
    ev = _OldEvaluator(5, 10, 3, False)
    res = D.stream_decode(syn, env, 10, 5, 2, True, ev, "union_find")
    assert res.frame.shape == (5, 5, 5) and res.windows == 2 and ev.calls == [("decode", 3), ("decode", 2)]
    ev = _OldEvaluator(9, 18, 3, True)
    r = DW.memory_experiment_wide((9, "DP"), 7, 40, None, None, None, 0.02, None, (3, 4), 100, 4, False, None, ev, False)
    assert r.counters["volumes"] == 7 and ev.calls == [("run", 3, 100), ("run", 3, 103), ("run", 1, 106)]
    ev = _OldEvaluator(9, 18, 3, True)
    res = DW.stream_decode_wide(syn9, 9, 18, 9, 2, True, ev)
    assert res.frame.shape == (5, 9, 9) and ev.calls == [("decode", 3), ("decode", 2)]
    with pytest.raises(TypeError):                                                     # such an evaluator cannot serve a closed request, and says so
        DW.stream_decode_wide(syn9, 9, evaluator=_OldEvaluator(9, 18, 3, True), final_round="perfect")
    # the closed forms hand the keyword to every chunk; the result's layout is the open one
    ev = _NewEvaluator(5, 10, 4, False)
    out = D.memory_experiment(env, 4, 40, rates=[0.01, 0.03], evaluator=ev, final_round="perfect", no_decoder=True)
    assert list(out) == [0.01, 0.03] and all(isinstance(v, D.EvalResult) and v.counters["volumes"] == 4 and v.no_decoder is not None for v in out.values())
    assert [c for c in ev.calls if c[0] == "final_round"] == [("final_round", "perfect")] * 2
    ev = _NewEvaluator(5, 10, 4, False)
    r, streams = D.memory_experiment(env, 6, 12, evaluator=ev, final_round="perfect", return_streams=True)
    assert set(streams) == {"syndromes", "hidden", "frame", "trivial"} and tuple(streams["syndromes"].shape) == (6, 12, 6, 6)
    ev = _NewEvaluator(5, 10, 2, False)
    res = D.stream_decode(syn, env, evaluator=ev, final_round="perfect", to_host=True)
    assert isinstance(res, D.StreamResult) and [c for c in ev.calls if c[0] == "final_round"] == [("final_round", "perfect")] * 3
    ev = _NewEvaluator(9, 18, 4, True)
    DW.memory_experiment_wide((9, "DP"), 6, 40, p_phys=0.01, seed=(1, 2), evaluator=ev, final_round="perfect")
    DW.stream_decode_wide(syn9, 9, evaluator=ev, final_round="perfect")
    assert [c for c in ev.calls if c[0] == "final_round"] == [("final_round", "perfect")] * 4
    ev = _NewEvaluator(9, 18, 4, True)
    DW.stream_decode_wide(syn9, 9, evaluator=ev, final_round="faulty")
    assert ("final_round", "faulty") in ev.calls and ("final_round", "perfect") not in ev.calls
