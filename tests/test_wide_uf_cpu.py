"""The wide sliding-window union-find decoder without a GPU (decoder_wide; include/deepq_hip.h dq_wide_uf_*): the restatement of
tests/wide_uf_ref.py against the two restatements it extends, the closing-syndrome rule at d = 9 and d = 13, validation before any library call, the C ABI,
and the chunk / id / rate-block plumbing with stubs."""
import contextlib
import ctypes
import importlib
import os
import types

import numpy as np
import pytest

import match_st_ref as M
import stream_uf_ref as S
import union_find_ref as U
import wide_uf_ref as W


# ---- 1. the restatement -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,model,T,w,c", [(3, "DP", 9, 2, 1), (5, "DP", 33, 10, 5), (5, "X", 20, 16, 16), (7, "DP", 20, 14, 7), (5, "DP", 12, 16, 3)])
def test_restatement_is_the_narrow_one_where_both_apply(d, model, T, w, c):
    rng = np.random.default_rng(d * 100 + w)
    syn = np.zeros((6, T, d + 1, d + 1), dtype=np.uint8)
    for comp in range(2):
        bits = np.stack([S.sample_component_rows(d, comp, T, 0.02, rng, model)[1] for _ in range(len(syn))])
        syn |= W.node_syndromes(d, comp, bits)
    got, want = W.decode(d, syn, w, c), S.decode(d, syn, w, c)
    for a, b in zip(got[:4], want[:4]):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    assert got[4] == want[4] and all(np.array_equal(a, b) for a, b in zip(got[5], want[5]))
    assert got[2].sum() > 0                                                            # (not vacuous)


def _d9_streams(T, n, p, seed):
    rng = np.random.default_rng(seed)
    syn = np.zeros((n, T, 10, 10), dtype=np.uint8)
    for comp in range(2):
        bits = np.stack([S.sample_component_rows(9, comp, T, p, rng, "DP")[1] for _ in range(n)])
        syn |= W.node_syndromes(9, comp, bits)
    return syn


@pytest.mark.parametrize("w", [6, 32])
def test_one_window_is_the_volume_decoder_at_d9(w):
    T = 6
    syn = _d9_streams(T, 4, 0.02, 9)
    frame, weight, ndef, rounds, windows, _ = W.decode(9, syn, w, 1)
    assert windows == 1 and ndef.sum() > 0 and frame.any()
    # union_find_ref.decode packs M into int64, which 81 qubits overflow: its decode_component, which it tabulates, is compared per component
    for comp in range(2):
        rows = M.Component(9, comp).defects(syn)
        plane = ((frame.reshape(len(syn), -1) == 1) | (frame.reshape(len(syn), -1) == 2)) if comp == 0 else frame.reshape(len(syn), -1) >= 2
        for i in range(len(syn)):
            M0, W0, n0, r0 = U.decode_component(9, comp, rows[i], T)
            assert sum(int(b) << q for q, b in enumerate(plane[i])) == M0 and (weight[i, comp], ndef[i, comp], rounds[i, comp]) == (W0, n0, r0)


def test_schedule_limits():
    for T, w, c in ((0, 4, 2), (5, 0, 1), (5, 33, 1), (5, 4, 5), (5, 4, 0)):
        with pytest.raises(ValueError):
            W.check_schedule(T, w, c)
    W.check_schedule(1, 32, 32)
    with pytest.raises(ValueError):
        S.check_schedule(40, 17, 1)                                                    # (what the narrow restatement cannot run)


@pytest.mark.parametrize("d,T,n", [(9, 40, 3), (13, 40, 2)])
@pytest.mark.parametrize("w,c", [(18, 9), (32, 16), (1, 1), (32, 1)])
def test_closing_syndrome_rule(d, T, n, w, c):
    """Section 17's rule: the committed correction's syndrome, together with the last-round time edges the final window committed, is the stream's last
    syndrome -- the frame closes every defect the stream has."""
    if (w, c) == (32, 1):
        T = 36                                                                         # (five windows of 32 rounds are enough to cross the carry at every round)
    rng = np.random.default_rng(d + w)
    for comp in range(2):
        C = M.Component(d, comp)
        for i in range(n):
            rows, s = S.sample_component_rows(d, comp, T, 0.01, rng, "DP")
            r = W.stream_component(d, comp, rows, w, c)
            plane = np.array([(r["M"] >> q) & 1 for q in range(d * d)], dtype=np.int64)
            assert np.array_equal(((plane @ C.H) & 1) ^ r["last"], s[T - 1]), (d, comp, i, w, c)
            assert r["windows"] == S.n_windows(T, w, c) and r["ndef"] == int(rows.sum())


def test_hand_cases_of_the_restatement():
    """No defect: no correction.  A same-site defect pair straddling the commit line is one time edge, committed by the first window and cancelled by its
    carry in the second, whatever d."""
    for d in (9, 15):
        n, w, c = (d * d - 1) // 2, 2 * d, d
        for comp in range(2):
            rows = np.zeros((3 * d, n), dtype=np.int64)
            assert W.stream_component(d, comp, rows, w, c)["W"] == 0
            rows[c - 1, n // 2] = rows[c, n // 2] = 1
            r = W.stream_component(d, comp, rows, w, c)
            assert (r["M"], r["W"], r["ndef"]) == (0, 1, 2) and not r["last"].any()


# ---- 2. validation before any library call ---------------------------------------------------------------------------------------------------------
def _no_library(monkeypatch):
    _lib = importlib.import_module("deepq-decoding_amd._lib")

    def no_library(*a, **k):
        raise AssertionError("a library call was made before the arguments were validated")
    monkeypatch.setattr(_lib, "lib", no_library)
    monkeypatch.setattr(_lib, "require_gpu", no_library)
    monkeypatch.setattr(_lib, "check", no_library)


def _stub(**kw):
    return types.SimpleNamespace(**dict(dict(d=9, error_model="DP", use_Y=False, volume_depth=5, wide=True, n_envs=8, p_phys=0.01, p_meas=0.01, seed=(1, 2)), **kw))


def test_arguments_are_validated_before_the_library_is_touched(dq, monkeypatch):
    _no_library(monkeypatch)
    DW = dq.decoder_wide
    assert dq.stream_decode_wide is DW.stream_decode_wide and dq.memory_experiment_wide is DW.memory_experiment_wide and dq.WideEvaluator is DW.WideEvaluator
    syn = np.zeros((2, 40, 10, 10), dtype=np.uint8)
    for d in (1, 2, 4, 17, 9.0, True, None):
        with pytest.raises(ValueError):
            DW.stream_decode_wide(syn, d)
        with pytest.raises(ValueError):
            DW.WideEvaluator(d, "DP")
    with pytest.raises(ValueError):
        DW.WideEvaluator(9, "Y")
    for bad in (np.full((2, 40, 10, 10), 2, dtype=np.uint8), np.zeros((2, 40, 10, 9), dtype=np.uint8), np.zeros((2, 40, 8, 8), dtype=np.uint8),
                np.zeros((40, 10), dtype=np.uint8), np.zeros((2, 40, 10, 10), dtype=np.int32), np.zeros((0, 40, 10, 10), dtype=np.uint8),
                np.zeros((2, 0, 10, 10), dtype=np.uint8), [[0]]):
        with pytest.raises(ValueError):
            DW.stream_decode_wide(bad, 9)
    for kw in (dict(window=0), dict(window=33), dict(window=2.0), dict(window=True), dict(commit=0), dict(window=4, commit=5), dict(commit=19), dict(chunk=0),
               dict(chunk=True)):
        with pytest.raises(ValueError):
            DW.stream_decode_wide(syn, 9, **kw)
    for kw in (dict(window=0), dict(window=33), dict(window=True), dict(chunk=0)):
        with pytest.raises(ValueError):
            DW.WideEvaluator(9, "DP", **kw)
    # the defaults and the limits
    assert DW.check_wide_schedule(3, 7, None, None) == (7, 6, 3) and DW.check_wide_schedule(9, 40, None, None) == (40, 18, 9)
    assert DW.check_wide_schedule(13, 1000, None, None) == (1000, 26, 13) and DW.check_wide_schedule(15, 1 << 20, None, None) == (1 << 20, 30, 15)
    assert DW.check_wide_schedule(15, 3, 32, 32) == (3, 32, 32) and DW.check_wide_schedule(15, 3, 32, None) == (3, 32, 16)
    for T in (0, (1 << 20) + 1, 2.5):
        with pytest.raises(ValueError):
            DW.check_wide_schedule(9, T, None, None)
    assert DW.check_wide_stream_args(syn, 9) == (9, 2, False, 40, 18, 9, DW.DEFAULT_CHUNK)
    assert DW.check_wide_stream_args(syn[0], 9, 32, 1, 7) == (9, 1, True, 40, 32, 1, 7)
    # validation passes: the next thing touched is the library
    with pytest.raises(AssertionError, match="library call"):
        DW.stream_decode_wide(syn, 9)
    # a foreign evaluator: another lattice or another window
    ev = lambda **kw: types.SimpleNamespace(**dict(dict(d=9, error_model="DP", window=18, chunk=4, device="cpu"), **kw))
    DW.check_wide_stream_args(syn, 9, evaluator=ev())
    for foreign in (ev(window=16), ev(d=11)):
        with pytest.raises(ValueError):
            DW.stream_decode_wide(syn, 9, evaluator=foreign)
        with pytest.raises(ValueError):
            DW.memory_experiment_wide((9, "DP"), 16, 40, p_phys=0.01, seed=(1, 2), evaluator=foreign)
    with pytest.raises(ValueError):
        DW.memory_experiment_wide((9, "DP"), 16, 40, p_phys=0.01, seed=(1, 2), evaluator=ev(error_model="X"))
    # memory_experiment_wide: the lattice, the schedule, the runs and the rates
    for lat in ((9,), (9, "DP", False), (8, "DP"), (9, "Y"), None, 9, types.SimpleNamespace(d=9)):
        with pytest.raises(ValueError):
            DW.memory_experiment_wide(lat, 16, 40, p_phys=0.01, seed=(1, 2))
    for args, kw in (((16, 0), {}), ((16, 40), dict(window=33)), ((16, 40), dict(window=4, commit=5)), ((0, 40), {}), ((16, 40), dict(p_phys=1.5)),
                     ((16, 40), dict(rates=[0.01], p_phys=0.01)), ((16, 40), dict(rates=[])), ((16, 40), dict(rates=[0.01, 0.01])), ((16, 40), dict(chunk=0)),
                     ((16, 40), dict(seed=(1,))), ((16, 40), dict(env_id_base=-1)), ((16, 40), dict(p_meas=0.1)), ((16, 40), dict(env_id_base=1 << 32)),
                     ((2.0, 40), {})):
        with pytest.raises(ValueError):
            DW.memory_experiment_wide(_stub(), *args, **kw)
    for kw in (dict(), dict(p_phys=0.01), dict(seed=(1, 2))):                          # a tuple has no rates and no seed of its own
        with pytest.raises(ValueError):
            DW.memory_experiment_wide((9, "DP"), 16, 40, **kw)
    got = DW.check_wide_experiment_args(_stub(d=15, error_model="X", p_phys=0.02, p_meas=0.03, seed=(5, 6)), 16, 40)
    assert got == (15, "X", 40, 30, 15, 16, 0.02, 0.03, (5, 6), 0, 16, None, DW.DEFAULT_CHUNK)
    got = DW.check_wide_experiment_args((9, "DP"), 4, 40, rates=[0.01, 0.03], p_meas=0.0, seed=(5, 6), env_id_base=7)
    assert got[5] == 8 and got[10] == 4 and got[11] == [0.01, 0.03] and got[9] == 7
    assert np.array_equal(got[6], [0.01] * 4 + [0.03] * 4) and np.array_equal(got[7], np.zeros(8))
    with pytest.raises(AssertionError, match="library call"):
        DW.memory_experiment_wide(_stub(), 16, 40)
    with pytest.raises(AssertionError, match="library call"):
        DW.memory_experiment_wide(_stub(wide=False, d=5), 16, 40)                      # an environment of either backend


def test_the_narrow_entry_points_still_refuse_d9(dq, monkeypatch):
    _no_library(monkeypatch)
    D = dq.decoder
    narrow = lambda **kw: types.SimpleNamespace(**dict(dict(d=9, error_model="DP", use_Y=False, volume_depth=5, wide=False, n_envs=8, identity_index=162,
                                                            p_phys=0.01, p_meas=0.01, seed=(1, 2)), **kw))
    with pytest.raises(NotImplementedError):
        D.stream_decode(np.zeros((2, 40, 10, 10), dtype=np.uint8), narrow())
    with pytest.raises(NotImplementedError):
        D.memory_experiment(narrow(), 16, 40)
    with pytest.raises(NotImplementedError):
        D.memory_experiment(narrow(d=5, wide=True), 16, 40)
    assert D.STREAM_MAX_WINDOW == 16
    with pytest.raises(ValueError):
        D.check_stream_schedule(5, 40, 17, None)


# ---- 3. the C ABI --------------------------------------------------------------------------------------------------------------------------------------
def test_wide_abi_is_declared_and_bound():
    L = importlib.import_module("deepq-decoding_amd._lib")
    lib = L.lib()
    assert lib.dq_version() == 8                                                       # new capability = the presence of the new symbols
    header = open(os.path.join(os.path.dirname(L.__file__), "..", "include", "deepq_hip.h")).read()
    vp, i, dbl, u32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_uint32
    want = {"dq_wide_uf_create": (i, [i, i, i, i, ctypes.POINTER(vp)]),
            "dq_wide_uf_destroy": (None, [vp]),
            "dq_wide_uf_decode": (i, [vp, vp, i, i, i, vp, vp, vp, vp, vp]),
            "dq_wide_uf_run": (i, [vp, i, i, i, u32, ctypes.POINTER(u32), dbl, dbl, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
            "dq_wide_uf_verdict": (i, [vp, vp, vp, i, vp, vp])}
    for name, sig in want.items():
        assert name + "(" in header and hasattr(lib, name) and L.SIGNATURES[name] == sig, name
    doc = header.split("Union-find stream decoding for any odd d")[1].split("typedef struct dq_wide_uf")[0]
    assert "not thread-safe" in doc and "one host thread" in doc and "one stream at a time" in doc and "DQ_ERR_UNSUPPORTED" in doc
    seed = (u32 * 2)(1, 2)
    h = vp()
    # DQ_ERR_INVALID on null handles and bad arguments, no device touched
    assert lib.dq_wide_uf_decode(None, None, 1, 1, 1, None, None, None, None, None) == -1
    assert lib.dq_wide_uf_run(None, 1, 1, 1, 0, seed, 0.01, 0.01, None, None, None, None, None, None, None, None, None, None) == -1
    assert lib.dq_wide_uf_verdict(None, None, None, 1, None, None) == -1
    assert lib.dq_wide_uf_create(9, 1, 18, 4, None) == -1
    for d, model, window, streams in ((1, 1, 2, 4), (4, 1, 8, 4), (17, 1, 32, 4), (9, 3, 18, 4), (9, -1, 18, 4), (9, 1, 0, 4), (9, 1, 33, 4), (9, 1, 18, 0)):
        assert lib.dq_wide_uf_create(d, model, window, streams, ctypes.byref(h)) == -1 and not h.value, (d, model, window, streams)
    lib.dq_wide_uf_destroy(None)
    # the existing entry points keep their signatures
    assert L.SIGNATURES["dq_stream_decode_uf"] == (i, [vp, vp, i, i, i, vp, vp, vp, vp, vp])
    assert L.SIGNATURES["dq_stream_run_uf"] == (i, [vp, vp, i, i, i, u32, ctypes.POINTER(u32), dbl, dbl, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp])
    digest = importlib.import_module("deepq-decoding_amd._digest")
    import glob
    names = {os.path.basename(f) for f in glob.glob(os.path.join(digest.HERE, "csrc", "*"))}
    assert {"uf_wide_dev.h", "uf_wide.hip"} <= names
    assert lib.dq_build_digest().decode() == digest.csrc_digest()


# ---- 4. plumbing with stubs ------------------------------------------------------------------------------------------------------------------------------
class _Ptr:
    def __init__(self, p):
        self.p = p

    def data_ptr(self):
        return self.p


def test_evaluator_methods_hand_their_arguments_to_the_library(dq, monkeypatch):
    DW = dq.decoder_wide
    L = importlib.import_module("deepq-decoding_amd._lib")
    monkeypatch.setattr(L, "check", lambda status: None)
    calls = []
    ev = object.__new__(DW.WideEvaluator)
    ev._h, ev._stream = "handle", lambda: "stream"
    ev.L = types.SimpleNamespace(dq_wide_uf_decode=lambda *a: calls.append(("decode",) + a), dq_wide_uf_run=lambda *a: calls.append(("run",) + a),
                                 dq_wide_uf_verdict=lambda *a: calls.append(("verdict",) + a), dq_decode_count=lambda *a: calls.append(("count",) + a),
                                 dq_wide_uf_destroy=lambda h: None)
    ev.decode_into(_Ptr(10), 3, 40, 5, _Ptr(11))
    assert calls.pop() == ("decode", "handle", 10, 3, 40, 5, 11, None, None, None, "stream")
    ev.decode_into(_Ptr(10), 3, 40, 5, _Ptr(11), _Ptr(12), _Ptr(13), _Ptr(14))
    assert calls.pop() == ("decode", "handle", 10, 3, 40, 5, 11, 12, 13, 14, "stream")
    ev.run_into(3, 40, 5, (1 << 32) + 9, (7, 8), 0.01, 0.02, _Ptr(20), _Ptr(21), _Ptr(22))
    got = calls.pop()
    assert got[:6] == ("run", "handle", 3, 40, 5, 9) and list(got[6]) == [7, 8] and got[7:] == (0.01, 0.02, None, None, 20, 21, 22, None, None, None, None, "stream")
    ph, pm = np.array([0.01, 0.02, 0.03]), np.array([0.0, 0.0, 0.1])
    ev.run_into(3, 40, 5, 0, (7, 8), ph, pm, _Ptr(20), _Ptr(21), _Ptr(22), _Ptr(23), _Ptr(24), _Ptr(25), _Ptr(26))
    got = calls.pop()
    assert got[7:] == (0.0, 0.0, ph.ctypes.data, pm.ctypes.data, 20, 21, 22, 23, 24, 25, 26, "stream")
    ev.verdict_into(_Ptr(30), None, 3, _Ptr(31))
    assert calls.pop() == ("verdict", "handle", 30, None, 3, 31, "stream")
    counters = types.SimpleNamespace(shape=(2, 9), data_ptr=lambda: 44)
    ev.count_into(_Ptr(40), _Ptr(41), None, _Ptr(43), 3, 5, 4, counters)
    assert calls.pop() == ("count", 40, 41, None, 43, 3, 5, 4, 2, 44, "stream")
    ev._h = None


class _FakeEvaluator:
    """Stands for a WideEvaluator on CPU tensors: the run marks stream i's frame with the low bits of its lattice id, the verdict calls that a success when
    the id is even, the counters are summed as dq_decode_count sums them."""

    def __init__(self, d, window, chunk, model="DP"):
        self.d, self.error_model, self.window, self.chunk, self.device = d, model, window, chunk, "cpu"
        self.runs, self.decodes = [], []

    def decode_into(self, syndromes, m, T, commit, frame, weight=None, n_defects=None, rounds=None):
        self.decodes.append((m, T, commit))
        frame.zero_()
        frame.reshape(m, -1)[:, 0] = syndromes.reshape(m, -1)[:, 0]
        for x in (weight, n_defects, rounds):
            x.fill_(m)

    def run_into(self, m, T, commit, lattice_id, seed, p_phys, p_meas, hidden, trivial, frame, weight=None, n_defects=None, rounds=None, syndromes=None):
        import torch
        self.runs.append((m, T, commit, lattice_id, seed, p_phys if isinstance(p_phys, float) else tuple(p_phys), syndromes is not None))
        ids = torch.arange(lattice_id, lattice_id + m)
        hidden.zero_()
        frame.zero_()
        frame.reshape(m, -1)[:, 0] = (ids & 3).to(torch.uint8)
        trivial.copy_((ids % 5 == 0).to(torch.uint8))
        if syndromes is not None:
            syndromes.fill_(1)

    def verdict_into(self, hidden, frame, m, out):
        import torch
        ok = (frame.reshape(m, -1)[:, 0] & 1) == 0 if frame is not None else torch.zeros(m, dtype=torch.bool)
        out.copy_(ok.to(torch.uint8) * 8)

    def count_into(self, verdict, trivial, status, n_corr, m, first, block, counters):
        for i in range(m):
            b = (first + i) // block
            counters[b, 0] += 1
            counters[b, 1] += int(trivial[i])
            counters[b, 3] += int(verdict[i]) // 8
            counters[b, 5] += int(status[i] == 1) if status is not None else 0
            counters[b, 8] += int(n_corr[i]) if n_corr is not None else 0


def _cpu_torch(monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "device", lambda dev: contextlib.nullcontext())
    monkeypatch.setattr(torch.cuda, "current_stream", lambda dev=None: types.SimpleNamespace(synchronize=lambda: None))


def test_stream_decode_wide_chunks_keep_the_order(dq, monkeypatch):
    _cpu_torch(monkeypatch)
    DW = dq.decoder_wide
    syn = np.zeros((10, 40, 10, 10), dtype=np.uint8)
    syn[:, 0, 0, 0] = np.arange(10) & 1
    ev = _FakeEvaluator(9, 32, 4)
    r = DW.stream_decode_wide(syn, 9, window=32, commit=3, evaluator=ev, to_host=True)
    assert ev.decodes == [(4, 40, 3), (4, 40, 3), (2, 40, 3)] and r.windows == 4 and isinstance(r, dq.decoder.StreamResult)
    assert np.array_equal(r.frame.reshape(10, -1)[:, 0], np.arange(10) & 1) and r.frame.shape == (10, 9, 9) and r.weight.shape == (10, 2)
    assert np.array_equal(r.weight[:, 0], [4] * 8 + [2] * 2) and r.weight.dtype == np.int32


def test_memory_experiment_wide_chunks_blocks_and_streams(dq, monkeypatch):
    _cpu_torch(monkeypatch)
    DW = dq.decoder_wide
    env = _stub()
    ev = _FakeEvaluator(9, 18, 7)
    r = DW.memory_experiment_wide(env, 20, 40, evaluator=ev, env_id_base=100, seed=(3, 4), p_phys=0.02, no_decoder=True)
    assert ev.runs == [(7, 40, 9, 100, (3, 4), 0.02, False), (7, 40, 9, 107, (3, 4), 0.02, False), (6, 40, 9, 114, (3, 4), 0.02, False)]
    ids = np.arange(100, 120)
    assert isinstance(r, dq.decoder.EvalResult)
    assert r.counters["volumes"] == 20 and r.counters["success"] == int((ids % 2 == 0).sum()) and r.counters["identity"] == 20
    assert r.counters["corrections"] == int((ids & 3 != 0).sum()) and r.counters["trivial"] == int((ids % 5 == 0).sum()) and r.inexact == 0
    assert r.no_decoder.counters["volumes"] == 20 and r.no_decoder.counters["success"] == 0 and r.p_phys == 0.02 and r.p_meas == 0.02
    # the environment's own rates and seed are the defaults; a tuple takes them as arguments
    ev = _FakeEvaluator(9, 18, 32)
    DW.memory_experiment_wide(env, 3, 40, evaluator=ev)
    DW.memory_experiment_wide((9, "DP"), 3, 40, evaluator=ev, p_phys=0.05, seed=(9, 9))
    assert ev.runs == [(3, 40, 9, 0, (1, 2), 0.01, False), (3, 40, 9, 0, (9, 9), 0.05, False)]
    # rates: one block of n_runs streams per rate, the chunk's scalar form where a chunk holds one rate
    ev = _FakeEvaluator(15, 32, 8)
    out = DW.memory_experiment_wide((15, "DP"), 8, 70, window=32, commit=1, rates=[0.01, 0.03], seed=(1, 2), evaluator=ev)
    assert list(out) == [0.01, 0.03] and [x[:4] + x[5:] for x in ev.runs] == [(8, 70, 1, 0, 0.01, False), (8, 70, 1, 8, 0.03, False)]
    assert all(v.counters["volumes"] == 8 for v in out.values()) and out[0.03].p_phys == 0.03 and out[0.03].no_decoder is None
    ev = _FakeEvaluator(15, 32, 6)
    DW.memory_experiment_wide((15, "DP"), 4, 70, window=32, commit=32, rates=[0.01, 0.03], seed=(1, 2), evaluator=ev)
    assert [x[0] for x in ev.runs] == [6, 2] and ev.runs[0][5] == (0.01,) * 4 + (0.03,) * 2 and ev.runs[1][5] == 0.03
    # return_streams: all streams stay, in order
    ev = _FakeEvaluator(9, 18, 7)
    timings = {}
    r, streams = DW.memory_experiment_wide(env, 20, 12, evaluator=ev, return_streams=True, timings=timings)
    assert tuple(streams["syndromes"].shape) == (20, 12, 10, 10) and bool((streams["syndromes"] == 1).all()) and all(x[6] for x in ev.runs)
    assert np.array_equal(streams["frame"].reshape(20, -1)[:, 0].numpy(), np.arange(20) & 3) and tuple(streams["hidden"].shape) == (20, 9, 9)
    assert np.array_equal(streams["trivial"].numpy(), (np.arange(20) % 5 == 0).astype(np.uint8)) and set(timings) == {"run", "verdict"}
