"""Sliding-window union-find decoding of syndrome streams, host side: tests/stream_uf_ref.py -- the numpy statement the device is
compared with bit for bit in tests/test_stream_uf_gpu.py -- checked on its own (the closing-syndrome rule stream-wide, the one-window equality with
union_find_ref, the window count, the carry rule on hand cases); then the validators before any library call, the C ABI and the Python plumbing."""
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

UF = "union_find"
WINDOWS = [(1, 1), (2, 1), (10, 5), (16, 15), (16, 16), (7, 7)]
STREAMS = {"d3_T7": (3, 7, 0.05, 48), "d5_T33": (5, 33, 0.011, 48), "d7_T64": (7, 64, 0.02, 16)}


def _plane(d, mask):
    return (mask >> np.arange(d * d)) & 1


# ---- 1. the restatement alone ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(STREAMS))
def test_closing_syndrome_holds_stream_wide(name):
    """sigma(F) xor S_{T-1} = the nodes whose last-round time edge to B the final window committed, for every stream and every (window, commit)."""
    d, T, p, n = STREAMS[name]
    weights = {}
    for i in range(n):
        comp = i & 1
        C = M.Component(d, comp)
        rows, s = S.sample_component_rows(d, comp, T, p, np.random.default_rng(1000 + i))
        for w, c in WINDOWS:
            r = S.stream_component(d, comp, rows, w, c)
            sig = (_plane(d, r["M"]) @ C.H) & 1
            assert np.array_equal(sig ^ s[-1], r["last"]), (name, i, w, c)
            assert r["ndef"] == rows.sum() and r["windows"] == S.n_windows(T, w, c)
            assert r["W"] >= int(_plane(d, r["M"]).sum()) + int(r["last"].sum())       # every frame qubit and every closing edge is a committed edge
            weights[(w, c)] = weights.get((w, c), 0) + r["W"]
    print(name, weights)
    assert min(weights.values()) > 0


@pytest.mark.parametrize("d,T", [(3, 1), (3, 2), (5, 5), (5, 16), (7, 7)])
def test_one_window_is_the_whole_volume_decode(d, T):
    rng = np.random.default_rng(d * 100 + T)
    vol = (rng.random((12, T, d + 1, d + 1)) < 0.08).astype(np.uint8)
    want = U.decode(d, vol, T)
    assert want[1].sum() > 0
    for w in range(T, 17):
        for c in sorted({1, (w + 1) // 2, w}):
            got = S.decode(d, vol, w, c)
            assert got[4] == 1 and all(np.array_equal(a, b) for a, b in zip(got[:4], want)), (d, T, w, c)


def test_window_count_formula():
    for T in (1, 2, 7, 16, 17, 33, 40, 64, 1000):
        for w in range(1, 17):
            for c in range(1, w + 1):
                k, a = 1, 0
                while a + w < T:
                    a += c
                    k += 1
                assert S.n_windows(T, w, c) == k, (T, w, c)
                D = importlib.import_module("deepq-decoding_amd.decoder")
                assert D.stream_windows(T, w, c) == k


def test_carry_rule_on_hand_cases():
    d = 7
    for comp in (0, 1):
        C = M.Component(d, comp)
        n = C.n
        u = next(j for j, cell in enumerate(C.cells) if tuple(cell) in ((3, 4), (4, 4)))      # the central plaquette: three edges from the spatial boundary
        # a lone defect in round commit - 1 = 0, window 2: the future boundary is two edges away, so it leaves by the time edge, window after window, until
        # the final window lets it reach B: one committed edge per round of the stream, no qubit
        T = 4
        rows = np.zeros((T, n), dtype=np.int64)
        rows[0, u] = 1
        edges, _ = S.window_edges(d, comp, rows[:2], 2)
        assert edges == [d * d + u, (d * d + n) + d * d + u]                               # (u, 0) -- (u, 1) -- B
        r = S.stream_component(d, comp, rows, 2, 1)
        want_last = np.zeros(n, dtype=np.int64)
        want_last[u] = 1
        assert (r["M"], r["W"], r["ndef"], r["windows"]) == (0, T, 1, 3) and np.array_equal(r["last"], want_last)
        # a same-site pair straddling the commit line (rounds c - 1 and c): the first window commits their time edge once and carries u, which cancels the
        # defect of round c in the next window; nothing else is ever committed
        w, c, T = 4, 2, 9
        rows = np.zeros((T, n), dtype=np.int64)
        rows[c - 1, u] = rows[c, u] = 1
        r = S.stream_component(d, comp, rows, w, c)
        assert (r["M"], r["W"], r["ndef"], r["rounds"]) == (0, 1, 2, 1) and not r["last"].any()
        # the same pair inside the committed rounds: one edge, no carry needed -- and inside the uncommitted rounds: decoded again by the next window
        for t0 in (0, c):
            rows = np.zeros((T, n), dtype=np.int64)
            rows[t0, u] = rows[t0 + 1, u] = 1
            r = S.stream_component(d, comp, rows, w, c)
            assert (r["M"], r["W"], r["ndef"]) == (0, 1, 2) and not r["last"].any()
            assert r["rounds"] == (1 if t0 == 0 else 2)                                  # (seen by one window, by two)


# ---- 2. validation before any library call ---------------------------------------------------------------------------------------------------------
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


def test_arguments_are_validated_before_the_library_is_touched(dq, monkeypatch):
    _no_library(monkeypatch)
    D = dq.decoder
    syn = np.zeros((2, 40, 6, 6), dtype=np.uint8)
    assert D.METHODS == ("matching", "union_find")
    with pytest.raises(NotImplementedError, match="committed rounds"):
        D.stream_decode(syn, _stub(), method="matching")
    for bad in ("uf", None, 1):
        with pytest.raises(ValueError):
            D.stream_decode(syn, _stub(), method=bad)
    with pytest.raises(NotImplementedError):
        D.stream_decode(syn, _stub(wide=True))
    with pytest.raises(NotImplementedError):
        D.stream_decode(np.zeros((2, 40, 10, 10), dtype=np.uint8), _stub(d=9))
    with pytest.raises(NotImplementedError):
        D.memory_experiment(_stub(wide=True), 16, 40)
    with pytest.raises(NotImplementedError):
        D.memory_experiment(_stub(d=9), 16, 40)
    for bad in (np.full((2, 40, 6, 6), 2, dtype=np.uint8), np.zeros((2, 40, 6, 5), dtype=np.uint8), np.zeros((2, 40, 8, 8), dtype=np.uint8),
                np.zeros((40, 6), dtype=np.uint8), np.zeros((2, 40, 6, 6), dtype=np.int32), np.zeros((0, 40, 6, 6), dtype=np.uint8),
                np.zeros((2, 0, 6, 6), dtype=np.uint8), [[0]]):
        with pytest.raises(ValueError):
            D.stream_decode(bad, _stub())
    for kw in (dict(window=0), dict(window=17), dict(window=2.0), dict(window=True), dict(commit=0), dict(window=4, commit=5), dict(commit=11), dict(chunk=0)):
        with pytest.raises(ValueError):
            D.stream_decode(syn, _stub(), **kw)
    # the defaults and the schedule's limits
    assert D.check_stream_schedule(3, 7, None, None) == (7, 6, 3) and D.check_stream_schedule(5, 33, None, None) == (33, 10, 5)
    assert D.check_stream_schedule(7, 1000, None, None) == (1000, 14, 7) and D.check_stream_schedule(7, 1 << 20, 16, None) == (1 << 20, 16, 8)
    assert D.check_stream_schedule(5, 3, 16, 16) == (3, 16, 16)
    for T in (0, (1 << 20) + 1, 2.5):
        with pytest.raises(ValueError):
            D.check_stream_schedule(5, T, None, None)
    # env.volume_depth is not consulted; one stream without the batch axis is accepted: validation passes and the stub fails as "not an environment handle"
    ok = D.check_stream_args(_stub(volume_depth=3), syn[0])
    assert ok == (5, "DP", False, 1, True, 40, 10, 5)
    assert D.check_stream_args(_stub(), syn, 16, 1) == (5, "DP", False, 2, False, 40, 16, 1)
    with pytest.raises(TypeError):
        D.stream_decode(syn, _stub())
    # a foreign evaluator: another lattice, or a volume_depth that is not the window
    ev = lambda **kw: types.SimpleNamespace(**dict(dict(d=5, error_model="DP", use_Y=False, volume_depth=10, _h=None), **kw))
    D.check_stream_args(_stub(), syn, evaluator=ev())
    for foreign in (ev(volume_depth=5), ev(d=7), ev(error_model="X"), ev(use_Y=True)):
        with pytest.raises(ValueError):
            D.stream_decode(syn, _stub(), evaluator=foreign)
        with pytest.raises(ValueError):
            D.memory_experiment(_stub(), 16, 40, evaluator=foreign)
    with pytest.raises(ValueError):
        D.stream_decode(syn, _stub(), window=16, evaluator=ev())
    # memory_experiment: the schedule, the runs and the rates
    for args, kw in (((16, 0), {}), ((16, 40), dict(window=17)), ((16, 40), dict(window=4, commit=5)), ((0, 40), {}), ((16, 40), dict(p_phys=1.5)),
                     ((16, 40), dict(rates=[0.01], p_phys=0.01)), ((16, 40), dict(rates=[])), ((16, 40), dict(rates=[0.01, 0.01])), ((16, 40), dict(chunk=0)),
                     ((16, 40), dict(seed=(1,))), ((16, 40), dict(env_id_base=-1)), ((16, 40), dict(p_meas=0.1))):
        with pytest.raises(ValueError):
            D.memory_experiment(_stub(), *args, **kw)
    with pytest.raises(TypeError):
        D.memory_experiment(_stub(), 16, 40)


# ---- 3. the C ABI --------------------------------------------------------------------------------------------------------------------------------------
def test_stream_abi_is_declared_and_bound():
    L = importlib.import_module("deepq-decoding_amd._lib")
    lib = L.lib()
    assert lib.dq_version() == 8                                                       # new capability = the presence of the new symbols
    header = open(os.path.join(os.path.dirname(L.__file__), "..", "include", "deepq_hip.h")).read()
    vp, i, dbl, u32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_uint32
    want = {"dq_stream_decode_uf": (i, [vp, vp, i, i, i, vp, vp, vp, vp, vp]),
            "dq_stream_run_uf": (i, [vp, vp, i, i, i, u32, ctypes.POINTER(u32), dbl, dbl, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp])}
    for name, sig in want.items():
        assert "dq_status " + name + "(" in header and hasattr(lib, name) and L.SIGNATURES[name] == sig, name
    doc = header.split("Sliding-window union-find decoding")[1].split("dq_status dq_stream_decode_uf")[0]
    assert "not thread-safe" in doc and "one host thread" in doc and "one stream at a time" in doc
    seed = (u32 * 2)(1, 2)
    assert lib.dq_stream_decode_uf(None, None, 1, 1, 1, None, None, None, None, None) == -1      # DQ_ERR_INVALID on null handles, no device touched
    assert lib.dq_stream_run_uf(None, None, 1, 1, 1, 0, seed, 0.01, 0.01, None, None, None, None, None, None, None, None, None, None) == -1
    assert L.SIGNATURES["dq_decode_uf"] == (i, [vp, vp, i, vp, vp, vp, vp, vp])            # the existing entry point keeps its signature
    digest = importlib.import_module("deepq-decoding_amd._digest")
    import glob
    names = {os.path.basename(f) for f in glob.glob(os.path.join(digest.HERE, "csrc", "*"))}
    assert {"uf_dev.h", "uf_st.hip", "uf_stream.hip"} <= names
    assert lib.dq_build_digest().decode() == digest.csrc_digest()


# ---- 4. plumbing with stubs ------------------------------------------------------------------------------------------------------------------------------
class _Ptr:
    def __init__(self, p):
        self.p = p

    def data_ptr(self):
        return self.p


def test_evaluator_methods_hand_their_arguments_to_the_library(dq, monkeypatch):
    D = dq.decoder
    L = importlib.import_module("deepq-decoding_amd._lib")
    monkeypatch.setattr(L, "check", lambda status: None)
    calls = []
    ev = object.__new__(D.Evaluator)
    ev._h, ev._stream = "handle", lambda: "stream"
    ev.L = types.SimpleNamespace(dq_stream_decode_uf=lambda *a: calls.append(("decode",) + a), dq_stream_run_uf=lambda *a: calls.append(("run",) + a),
                                 dq_decode_eval_destroy=lambda h: None)
    ev.stream_uf_into(_Ptr(10), 3, 40, 5, _Ptr(11))
    assert calls.pop() == ("decode", "handle", 10, 3, 40, 5, 11, None, None, None, "stream")
    ev.stream_uf_into(_Ptr(10), 3, 40, 5, _Ptr(11), _Ptr(12), _Ptr(13), _Ptr(14))
    assert calls.pop() == ("decode", "handle", 10, 3, 40, 5, 11, 12, 13, 14, "stream")
    venv = types.SimpleNamespace(_h="env")
    ev.stream_run_into(venv, 3, 40, 5, (1 << 32) + 9, (7, 8), 0.01, 0.02, _Ptr(20), _Ptr(21), _Ptr(22))
    got = calls.pop()
    assert got[:7] == ("run", "handle", "env", 3, 40, 5, 9) and list(got[7]) == [7, 8] and got[8:] == (0.01, 0.02, None, None, 20, 21, 22, None, None, None, None, "stream")
    ph, pm = np.array([0.01, 0.02, 0.03]), np.array([0.0, 0.0, 0.1])
    ev.stream_run_into(venv, 3, 40, 5, 0, (7, 8), ph, pm, _Ptr(20), _Ptr(21), _Ptr(22), _Ptr(23), _Ptr(24), _Ptr(25), _Ptr(26))
    got = calls.pop()
    assert got[8:] == (0.0, 0.0, ph.ctypes.data, pm.ctypes.data, 20, 21, 22, 23, 24, 25, 26, "stream")
    ev._h = None


class _FakeEvaluator:
    """Stands for an Evaluator on CPU tensors: the run marks stream i's frame with the low bits of its lattice id, the verdict calls that a success when the
    id is even, the counters are summed as dq_decode_count sums them."""

    def __init__(self, d, window, chunk):
        self.d, self.error_model, self.use_Y, self.volume_depth, self.chunk = d, "DP", False, window, chunk
        self.runs = []

    def stream_run_into(self, venv, m, T, commit, lattice_id, seed, p_phys, p_meas, hidden, trivial, frame, weight=None, n_defects=None, rounds=None,
                        syndromes=None):
        import torch
        self.runs.append((m, T, commit, lattice_id, seed, p_phys if isinstance(p_phys, float) else tuple(p_phys), syndromes is not None))
        ids = torch.arange(lattice_id, lattice_id + m)
        hidden.zero_()
        frame.zero_()
        frame.reshape(m, -1)[:, 0] = (ids & 3).to(torch.uint8)
        trivial.copy_((ids % 5 == 0).to(torch.uint8))
        if syndromes is not None:
            syndromes.fill_(1)

    def verdict_into(self, venv, hidden, frame, m, out):
        import torch
        ok = (frame.reshape(m, -1)[:, 0] & 1) == 0 if frame is not None else torch.zeros(m, dtype=torch.bool)
        out.copy_(ok.to(torch.uint8) * 8)

    def count_into(self, verdict, trivial, status, n_corr, m, first, block, counters):
        import torch
        for i in range(m):
            b = (first + i) // block
            counters[b, 0] += 1
            counters[b, 1] += int(trivial[i])
            counters[b, 3] += int(verdict[i]) // 8
            counters[b, 5] += int(status[i] == 1) if status is not None else 0
            counters[b, 8] += int(n_corr[i]) if n_corr is not None else 0


def test_memory_experiment_chunks_blocks_and_streams(dq, monkeypatch):
    import torch
    D = dq.decoder
    monkeypatch.setattr(torch.cuda, "device", lambda dev: contextlib.nullcontext())
    env = _stub(_h=1, device="cpu")
    ev = _FakeEvaluator(5, 10, 7)
    r = D.memory_experiment(env, 20, 40, evaluator=ev, env_id_base=100, seed=(3, 4), p_phys=0.02, no_decoder=True)
    assert ev.runs == [(7, 40, 5, 100, (3, 4), 0.02, False), (7, 40, 5, 107, (3, 4), 0.02, False), (6, 40, 5, 114, (3, 4), 0.02, False)]
    ids = np.arange(100, 120)
    assert r.counters["volumes"] == 20 and r.counters["success"] == int((ids % 2 == 0).sum()) and r.counters["identity"] == 20
    assert r.counters["corrections"] == int((ids & 3 != 0).sum()) and r.counters["trivial"] == int((ids % 5 == 0).sum()) and r.inexact == 0
    assert r.no_decoder.counters["volumes"] == 20 and r.no_decoder.counters["success"] == 0 and r.p_phys == 0.02 and r.p_meas == 0.02
    # rates: one block of n_runs streams per rate, the chunk's scalar form where a chunk holds one rate
    ev = _FakeEvaluator(5, 16, 8)
    out = D.memory_experiment(env, 8, 33, window=16, commit=1, rates=[0.01, 0.03], evaluator=ev)
    assert list(out) == [0.01, 0.03] and [x[:4] + x[5:] for x in ev.runs] == [(8, 33, 1, 0, 0.01, False), (8, 33, 1, 8, 0.03, False)]
    assert all(v.counters["volumes"] == 8 for v in out.values()) and out[0.03].p_phys == 0.03 and out[0.03].no_decoder is None
    ev = _FakeEvaluator(5, 16, 6)
    D.memory_experiment(env, 4, 33, window=16, commit=16, rates=[0.01, 0.03], evaluator=ev)
    assert [x[0] for x in ev.runs] == [6, 2] and ev.runs[0][5] == (0.01,) * 4 + (0.03,) * 2 and ev.runs[1][5] == 0.03
    # return_streams: all streams stay, in order
    ev = _FakeEvaluator(5, 10, 7)
    timings = {}
    monkeypatch.setattr(torch.cuda, "current_stream", lambda dev=None: types.SimpleNamespace(synchronize=lambda: None))
    r, streams = D.memory_experiment(env, 20, 12, evaluator=ev, return_streams=True, timings=timings)
    assert tuple(streams["syndromes"].shape) == (20, 12, 6, 6) and bool((streams["syndromes"] == 1).all()) and all(x[6] for x in ev.runs)
    assert np.array_equal(streams["frame"].reshape(20, -1)[:, 0].numpy(), np.arange(20) & 3) and tuple(streams["hidden"].shape) == (20, 5, 5)
    assert np.array_equal(streams["trivial"].numpy(), (np.arange(20) % 5 == 0).astype(np.uint8)) and {"run", "verdict"} <= set(timings)


def test_stream_result_fields(dq):
    r = dq.decoder.StreamResult(1, 2, 3, 4, 5)
    assert (r.frame, r.weight, r.n_defects, r.rounds, r.windows) == (1, 2, 3, 4, 5)
