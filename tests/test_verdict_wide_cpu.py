"""The refereed verdict at d = 3 .. 15 without a GPU (decoder_wide.verdict_wide, referee="matching"; include/deepq_hip.h dq_wide_uf_verdict_refereed;
DESIGN.md section 22): the numpy restatement of tests/verdict_wide_ref.py against the Python matching referee plus the step's rule and against the narrow C
oracle environment, validation before any library call, the C ABI, the plumbing with stubs, and the input conditions of the GPU cases
(tests/test_verdict_wide_gpu.py), asserted here on the restatement alone so that a retune of a seed or a density cannot make those cases vacuous."""
import contextlib
import ctypes
import importlib
import os
import types

import numpy as np
import pytest

import verdict_wide_ref as V
from oracle import c_oracle, lattice, matching_referee


def _mask(row):
    return sum(1 << int(q) for q in np.flatnonzero(row))


# ---- 1. the restatement against the Python referee and the step's rule -----------------------------------------------------------------------------------
def _step_rule(d, model, hidden, frame=None):
    """Environments.py:139-151 on the residual, with oracle/matching_referee.MatchingReferee as the static decoder."""
    ref, masks = matching_referee.MatchingReferee(d, model), lattice.Masks(d)
    x, z = V.planes(hidden, frame)
    out = []
    for i in range(len(x)):
        xm, zm = _mask(x[i]), _mask(z[i])
        word = masks.syndrome_word(xm, zm)
        cls = (bin(xm & masks.col0_mask).count("1") & 1) + 2 * (bin(zm & masks.row0_mask).count("1") & 1)
        dec = ref.classify_word(word)
        reward = cls == 0 and word == 0
        done = not reward and dec != cls
        out.append((word == 0, cls, reward, not done, dec))
    return out


def _fields(b):
    b = int(b)
    return (bool(b & V.IN_CODESPACE), (b >> V.CLASS_SHIFT) & 3, bool(b & V.SUCCESS), bool(b & V.ALIVE), b >> V.DECODED_SHIFT)


def test_restatement_is_the_matching_referee_and_the_steps_rule_on_every_x_pattern_of_d3():
    hidden = V.exhaustive_d3("X")
    got = V.restatement(3, "X").verdict(hidden)
    assert [_fields(b) for b in got["byte"]] == _step_rule(3, "X", hidden)
    assert not got["inexact"].any()
    k = V.kinds(got["byte"])
    assert min(k.values()) > 0 and k["success"] == 16                # the X-plane stabilizer group of d = 3 has 2^4 elements


def test_restatement_is_the_matching_referee_and_the_steps_rule_on_d5_dp_residuals():
    rng = np.random.default_rng(55)
    hidden, frame = V.iid_hidden(5, 200, 0.06, rng), V.iid_hidden(5, 200, 0.03, rng)
    got = V.restatement(5, "DP").verdict(hidden, frame)
    want = _step_rule(5, "DP", hidden, frame)
    assert [_fields(b) for b in got["byte"]] == want
    assert sum(1 for w in want if not w[3]) >= 10 and sum(1 for w in want if w[3] and not w[0]) >= 10      # dead and alive outside the code space


def test_array_form_is_the_masks_form():
    """Restatement's sums are Masks.syndrome_word / referee_index / col0_mask / row0_mask, volume by volume, at a width of one and of four words."""
    for d, model in ((5, "X"), (9, "DP"), (15, "IIDXZ")):
        R = V.restatement(d, model)
        rng = np.random.default_rng(d)
        hidden, frame = V.iid_hidden(d, 12, 0.05, rng), V.iid_hidden(d, 12, 0.02, rng)
        frame[:3] = hidden[:3]                                          # (residuals in the code space too)
        got = R.verdict(hidden, frame)
        x, z = V.planes(hidden, frame)
        classify = lambda c, idx: int(R.match.classify_bits(c, np.array([[idx & (2 ** 64 - 1), idx >> 64]], dtype=np.uint64))[0][0])
        for i in range(len(x)):
            xm, zm = _mask(x[i]), _mask(z[i])
            w = R.masks.syndrome_word(xm, zm)
            for c, typ in ((0, 3), (1, 1)):
                assert int(got["bits"][c][i, 0]) | int(got["bits"][c][i, 1]) << 64 == R.masks.referee_index(w, typ)
            assert int(got["byte"][i]) == V.verdict_one(R.masks, model, xm, zm, classify), (d, i)


# ---- 2. the narrow C oracle environment --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["DP", "X"])
def test_restatement_is_the_narrow_oracle_environments_step_at_d5(model):
    n, d = 256, 5
    rng = np.random.default_rng(7 + len(model))
    x, z = rng.random((n, d * d)) < 0.04, rng.random((n, d * d)) < 0.04
    if model == "X":
        z[:] = False                                                    # the X model's lattices hold X errors only
    x[:4], z[:4] = False, False                                         # clean lattices: the reward
    hidden = V.codes(x, z).reshape(n, d, d)
    got = V.restatement(d, model).verdict(hidden)["byte"]
    env = c_oracle.COracleEnv(d=d, error_model=model, n_envs=n, p_phys=0.01, p_meas=0.01)      # (rate 0 never leaves the redraw of all-zero volumes)
    env.reset()
    for i in range(n):
        env.poke(i, _mask(x[i]), _mask(z[i]))
    env.step(np.full(n, env.num_actions - 1, dtype=np.int32), want_obs=False)
    assert np.array_equal(env.reward == 1, (got & V.SUCCESS) != 0)
    assert np.array_equal(env.done != 0, (got & V.ALIVE) == 0)
    assert (env.reward == 1).sum() >= 4 and (env.done != 0).sum() >= 1 and (env.done == 0).sum() >= 100, (int(env.reward.sum()), int(env.done.sum()))


# ---- 3. validation and the C ABI ----------------------------------------------------------------------------------------------------------------------------
def _no_library(monkeypatch):
    _lib = importlib.import_module("deepq-decoding_amd._lib")

    def no_library(*a, **k):
        raise AssertionError("a library call was made before the arguments were validated")
    monkeypatch.setattr(_lib, "lib", no_library)
    monkeypatch.setattr(_lib, "require_gpu", no_library)
    monkeypatch.setattr(_lib, "check", no_library)


def test_a_bad_referee_is_refused_before_the_library_is_touched(dq, monkeypatch):
    _no_library(monkeypatch)
    DW = dq.decoder_wide
    assert dq.verdict_wide is DW.verdict_wide
    hidden = np.zeros((4, 9, 9), dtype=np.uint8)
    for bad in ("lut", "union_find", "Matching", True, 1, b"matching", ("matching",)):
        with pytest.raises(ValueError, match="referee"):
            DW.verdict_wide(hidden, None, 9, referee=bad)
        with pytest.raises(ValueError, match="referee"):
            DW.memory_experiment_wide((9, "DP"), 16, 6, p_phys=0.01, seed=(1, 2), referee=bad)
        with pytest.raises(ValueError, match="referee"):
            DW.check_decode_benchmark_wide_args((9, "DP", False, 5), 16, p_phys=0.01, seed=(1, 2), referee=bad)
        with pytest.raises(ValueError, match="referee"):
            DW.WideEvaluator.verdict_into(object.__new__(DW.WideEvaluator), None, None, 1, None, referee=bad)
    assert DW.check_referee(None) is False and DW.check_referee("matching") is True
    # the other arguments of verdict_wide
    for kw in (dict(d=4), dict(d=9, error_model="Y"), dict(d=9, chunk=0), dict(d=11)):
        with pytest.raises(ValueError):
            DW.verdict_wide(hidden, None, referee="matching", **kw)
    with pytest.raises(ValueError):
        DW.verdict_wide(hidden, np.zeros((3, 9, 9), dtype=np.uint8), 9, referee="matching")
    with pytest.raises(ValueError):
        DW.verdict_wide(hidden + 4, None, 9, referee="matching")
    with pytest.raises(ValueError):
        DW.verdict_wide(hidden, None, 9, referee="matching", evaluator=types.SimpleNamespace(d=11, error_model="DP", chunk=4))
    import inspect
    agent = importlib.import_module("deepq-decoding_amd.agent")
    for fn in (DW.memory_experiment_wide, DW.score_decode_wide, DW.verdict_wide, agent.DQNAgent.decode_benchmark_wide, DW.WideEvaluator.verdict_into):
        assert inspect.signature(fn).parameters["referee"].default is None, fn


def test_refereed_verdict_abi_is_declared_and_bound():
    L = importlib.import_module("deepq-decoding_amd._lib")
    lib = L.lib()
    assert lib.dq_version() == 8                                                       # the capability is the symbol
    header = open(os.path.join(os.path.dirname(L.__file__), "..", "include", "deepq_hip.h")).read()
    vp, i = ctypes.c_void_p, ctypes.c_int
    assert "dq_wide_uf_verdict_refereed(dq_wide_uf* h, const dq_match* m, const uint8_t* hidden_dev, const uint8_t* frame_dev, int n" in header
    assert hasattr(lib, "dq_wide_uf_verdict_refereed") and L.SIGNATURES["dq_wide_uf_verdict_refereed"] == (i, [vp, vp, vp, vp, i, vp, vp, vp])
    assert L.SIGNATURES["dq_wide_uf_verdict"] == (i, [vp, vp, vp, i, vp, vp])         # the unrefereed entry point keeps its signature
    assert lib.dq_wide_uf_verdict_refereed(None, None, None, None, 1, None, None, None) == -1      # DQ_ERR_INVALID, no device touched
    doc = header.split("The refereed verdict at these sizes")[1].split("dq_status dq_wide_uf_verdict_refereed")[0]
    assert "DQ_ERR_INVALID" in doc and "re-zeroed" in doc and "inexact_dev" in doc
    digest = importlib.import_module("deepq-decoding_amd._digest")
    assert os.path.exists(os.path.join(digest.HERE, "csrc", "verdict_wide.hip"))
    assert lib.dq_build_digest().decode() == digest.csrc_digest()


# ---- 4. plumbing with stubs ---------------------------------------------------------------------------------------------------------------------------------
class _Ptr:
    def __init__(self, p):
        self.p = p

    def data_ptr(self):
        return self.p


def test_verdict_into_hands_its_arguments_to_the_library(dq, monkeypatch):
    DW = dq.decoder_wide
    L = importlib.import_module("deepq-decoding_amd._lib")
    monkeypatch.setattr(L, "check", lambda status: None)
    calls = []
    ev = object.__new__(DW.WideEvaluator)
    ev._h, ev._m, ev._stream, ev._referee = "handle", None, lambda: "stream", lambda: "referee"
    ev.L = types.SimpleNamespace(dq_wide_uf_verdict=lambda *a: calls.append(("plain",) + a),
                                 dq_wide_uf_verdict_refereed=lambda *a: calls.append(("refereed",) + a), dq_wide_uf_destroy=lambda h: None)
    ev.verdict_into(_Ptr(30), None, 3, _Ptr(31))
    assert calls.pop() == ("plain", "handle", 30, None, 3, 31, "stream")
    ev.verdict_into(_Ptr(30), _Ptr(32), 3, _Ptr(31), referee="matching", inexact=_Ptr(33))
    assert calls.pop() == ("refereed", "handle", "referee", 30, 32, 3, 31, 33, "stream")
    ev.verdict_into(_Ptr(30), None, 3, _Ptr(31), referee="matching")
    assert calls.pop() == ("refereed", "handle", "referee", 30, None, 3, 31, None, "stream")
    with pytest.raises(ValueError):
        ev.verdict_into(_Ptr(30), None, 3, _Ptr(31), inexact=_Ptr(33))      # flags without a referee
    assert not calls
    ev._h = None


def test_the_evaluator_owns_its_referee_handle(dq, monkeypatch):
    import torch
    DW = dq.decoder_wide
    L = importlib.import_module("deepq-decoding_amd._lib")
    monkeypatch.setattr(L, "check", lambda status: None)
    monkeypatch.setattr(torch.cuda, "device", lambda dev: contextlib.nullcontext())
    made, gone = [], []

    def create(d, out):
        made.append(d)
        ctypes.cast(out, ctypes.POINTER(ctypes.c_void_p))[0] = 0x1234
        return 0
    ev = object.__new__(DW.WideEvaluator)
    ev._h, ev._m, ev.d, ev.device = ctypes.c_void_p(1), None, 13, "cpu"
    ev.L = types.SimpleNamespace(dq_match_create=create, dq_match_destroy=lambda m: gone.append(("match", m.value)),
                                 dq_wide_uf_destroy=lambda h: gone.append(("handle", h.value)))
    assert ev._referee().value == 0x1234 and ev._referee().value == 0x1234 and made == [13]       # created once, at the first refereed call
    ev.close()
    ev.close()
    assert gone == [("match", 0x1234), ("handle", 1)] and ev._m is None and ev._h is None


class _FakeEvaluator:
    """A WideEvaluator on CPU tensors: hidden = the low bits of the lattice id; the refereed verdict calls a volume alive when its residual's first cell is
    not 3 and flags it when that cell is 2; the unrefereed one takes no keyword and sets alive := success."""

    def __init__(self, d, window, chunk, model="DP"):
        self.d, self.error_model, self.window, self.chunk, self.device = d, model, window, chunk, "cpu"
        self.verdicts = []

    def run_into(self, m, T, commit, lattice_id, seed, p_phys, p_meas, hidden, trivial, frame, weight=None, n_defects=None, rounds=None, syndromes=None):
        import torch
        ids = torch.arange(lattice_id, lattice_id + m)
        hidden.zero_()
        frame.zero_()
        hidden.reshape(m, -1)[:, 0] = (ids & 3).to(torch.uint8)
        frame.reshape(m, -1)[:, 0] = ((ids >> 2) & 1).to(torch.uint8)
        trivial.zero_()

    def verdict_into(self, hidden, frame, m, out, **kw):
        import torch
        self.verdicts.append((m, frame is not None, sorted(kw)))
        res = hidden.reshape(m, -1)[:, 0] ^ (frame.reshape(m, -1)[:, 0] if frame is not None else 0)
        ok = res == 0
        alive = (res != 3) if kw else ok
        out.copy_(ok.to(torch.uint8) * 8 + alive.to(torch.uint8) * 16)
        if kw:
            assert kw["referee"] == "matching"
            kw["inexact"][:m] = (res == 2).to(torch.uint8)

    def count_into(self, verdict, trivial, status, n_corr, m, first, block, counters):
        for i in range(m):
            b = (first + i) // block
            counters[b, 0] += 1
            counters[b, 3] += (int(verdict[i]) >> 3) & 1
            counters[b, 4] += (int(verdict[i]) >> 4) & 1


def test_memory_experiment_wide_counts_alive_and_inexact_per_block(dq, monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "device", lambda dev: contextlib.nullcontext())
    monkeypatch.setattr(torch.cuda, "current_stream", lambda dev=None: types.SimpleNamespace(synchronize=lambda: None))
    DW = dq.decoder_wide
    ids = np.arange(40, 64)
    res, res0 = (ids & 3) ^ ((ids >> 2) & 1), ids & 3
    ev = _FakeEvaluator(9, 18, 7)
    r = DW.memory_experiment_wide((9, "DP"), 24, 40, p_phys=0.02, seed=(3, 4), env_id_base=40, evaluator=ev, no_decoder=True, referee="matching")
    assert ev.verdicts == [(m, f, ["inexact", "referee"]) for m in (7, 7, 7, 3) for f in (True, False)]
    assert r.counters["success"] == int((res == 0).sum()) and r.counters["alive"] == int((res != 3).sum()) and r.inexact == int((res == 2).sum())
    assert r.no_decoder.counters["alive"] == int((res0 != 3).sum()) and r.no_decoder.inexact == int((res0 == 2).sum())
    assert r.summary()["inexact"] == r.inexact > 0 and r.summary()["no_decoder"]["inexact"] == r.no_decoder.inexact > 0
    # the default: the calls of before, argument for argument, and nothing flagged
    ev = _FakeEvaluator(9, 18, 7)
    plain = DW.memory_experiment_wide((9, "DP"), 24, 40, p_phys=0.02, seed=(3, 4), env_id_base=40, evaluator=ev, no_decoder=True)
    assert all(kw == [] for _, _, kw in ev.verdicts) and plain.inexact == 0 and plain.no_decoder.inexact == 0
    assert plain.counters["alive"] == plain.counters["success"] == r.counters["success"]
    # no correction at d >= 13: launches of at most UNCORRECTED_REFEREE_SLICE volumes, the same counts
    assert (DW.UNCORRECTED_REFEREE_D, DW.UNCORRECTED_REFEREE_SLICE) == (13, 2048)
    monkeypatch.setattr(DW, "UNCORRECTED_REFEREE_SLICE", 3)
    ev = _FakeEvaluator(13, 26, 7)
    sliced = DW.memory_experiment_wide((13, "DP"), 24, 40, p_phys=0.02, seed=(3, 4), env_id_base=40, evaluator=ev, no_decoder=True, referee="matching")
    assert [(m, f) for m, f, _ in ev.verdicts] == [x for m in (7, 7, 7, 3) for x in [(m, True)] + [(k, False) for k in ((3, 3, 1) if m == 7 else (3,))]]
    assert sliced.no_decoder.counters == r.no_decoder.counters and sliced.no_decoder.inexact == r.no_decoder.inexact and sliced.counters == r.counters
    monkeypatch.undo()
    monkeypatch.setattr(torch.cuda, "device", lambda dev: contextlib.nullcontext())
    monkeypatch.setattr(torch.cuda, "current_stream", lambda dev=None: types.SimpleNamespace(synchronize=lambda: None))
    # rates: one block per rate, chunks that straddle the blocks
    ev = _FakeEvaluator(9, 18, 5)
    out = DW.memory_experiment_wide((9, "DP"), 12, 40, rates=[0.01, 0.03], seed=(3, 4), env_id_base=40, evaluator=ev, referee="matching")
    for k, rate in enumerate((0.01, 0.03)):
        part = res[12 * k:12 * k + 12]
        assert out[rate].counters["alive"] == int((part != 3).sum()) and out[rate].inexact == int((part == 2).sum()), rate


# ---- 5. the input conditions of the GPU cases -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,model", V.SPARSE_CASES)
def test_sparse_cases_hold_every_kind_of_volume(d, model):
    hidden, frame = V.sparse_case(d, model)
    assert hidden.shape == frame.shape == (V.SPARSE_N, d, d) and V.SPARSE_N % 64 == 1           # (a ragged last chunk at any chunk of whole waves)
    a, b = V.SPARSE_N // 3, 2 * (V.SPARSE_N // 3)
    assert not frame[:a].any() and frame[a:b].any() and all(1 <= int((frame[i] != hidden[i]).sum()) <= 3 for i in range(b, V.SPARSE_N))
    k = V.kinds(V.sparse_expected(d, model)["byte"])
    assert min(k.values()) >= 1, k
    x, z = V.planes(hidden)
    assert 0.012 < x.mean() < 0.028 and 0.012 < z.mean() < 0.028


def test_the_logical_strings_are_in_the_code_space_with_their_class():
    for d in (3, 9, 15):
        R = V.restatement(d, "DP")
        lx, lz = V.logical_planes(d)
        none = np.zeros_like(lx)
        got = R.verdict(np.stack([V.codes(lx, none), V.codes(none, lz), V.codes(lx, lz)]).reshape(3, d, d))["byte"]
        assert [_fields(b) for b in got] == [(True, c, False, False, 0) for c in (1, 2, 3)]


def test_pool_case_holds_clusters_beyond_the_lds_table():
    c = V.POOL_CASE
    hidden, want = V.dense_case("pool")
    assert (c["d"], c["error_model"], len(hidden), c["density"]) == (9, "DP", 256, 0.12)
    largest = [max(V.cluster_sizes(9, typ, want["bits"][comp][i]), default=0) for comp, typ in ((0, 3), (1, 1)) for i in range(len(hidden))]
    assert sum(15 <= s <= 20 for s in largest) >= 20                   # solved in a scratch-pool slot, exactly
    assert sum(s <= 14 for s in largest) >= 20                         # and the LDS table beside it
    # the array form of the cluster rule is ComponentGraph.clusters
    for comp, typ in ((0, 3), (1, 1)):
        g = matching_referee.ComponentGraph(9, typ)
        for i in range(3):
            words = want["bits"][comp][i]
            assert V.cluster_sizes(9, typ, words) == [len(cl) for cl in g.clusters(V.listed_defects(9, typ, words))]


def test_fallback_case_holds_flagged_and_unflagged_volumes():
    c = V.FALLBACK_CASE
    hidden, want = V.dense_case("fallback")
    assert (c["d"], c["error_model"], len(hidden), c["density"]) == (15, "DP", 64, 0.06)
    assert int(want["inexact"].sum()) >= 10 and int((want["inexact"] == 0).sum()) >= 10
    assert np.array_equal(want["inexact"] != 0, (want["flags"] != 0).any(axis=1))
    both = np.bitwise_or.reduce(want["flags"].reshape(-1))
    assert both & c_oracle.CWideMatch.CLUSTER_FALLBACK and both & c_oracle.CWideMatch.LIST_FALLBACK      # both fallbacks fire
