"""Sliding-window union-find decoding of syndrome streams on the device (decoder.stream_decode / memory_experiment; csrc/uf_stream.hip and uf_dev.h's
uf_component_commit) against tests/stream_uf_ref.py, bit for bit: the algorithm is a function of the stream alone, so frames, weights,
defect counts and growth rounds are compared as they are."""
import numpy as np
import pytest

import decode_eval_ref as V
import match_st_ref as M
import shipped
import stream_uf_ref as S
from oracle import referee

pytestmark = pytest.mark.gpu

SEED = (1234, 5678)
UF = "union_find"
WINDOWS = [(1, 1), (2, 1), (10, 5), (16, 15), (16, 16), (7, 7)]
KEYS = ("frame", "weight", "n_defects", "rounds")


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return torch


_envs = {}


def _env(dq, d, model, depth=5, p=0.01, ref=None):
    """One environment per lattice for the module: it supplies the lattice tables (and the referee); its volume_depth is not consulted by the stream calls."""
    key = (d, model, depth, p, ref)
    if key not in _envs:
        _envs[key] = dq.VectorEnv(n_envs=1, p_phys=p, p_meas=p, seed=SEED, referee=ref, d=d, error_model=model, use_Y=False, volume_depth=depth)
    return _envs[key]


_streams = {}


def _sampled(d, model, T, n, p, base=0):
    """(syndromes, hidden, trivial) of n streams of T rounds, restated on the host once per shape."""
    key = (d, model, T, n, p, base)
    if key not in _streams:
        _streams[key] = V.sample_volumes(d, model, T, n, p, p, SEED, base)
    return _streams[key]


def _assert_is_reference(d, syn, w, c, res, tag):
    frame, weight, ndef, rounds, windows, _ = S.decode(d, syn, w, c)
    for key, want in (("frame", frame), ("weight", weight), ("n_defects", ndef), ("rounds", rounds)):
        got = getattr(res, key)
        assert got.dtype == want.dtype and got.shape == want.shape, (tag, key, got.dtype, got.shape)
        bad = np.flatnonzero((got != want).reshape(len(syn), -1).any(axis=1))
        assert bad.size == 0, (tag, key, bad[:8], got[bad[:2]], want[bad[:2]])
    assert res.windows == windows, tag
    return frame, weight, ndef, rounds


# ---- 1. exhaustive ---------------------------------------------------------------------------------------------------------------------------
def test_every_pattern_of_d3_three_rounds_window_two(dq, torch_mod):
    d, T, bits = 3, 3, 12
    n = 1 << bits
    idx = np.arange(n, dtype=np.int64)
    rev = np.zeros_like(idx)
    for b in range(bits):
        rev |= ((idx >> b) & 1) << (bits - 1 - b)
    syn = np.zeros((n, T, d + 1, d + 1), dtype=np.uint8)
    for comp, pat in ((0, idx), (1, rev)):                                       # every pattern of both components appears
        cells = M.Component(d, comp).cells
        assert len(cells) * T == bits
        for t in range(T):
            for j, (a, b) in enumerate(cells):
                syn[:, t, a, b] = (pat >> (t * len(cells) + j)) & 1
    res = dq.decoder.stream_decode(syn, _env(dq, d, "DP"), window=2, commit=1, chunk=3000, to_host=True)
    frame, weight, _, rounds = _assert_is_reference(d, syn, 2, 1, res, "d3")
    assert res.windows == 2 and len(np.unique(frame.reshape(n, -1), axis=0)) > 50 and rounds.max() >= 3 and weight.max() >= 4      # (not vacuous)


# ---- 2. d = 5 depolarising -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,c", WINDOWS)
def test_d5_depolarising_streams_are_the_reference(dq, torch_mod, w, c):
    d, T, n, p = 5, 33, 256, 0.011
    syn = _sampled(d, "DP", T, n, p)[0]
    res = dq.decoder.stream_decode(syn, _env(dq, d, "DP"), window=w, commit=c, to_host=True)
    _, weight, ndef, rounds = _assert_is_reference(d, syn, w, c, res, (w, c))
    print((w, c), dict(windows=res.windows, max_defects=int(ndef.max()), max_weight=int(weight.max()), max_rounds=int(rounds.max())))
    assert (ndef.sum(axis=1) > 0).sum() > n // 2
    if (w, c) == (10, 5):
        assert res.windows == 6 and T - 5 * 5 == 8                               # a ragged final window of 8 rounds


@pytest.mark.parametrize("T", [10, 11, 7])
def test_d5_streams_of_about_one_window(dq, torch_mod, T):
    """T = w (one window), T = w + 1 (a full window and a final one of 6 rounds) and T < w, on prefixes of the same streams."""
    d, w, c = 5, 10, 5
    syn = np.ascontiguousarray(_sampled(d, "DP", 33, 256, 0.011)[0][:, :T])
    res = dq.decoder.stream_decode(syn, _env(dq, d, "DP"), window=w, commit=c, to_host=True)
    _assert_is_reference(d, syn, w, c, res, T)
    assert res.windows == (2 if T == 11 else 1)


# ---- 3. d = 7, dense windows -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,c", [(16, 8), (16, 1)])
def test_d7_dense_windows_are_the_reference(dq, torch_mod, w, c):
    d, T, n, p = 7, 64, 64, 0.02
    syn = _sampled(d, "DP", T, n, p)[0]
    res = dq.decoder.stream_decode(syn, _env(dq, d, "DP"), window=w, commit=c, to_host=True)
    _, weight, ndef, rounds = _assert_is_reference(d, syn, w, c, res, (w, c))
    print((w, c), dict(windows=res.windows, max_defects=int(ndef.max()), max_weight=int(weight.max()), max_rounds=int(rounds.max())))
    assert ndef.min() > 20


# ---- 4. bit-flip noise: component 1 sees measurement faults only ---------------------------------------------------------------------------------------
def test_d5_bit_flip_streams_are_the_reference(dq, torch_mod):
    d, T, n, p = 5, 33, 128, 0.011
    syn, hid, _ = _sampled(d, "X", T, n, p)
    assert not (hid >= 2).any()                                                  # no Z component in the error
    res = dq.decoder.stream_decode(syn, _env(dq, d, "X"), window=10, commit=5, to_host=True)
    _, weight, ndef, _ = _assert_is_reference(d, syn, 10, 5, res, "X")
    assert ndef[:, 1].sum() > 0 and weight[:, 1].sum() > 0


# ---- 5. one window against the existing union-find decode -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 5, 16])
def test_one_window_is_matching_decode_union_find(dq, torch_mod, T):
    d, n, p = 5, 256, 0.02
    D = dq.decoder
    env = _env(dq, d, "DP", depth=T)
    vol, _, _ = D.sample_volumes(env, n, p_phys=p, seed=SEED, to_host=True)
    want = D.matching_decode(vol, env, to_host=True, method=UF)
    assert want.weight.sum() > 0
    for c in sorted({1, (T + 1) // 2, T}):
        got = D.stream_decode(vol, env, window=T, commit=c, to_host=True)
        assert got.windows == 1 and all(np.array_equal(getattr(got, k), getattr(want, k)) for k in KEYS), (T, c)
    if T < 16:                                                                   # a window longer than the stream is one window too
        got = D.stream_decode(vol, _env(dq, d, "DP"), window=16, commit=3, to_host=True)
        assert got.windows == 1 and all(np.array_equal(getattr(got, k), getattr(want, k)) for k in KEYS), T


# ---- 6. batch, chunk, handle ------------------------------------------------------------------------------------------------------------------------
def test_results_depend_on_the_stream_alone_and_the_handle_is_shared(dq, torch_mod):
    D = dq.decoder
    d, T, n, w, c = 5, 33, 256, 10, 5
    env = _env(dq, d, "DP")
    syn = _sampled(d, "DP", T, n, 0.011)[0]
    same = lambda a, b, ks=KEYS: all(np.array_equal(getattr(a, k), getattr(b, k)) for k in ks)
    base = D.stream_decode(syn, env, window=w, commit=c, to_host=True)
    assert np.array_equal(D.stream_decode(syn[3], env, window=w, commit=c, to_host=True).frame[0], base.frame[3])      # one stream without the batch axis
    for chunk in (1, 7, n):
        assert same(base, D.stream_decode(syn, env, window=w, commit=c, chunk=chunk, to_host=True)), chunk
    perm = np.random.default_rng(3).permutation(n)
    shuffled = D.stream_decode(syn[perm], env, window=w, commit=c, chunk=64, to_host=True)
    assert all(np.array_equal(getattr(shuffled, k), getattr(base, k)[perm]) for k in KEYS)
    # one handle: the whole-volume decoders give their own results before and after a stream call
    env10 = _env(dq, d, "DP", depth=10)
    vol = np.ascontiguousarray(syn[:, :10])
    ev = D.Evaluator(d, "DP", False, 10, chunk=n, device=env.device)
    try:
        uf0 = D.matching_decode(vol, env10, to_host=True, evaluator=ev, method=UF)
        mt0 = D.matching_decode(vol, env10, to_host=True, evaluator=ev)
        first = D.stream_decode(syn, env, window=w, commit=c, to_host=True, evaluator=ev)
        assert same(first, base) and same(base, D.stream_decode(syn, env, window=w, commit=c, to_host=True, evaluator=ev))      # a repeated call
        mk = ("frame", "weight", "n_defects", "inexact")
        assert same(uf0, D.matching_decode(vol, env10, to_host=True, evaluator=ev, method=UF), KEYS + ("inexact",))
        assert same(mt0, D.matching_decode(vol, env10, to_host=True, evaluator=ev), mk)
        assert same(uf0, D.matching_decode(vol, env10, to_host=True, method=UF), KEYS) and same(mt0, D.matching_decode(vol, env10, to_host=True), mk)
    finally:
        ev.close()


# ---- 7. the fused run ------------------------------------------------------------------------------------------------------------------------------------
def test_fused_run_samples_the_environments_rounds_and_decodes_them(dq, torch_mod):
    D = dq.decoder
    d, T, n, p, base = 5, 40, 192, 0.011, 77
    env = _env(dq, d, "DP", ref="lut")                                           # (memory_experiment asks the referee for its verdict)
    host = lambda s: {k: v.cpu().numpy() for k, v in s.items()}
    _, got = D.memory_experiment(env, n, T, p_phys=p, seed=SEED, env_id_base=base, chunk=80, return_streams=True)
    got = host(got)
    syn, hid, triv = _sampled(d, "DP", T, n, p, base)
    assert np.array_equal(got["syndromes"], syn) and np.array_equal(got["hidden"], hid) and np.array_equal(got["trivial"], triv)
    dec = D.stream_decode(got["syndromes"], env, to_host=True)                   # the defaults on both sides: window 10, commit 5
    assert np.array_equal(got["frame"], dec.frame) and dec.frame.any()
    # per-stream rates
    ph = np.where(np.arange(n) % 3 == 0, 0.0, np.where(np.arange(n) % 3 == 1, 0.007, 0.02))
    pm = ph[::-1].copy()
    _, each = D.memory_experiment(env, n, T, p_phys=ph, p_meas=pm, seed=SEED, env_id_base=base, return_streams=True)
    each = host(each)
    want = V.sample_volumes(d, "DP", T, n, ph, pm, SEED, base)
    assert all(np.array_equal(each[k], x) for k, x in zip(("syndromes", "hidden", "trivial"), want))
    assert np.array_equal(each["frame"], D.stream_decode(each["syndromes"], env, to_host=True).frame)
    # T = 5: the sampler of a depth-5 environment
    env5 = _env(dq, d, "DP", depth=5, ref="lut")
    _, five = D.memory_experiment(env5, n, 5, p_phys=p, seed=SEED, env_id_base=base, return_streams=True)
    five = host(five)
    vol, hid5, triv5 = D.sample_volumes(env5, n, p_phys=p, seed=SEED, env_id_base=base, to_host=True)
    assert np.array_equal(five["syndromes"], vol) and np.array_equal(five["hidden"], hid5) and np.array_equal(five["trivial"], triv5)
    assert np.array_equal(five["frame"], D.matching_decode(vol, env5, to_host=True, method=UF).frame)      # window 10 >= T: one window
    # the frame is the same without the syndromes buffer
    ev = D.Evaluator(d, "DP", False, 10, chunk=n, device=env.device)
    try:
        t = torch_mod
        hid_d = t.empty((n, d, d), dtype=t.uint8, device=env.device)
        frame_d = t.empty((n, d, d), dtype=t.uint8, device=env.device)
        triv_d = t.empty(n, dtype=t.uint8, device=env.device)
        stats = [t.empty((n, 2), dtype=t.int32, device=env.device) for _ in range(3)]
        with t.cuda.device(env.device):
            ev.stream_run_into(env, n, T, 5, base, SEED, p, p, hid_d, triv_d, frame_d, *stats)
            t.cuda.current_stream(env.device).synchronize()
        assert np.array_equal(frame_d.cpu().numpy(), got["frame"]) and np.array_equal(hid_d.cpu().numpy(), hid)
        for x, k in zip(stats, ("weight", "n_defects", "rounds")):
            assert np.array_equal(x.cpu().numpy(), getattr(dec, k)), k
    finally:
        ev.close()


# ---- 8. the counters of memory_experiment -------------------------------------------------------------------------------------------------------------------
def test_memory_experiment_counters(dq, torch_mod):
    from oracle import c_oracle
    D = dq.decoder
    d, T, n, p = 5, 40, 512, 0.007
    env = _env(dq, d, "DP", p=p, ref="lut")
    timings = {}
    res, streams = D.memory_experiment(env, n, T, seed=SEED, no_decoder=True, chunk=200, return_streams=True, timings=timings)
    hid, frame, triv = (streams[k].cpu().numpy() for k in ("hidden", "frame", "trivial"))
    lx, lz = c_oracle.luts(d)
    classify = V.classify_with(referee.LutReferee(d, "DP", lx, lz))
    want = D.counters_from_arrays(V.verdict(d, hid, frame, classify), triv, np.full(n, D.STATUS_IDENTITY), (frame.reshape(n, -1) != 0).sum(axis=1))
    assert [res.counters[k] for k in D.COUNTER_NAMES] == want and res.inexact == 0 and res.p_phys == p
    want0 = D.counters_from_arrays(V.verdict(d, hid, None, classify), triv)
    assert [res.no_decoder.counters[k] for k in D.COUNTER_NAMES] == want0 and {"run", "verdict"} <= set(timings)
    assert D.memory_experiment(env, n, T, seed=SEED).counters == res.counters     # without the streams, in one chunk
    rates = [0.003, 0.011]
    swept = D.memory_experiment(env, 256, T, rates=rates, seed=SEED, chunk=100)
    assert list(swept) == rates
    for k, r in enumerate(rates):
        one = D.memory_experiment(env, 256, T, p_phys=r, seed=SEED, env_id_base=256 * k)
        assert one.counters == swept[r].counters and swept[r].p_phys == r and swept[r].p_meas == r, r
    clean = D.memory_experiment(env, 256, T, p_phys=0.0, seed=SEED, no_decoder=True)
    assert clean.counters["success"] == 256 and clean.counters["trivial"] == 256 and clean.counters["corrections"] == 0 and clean.failure_rate == 0.0
    assert clean.no_decoder.counters["success"] == 256


# ---- 9. one sanity row ---------------------------------------------------------------------------------------------------------------------------------
def test_decoded_streams_fail_less_often_than_undecoded_ones(dq, torch_mod):
    D = dq.decoder
    env = dq.VectorEnv(n_envs=1, p_phys=0.007, p_meas=0.007, seed=SEED, referee="lut", **shipped.CONFIGS["d5_dp"])
    got = D.memory_experiment(env, 4096, 40, seed=SEED, no_decoder=True)
    print(f"d5_dp p = 0.007, 40 rounds, window 10 / commit 5: failure rate {got.failure_rate:.4f} {got.failure_interval}, no decoder "
          f"{got.no_decoder.failure_rate:.4f} {got.no_decoder.failure_interval}")
    assert got.counters["volumes"] == 4096
    assert got.failure_rate < got.no_decoder.failure_rate and got.failure_interval[1] < got.no_decoder.failure_interval[0]
