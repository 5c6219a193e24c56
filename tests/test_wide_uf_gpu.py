"""The wide sliding-window union-find decoder on the device (decoder_wide.stream_decode_wide / memory_experiment_wide; csrc/uf_wide.hip and uf_wide_dev.h;
DESIGN.md section 18), bit for bit in frame, weight, defect count and growth rounds: against the narrow kernels where both run, against tests/wide_uf_ref.py
everywhere else.  No stream is left out of any comparison."""
import numpy as np
import pytest

import decode_eval_ref as V
import match_st_ref as M
import wide_uf_ref as W

pytestmark = pytest.mark.gpu

SEED = (1234, 5678)
KEYS = ("frame", "weight", "n_defects", "rounds")


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return torch


_envs, _streams, _refs = {}, {}, {}


def _env(dq, d, model, p=0.01):
    """One narrow environment per lattice for the module (d <= 7): what decoder.stream_decode / memory_experiment / verdict need."""
    key = (d, model, p)
    if key not in _envs:
        _envs[key] = dq.VectorEnv(n_envs=1, p_phys=p, p_meas=p, seed=SEED, d=d, error_model=model, use_Y=False, volume_depth=5)
    return _envs[key]


def _sampled(d, model, T, n, p, base=0):
    """(syndromes, hidden, trivial) of n streams of T rounds, restated on the host once per shape."""
    key = (d, model, T, n, p, base)
    if key not in _streams:
        _streams[key] = V.sample_volumes(d, model, T, n, p, p, SEED, base)
    return _streams[key]


def _reference(d, syn, w, c, key):
    """The restatement's (frame, weight, n_defects, rounds, windows), computed once per key and left unchanged."""
    if key not in _refs:
        _refs[key] = W.decode(d, syn, w, c)[:5]
    return _refs[key]


def _assert_equal(res, want, windows, n, tag):
    for key, w in zip(KEYS, want):
        got = getattr(res, key)
        assert got.dtype == w.dtype and got.shape == w.shape, (tag, key, got.dtype, got.shape)
        bad = np.flatnonzero((got != w).reshape(n, -1).any(axis=1))
        assert bad.size == 0, (tag, key, bad[:8], got[bad[:2]], w[bad[:2]])
    assert res.windows == windows, tag


def _assert_is_reference(dq, d, syn, w, c, key, **kw):
    res = dq.stream_decode_wide(syn, d, window=w, commit=c, to_host=True, **kw)
    want = _reference(d, syn, w, c, key)
    _assert_equal(res, want[:4], want[4], len(syn), key)
    return res


# ---- 1. against the existing kernels -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,n", [(5, 256), (7, 64)])
@pytest.mark.parametrize("w,c", [(10, 5), (16, 8), (16, 16)])
def test_narrow_lattices_equal_the_narrow_kernel(dq, torch_mod, d, n, w, c):
    syn = _sampled(d, "DP", 33, n, 0.011)[0]
    want = dq.decoder.stream_decode(syn, _env(dq, d, "DP"), window=w, commit=c, to_host=True)
    res = dq.stream_decode_wide(syn, d, window=w, commit=c, to_host=True)
    _assert_equal(res, [getattr(want, k) for k in KEYS], want.windows, n, (d, w, c))
    assert (res.n_defects.sum(axis=1) > 0).sum() > n // 2 and res.frame.any() and res.rounds.max() >= 2


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
    want = dq.decoder.stream_decode(syn, _env(dq, d, "DP"), window=2, commit=1, to_host=True)
    res = dq.stream_decode_wide(syn, d, window=2, commit=1, chunk=3000, to_host=True)
    _assert_equal(res, [getattr(want, k) for k in KEYS], 2, n, "d3")
    assert len(np.unique(res.frame.reshape(n, -1), axis=0)) > 50 and res.rounds.max() >= 3 and res.weight.max() >= 4      # (not vacuous)


# ---- 2. windows the narrow kernel cannot run -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,c", [(17, 9), (32, 16)])
def test_d5_windows_beyond_sixteen(dq, torch_mod, w, c):
    syn = _sampled(5, "DP", 70, 64, 0.011)[0]
    res = _assert_is_reference(dq, 5, syn, w, c, (5, 70, w, c))
    assert res.windows == W.n_windows(70, w, c) and res.frame.any()


# ---- 3. word boundaries ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,n,T,p,w,c", [(9, 64, 40, 0.01, 18, 9), (9, 64, 40, 0.01, 2, 1), (9, 64, 40, 0.01, 32, 32), (13, 16, 40, 0.01, 26, 13),
                                         (15, 16, 64, 0.01, 30, 15), (15, 16, 64, 0.01, 32, 1), (15, 8, 32, 0.04, 32, 16)])
def test_wide_lattices_are_the_restatement(dq, torch_mod, d, n, T, p, w, c):
    syn = _sampled(d, "DP", T, n, p)[0]
    res = _assert_is_reference(dq, d, syn, w, c, (d, n, T, p, w, c))
    assert (res.n_defects.sum(axis=1) > 0).all() and res.frame.any()
    if p == 0.04:                                                                # the dense case: hundreds of defects per component, several growth rounds
        assert res.n_defects.max() > 500 and res.weight.max() > 400 and res.rounds.max() >= 4
    if (w, c) in ((2, 1), (32, 1)):                                              # many windows: the growth rounds add up over them
        assert res.windows >= 33 and res.rounds.max() > 100
    # both halves of every word count are in use: qubits and nodes beyond the first 32 / 64 / ... carry corrections and defects
    flat = res.frame.reshape(n, -1)
    for lo in range(0, d * d, 64):
        assert flat[:, lo:lo + 64].any(), (d, lo)


def _hand_cases(d):
    """Streams of 3 d rounds under (2 d, d) as node bits [K, T, n] per component: nothing; a lone DEFECT (a syndrome bit that stays set from round t on) on nodes
    0, n - 1, 32 and 64 in the first and the last round of the first window; a same-site defect pair straddling the commit line (one round's syndrome bit)."""
    n, w, c = (d * d - 1) // 2, min(2 * d, 32), d
    T = 3 * d
    nodes = [u for u in (0, n - 1, 32, 64) if u < n]
    cases = [np.zeros((T, n), dtype=np.uint8)]
    for u in nodes:
        for t in (0, w - 1):
            b = np.zeros((T, n), dtype=np.uint8)
            b[t:, u] = 1
            cases.append(b)
        b = np.zeros((T, n), dtype=np.uint8)
        b[c - 1, u] = 1                                                          # defects (u, c - 1) and (u, c)
        cases.append(b)
    bits = np.stack(cases)
    return np.concatenate([W.node_syndromes(d, 0, bits), W.node_syndromes(d, 1, bits)]), w, c, len(bits), len(nodes)


@pytest.mark.parametrize("d", [9, 15])
def test_hand_cases(dq, torch_mod, d):
    syn, w, c, K, n_nodes = _hand_cases(d)
    res = _assert_is_reference(dq, d, syn, w, c, ("hand", d))
    assert n_nodes == (3 if d == 9 else 4)                                       # (node 64 exists from d = 13 on)
    for comp in range(2):
        o = comp * K
        assert not res.frame[o].any() and not res.weight[o].any() and not res.rounds[o].any()      # no defect: nothing happens
        assert res.n_defects[o:o + K, 1 - comp].sum() == 0 and res.weight[o:o + K, 1 - comp].sum() == 0
        for k in range(n_nodes):
            pair = o + 3 + 3 * k                                                 # the straddling pair: one committed time edge, no qubit
            assert res.weight[pair, comp] == 1 and res.n_defects[pair, comp] == 2 and not res.frame[pair].any(), (d, comp, k)
            for lone in (o + 1 + 3 * k, o + 2 + 3 * k):
                assert res.n_defects[lone, comp] == 1 and res.weight[lone, comp] >= 1, (d, comp, k)


# ---- 4. independence ----------------------------------------------------------------------------------------------------------------------------------------
def test_results_depend_on_the_stream_alone(dq, torch_mod):
    d, n, T, w, c = 9, 64, 40, 18, 9
    syn = _sampled(d, "DP", T, n, 0.01)[0]
    want = _reference(d, syn, w, c, (d, n, T, 0.01, w, c))
    perm = np.random.default_rng(3).permutation(n)
    res = dq.stream_decode_wide(syn[perm], d, window=w, commit=c, to_host=True)
    _assert_equal(res, [x[perm] for x in want[:4]], want[4], n, "permuted")
    narrow_syn = _sampled(5, "DP", 33, 256, 0.011)[0]
    env = _env(dq, 5, "DP")
    before = dq.decoder.stream_decode(narrow_syn, env, window=10, commit=5, to_host=True)
    ev = dq.WideEvaluator(d, "DP", w, chunk=n)
    try:
        for chunk in (1, 7, n):
            res = dq.stream_decode_wide(syn, d, window=w, commit=c, chunk=chunk, to_host=True)
            _assert_equal(res, want[:4], want[4], n, ("chunk", chunk))
        for rep in range(3):                                                     # repeated calls on one handle, the batch shrinking
            m = n >> rep
            res = dq.stream_decode_wide(syn[:m], d, window=w, commit=c, evaluator=ev, to_host=True)
            _assert_equal(res, [x[:m] for x in want[:4]], want[4], m, ("repeat", rep))
    finally:
        ev.close()
    after = dq.decoder.stream_decode(narrow_syn, env, window=10, commit=5, to_host=True)
    for k in KEYS:
        assert np.array_equal(getattr(before, k), getattr(after, k)), k


def test_a_handle_serves_growing_batches_of_per_stream_rates(dq, torch_mod):
    """The handle's rate table holds max_streams pairs from the start: per-stream rates at a small n, then at n = max_streams, on one handle."""
    torch = torch_mod
    d, T, big = 9, 12, 96
    ev = dq.WideEvaluator(d, "DP", 18, chunk=big)
    try:
        for n in (4, big, 7):
            ph, pm = np.linspace(0.004, 0.03, n), np.linspace(0.03, 0.0, n)
            want_syn, want_hid, want_triv = V.sample_volumes(d, "DP", T, n, ph, pm, SEED, 50)
            hid, frame = (torch.zeros((n, d, d), dtype=torch.uint8, device="cuda") for _ in range(2))
            triv = torch.zeros(n, dtype=torch.uint8, device="cuda")
            syn = torch.zeros((n, T, d + 1, d + 1), dtype=torch.uint8, device="cuda")
            ev.run_into(n, T, 9, 50, SEED, ph, pm, hid, triv, frame, syndromes=syn)
            torch.cuda.synchronize()
            assert np.array_equal(syn.cpu().numpy(), want_syn) and np.array_equal(hid.cpu().numpy(), want_hid), n
            assert np.array_equal(triv.cpu().numpy(), want_triv), n
        # through the public entry point: rates=[...] with few runs, then with many, on the same evaluator
        for runs in (4, big // 2):
            both = dq.memory_experiment_wide((d, "DP"), runs, T, rates=[0.004, 0.02], seed=SEED, evaluator=ev)
            for k, r in enumerate((0.004, 0.02)):
                one = dq.memory_experiment_wide((d, "DP"), runs, T, p_phys=r, seed=SEED, env_id_base=runs * k)
                assert both[r].counters == one.counters, (runs, r)
    finally:
        ev.close()


def test_a_small_handle_does_not_lower_a_large_ones_lds(dq, torch_mod):
    """The kernels' dynamic-LDS limit is the largest shape's whatever handles exist: a d = 15 / window 32 handle decodes after a d = 3 one was created."""
    d, n, T, p, w, c = 15, 8, 32, 0.04, 32, 16
    syn = _sampled(d, "DP", T, n, p)[0]
    want = _reference(d, syn, w, c, (d, n, T, p, w, c))
    large = dq.WideEvaluator(d, "DP", w, chunk=n)
    small = dq.WideEvaluator(3, "DP", 2, chunk=n)
    try:
        tiny = dq.stream_decode_wide(np.zeros((n, 4, 4, 4), dtype=np.uint8), 3, window=2, commit=1, evaluator=small, to_host=True)
        assert not tiny.frame.any()
        res = dq.stream_decode_wide(syn, d, window=w, commit=c, evaluator=large, to_host=True)
        _assert_equal(res, want[:4], want[4], n, "large after small")
    finally:
        small.close()
        large.close()


# ---- 5. sampler and verdict ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,T,n", [(9, 12, 48), (15, 6, 24)])
@pytest.mark.parametrize("model", ["X", "DP", "IIDXZ"])
def test_fused_run_samples_the_restated_rounds_and_decodes_them(dq, torch_mod, d, T, n, model):
    torch = torch_mod
    base = 4_294_967_290                                                         # the lattice ids wrap
    w, c = min(2 * d, 32), d
    ev = dq.WideEvaluator(d, model, w, chunk=n)
    try:
        for each in (False, True):
            ph = np.linspace(0.004, 0.03, n) if each else 0.02
            pm = ph[::-1].copy() if each else 0.01
            want_syn, want_hid, want_triv = V.sample_volumes(d, model, T, n, ph, pm, SEED, base)
            for with_syn in (True, False):
                hid = torch.zeros((n, d, d), dtype=torch.uint8, device="cuda")
                frame = torch.full((n, d, d), 9, dtype=torch.uint8, device="cuda")
                triv = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
                outs = [torch.zeros((n, 2), dtype=torch.int32, device="cuda") for _ in range(3)]
                syn = torch.full((n, T, d + 1, d + 1), 9, dtype=torch.uint8, device="cuda") if with_syn else None
                ev.run_into(n, T, c, base, SEED, ph, pm, hid, triv, frame, *outs, syndromes=syn)
                torch.cuda.synchronize()
                assert np.array_equal(hid.cpu().numpy(), want_hid) and np.array_equal(triv.cpu().numpy(), want_triv), (model, each, with_syn)
                if with_syn:
                    assert np.array_equal(syn.cpu().numpy(), want_syn), (model, each)
                dec = dq.stream_decode_wide(want_syn, d, window=w, commit=c, evaluator=ev, to_host=True)
                for key, got in zip(KEYS, [frame] + outs):
                    assert np.array_equal(got.cpu().numpy(), getattr(dec, key)), (model, each, with_syn, key)
            # the verdict of the residual, with and without the frame
            verd = torch.zeros(n, dtype=torch.uint8, device="cuda")
            for f in (frame, None):
                ev.verdict_into(hid, f, n, verd)
                torch.cuda.synchronize()
                want = V.verdict(d, want_hid, None if f is None else f.cpu().numpy(), W.classify_none)
                assert np.array_equal(verd.cpu().numpy(), want), (model, each, f is None)
        assert want_hid.any() and want_syn.any()
    finally:
        ev.close()


def test_verdict_bits_at_d5_are_the_narrow_verdicts(dq, torch_mod):
    torch = torch_mod
    d, n = 5, 512
    _, hid, _ = _sampled(d, "DP", 8, n, 0.03)
    frame = _sampled(d, "DP", 3, n, 0.03, base=7000)[1]                          # any frames: other lattices' errors
    ev = dq.WideEvaluator(d, "DP", 10, chunk=n)
    try:
        for f in (frame, None):
            want, _ = dq.decoder.verdict(hid, f, _env(dq, d, "DP"), to_host=True)
            out = torch.zeros(n, dtype=torch.uint8, device="cuda")
            ev.verdict_into(torch.from_numpy(hid).cuda(), None if f is None else torch.from_numpy(f).cuda(), n, out)
            got = out.cpu().numpy()
            mask = V.IN_CODESPACE | V.SUCCESS | (3 << V.CLASS_SHIFT)
            assert np.array_equal(got & mask, want & mask) and ((got & V.SUCCESS) != 0).any() and ((got & V.SUCCESS) == 0).any()
            assert np.array_equal((got & V.ALIVE) != 0, (got & V.SUCCESS) != 0) and not (got >> V.DECODED_SHIFT).any()
    finally:
        ev.close()


# ---- 6. end to end ------------------------------------------------------------------------------------------------------------------------------------------
def test_memory_experiment_wide_counters(dq, torch_mod):
    D = dq.decoder
    d, n, T, p, w, c = 9, 96, 40, 0.01, 18, 9
    syn, hid, triv = _sampled(d, "DP", T, n, p)
    frame = _reference(d, syn[:64], w, c, (d, 64, T, p, w, c))[0]
    frame = np.concatenate([frame, W.decode(d, syn[64:], w, c)[0]])
    got, streams = dq.memory_experiment_wide((d, "DP"), n, T, p_phys=p, seed=SEED, chunk=40, no_decoder=True, return_streams=True)
    assert np.array_equal(streams["syndromes"].cpu().numpy(), syn) and np.array_equal(streams["frame"].cpu().numpy(), frame)
    want = D.counters_from_arrays(V.verdict(d, hid, frame, W.classify_none), triv, np.full(n, D.STATUS_IDENTITY), (frame != 0).reshape(n, -1).sum(axis=1))
    want0 = D.counters_from_arrays(V.verdict(d, hid, None, W.classify_none), triv)
    assert [got.counters[k] for k in D.COUNTER_NAMES] == want and [got.no_decoder.counters[k] for k in D.COUNTER_NAMES] == want0
    assert got.counters["alive"] == got.counters["success"] and got.death_rate == got.failure_rate
    # an environment of the wide backend supplies d, the model, the rates and the seed
    env = dq.VectorEnv(n_envs=1, p_phys=p, p_meas=p, seed=SEED, d=d, error_model="DP", use_Y=False, volume_depth=5)
    again = dq.memory_experiment_wide(env, n, T)
    assert again.counters == got.counters
    # rates=[...] is one call per rate on the same lattice ids
    rates = [0.004, 0.012]
    both = dq.memory_experiment_wide((d, "DP"), 64, T, rates=rates, seed=SEED, env_id_base=500, chunk=48, no_decoder=True)
    for k, r in enumerate(rates):
        one = dq.memory_experiment_wide((d, "DP"), 64, T, p_phys=r, seed=SEED, env_id_base=500 + 64 * k, no_decoder=True)
        assert both[r].counters == one.counters and both[r].no_decoder.counters == one.no_decoder.counters and both[r].p_phys == r
    # p = 0: nothing to decode, nothing fails
    zero = dq.memory_experiment_wide((d, "DP"), 64, T, p_phys=0.0, seed=SEED, no_decoder=True)
    assert zero.counters["success"] == 64 and zero.counters["trivial"] == 64 and zero.counters["corrections"] == 0 and zero.failure_rate == 0.0


def test_decoded_streams_fail_less_often_than_undecoded_ones(dq, torch_mod):
    got = dq.memory_experiment_wide((9, "DP"), 2048, 100, p_phys=0.003, seed=SEED, no_decoder=True)
    assert got.counters["volumes"] == 2048 and got.failure_rate < 0.15 and got.no_decoder.failure_rate > 0.9
    assert got.failure_interval[1] < got.no_decoder.failure_interval[0]
