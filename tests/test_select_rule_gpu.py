"""The action-selection rule on the device, every selecting kernel against its one numpy statement (decoder_wide.guided_actions_wide with
guide_share = 0), on the rows random Q values almost never produce: exact ties and masked-out maxima at the boundaries of
each kernel's lane groups (16 lanes per row in dq_policy_select, a whole wavefront elsewhere) and of the 64-bit legal words, legal sets of one
member, sets that live in the last word only, empty sets, rows that are -inf on every legal action and rows of one value.  Q values are multiples
of 1/8, so equal means equal bits.  Expected values never come from another kernel.  Rows holding NaN are not covered: the rule leaves their
index undefined (csrc/common.h)."""
import ctypes
from importlib import import_module

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = (1234, 5678)
N = 64
# What a greedy selection over the legal set (masked_greedy, no exploration) yields for an EMPTY legal set: the scan's "no candidate" index, on
# both entry points (read off the kernels as they stood before the rule moved into one place).  An exploring lattice with an empty set yields -1.
NO_CANDIDATE = 0x7FFFFFFF


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return torch


def tie_pairs(A):
    """Index pairs for equal maxima: one lane's successive strides (16 lanes: 5, 21; 64 lanes: 5, 69), neighbouring lanes across a 16-lane row
    boundary (15, 16), and every kind of word boundary (63, 64; 127, 128; into and inside the last word)."""
    last = 64 * ((A - 1) // 64)
    pairs = [(5, 21), (5, 69), (15, 16), (63, 64), (127, 128), (last - 1, last), (last, A - 1), (0, A - 1)]
    return [(i, j) for i, j in dict.fromkeys(pairs) if 0 <= i < j < A]


def to_words(legal):
    """bool [n, A] -> the legal sets as int64 words [n, ceil(A / 64)] (bit a of the set = action a)."""
    n, A = legal.shape
    LW = (A + 63) // 64
    padded = np.zeros((n, 64 * LW), dtype=np.uint64)
    padded[:, :A] = legal
    shifts = np.arange(64, dtype=np.uint64)
    return (padded.reshape(n, LW, 64) << shifts).sum(axis=2, dtype=np.uint64).view(np.int64)


def from_words(words, A):
    w = np.ascontiguousarray(words).view(np.uint64)
    a = np.arange(A)
    return ((w[:, a >> 6] >> (a & 63).astype(np.uint64)) & np.uint64(1)).astype(bool)


def adversarial_q(legal, seed):
    """float32 [n, A] of multiples of 1/8 for the legal sets `legal` (bool [n, A]): background values in [-2, 0] (ties among them abound), and row by
    row, cycling: equal maxima at each pair of tie_pairs; the same with a larger value on an illegal action; the same with the pair's lower index
    only reachable unmasked; -inf on every legal action; one value in the whole row."""
    rng = np.random.RandomState(seed)
    n, A = legal.shape
    q = (rng.randint(-16, 1, size=(n, A)) / 8.0).astype(np.float32)
    pairs = tie_pairs(A)
    recipes = [("tie", p) for p in pairs] + [("tie_illegal_top", p) for p in pairs] + [("legal_minus_inf", None), ("flat", None)]
    for i in range(n):
        kind, pair = recipes[i % len(recipes)]
        ill = np.flatnonzero(~legal[i])
        if kind == "flat":
            q[i, :] = 0.375
        elif kind == "legal_minus_inf":
            q[i, legal[i]] = -np.inf
        else:
            q[i, pair[0]] = q[i, pair[1]] = 1.0
            if kind == "tie_illegal_top" and len(ill):
                q[i, ill[rng.randint(len(ill))]] = 2.0                        # the global maximum on an illegal action
    return q


def hand_made_legal(A, seed):
    """bool [N, A]: random sets of every density; then, row by row from the end: the empty set (twice), one member (first, last, the last word's
    first, a random one), members in the last word only, the full set.  The first 2 len(tie_pairs) rows are arranged for adversarial_q's recipes: the
    pair legal; in every third row the pair's lower index illegal (the masked answer is then the higher one)."""
    rng = np.random.RandomState(seed)
    legal = rng.rand(N, A) < rng.rand(N, 1)
    pairs = tie_pairs(A)
    assert 2 * len(pairs) <= N - 8                                            # the arranged rows at the front and those at the end do not overlap
    for i in range(2 * len(pairs)):
        lo, hi = pairs[i % len(pairs)]
        legal[i, hi] = True
        legal[i, lo] = i % 3 != 0
    last = 64 * ((A - 1) // 64)
    legal[N - 1] = legal[N - 2] = False
    for row, member in ((N - 3, 0), (N - 4, A - 1), (N - 5, last), (N - 6, int(rng.randint(A)))):
        legal[row] = False
        legal[row, member] = True
    legal[N - 7] = False
    legal[N - 7, last:] = rng.rand(A - last) < 0.5
    legal[N - 7, A - 1] = True
    legal[N - 8] = True
    return legal


def rule(dq, q, legal, eps, masked, t, base=0):
    """The numpy rule's actions for legal sets bool [n, A], empty sets included: an exploring lattice's -1 is the numpy rule's own.  Only the first
    maximum over an empty legal set (masked, eps = 0, so that every such row is known to take that branch) is not: there the numpy rule raises, the
    kernels write NO_CANDIDATE, and the set is filled for the call."""
    empty = ~legal.any(axis=1)
    no_candidate = bool(masked and q is not None and eps < 1.0 and empty.any())
    sets = legal
    if no_candidate:
        assert eps == 0.0
        sets = legal.copy()
        sets[empty] = True
    teacher = np.zeros(len(legal), dtype=np.int32)
    want, guided = dq.guided_actions_wide(q, to_words(sets), teacher, eps, 0.0, masked, SEED, base, t)
    assert not guided.any()
    if no_candidate:
        want[empty] = NO_CANDIDATE
    return want


def raw_select(torch, A, LW, q, legal, eps, masked, t, wide, base=0):
    """dq_policy_select / dq_policy_select_wide on hand-made legal words; no environment handle."""
    L = import_module("deepq-decoding_amd._lib")
    words = to_words(legal)
    if words.shape[1] < LW:
        words = np.concatenate([words, np.zeros((len(words), LW - words.shape[1]), dtype=np.int64)], axis=1)
    dev = torch.device("cuda")
    w = torch.from_numpy(np.ascontiguousarray(words)).to(dev)
    qd = None if q is None else torch.from_numpy(q).to(dev).contiguous()
    out = torch.full((len(legal),), -7, dtype=torch.int32, device=dev)
    seed = (ctypes.c_uint32 * 2)(*SEED)
    st = L.current_stream(dev)
    if wide:
        L.check(L.lib().dq_policy_select_wide(L.ptr(qd), L.ptr(w), len(legal), A, LW, float(eps), int(masked), seed, base, int(t), L.ptr(out), st))
    else:
        L.check(L.lib().dq_policy_select(L.ptr(qd), L.ptr(w), len(legal), A, float(eps), int(masked), seed, base, int(t), L.ptr(out), st))
    return out.cpu().numpy()


RAW = [("narrow", 26, 2), ("narrow", 76, 2), ("narrow", 128, 2), ("wide", 76, 2), ("wide", 244, 4), ("wide", 676, 11)]


@pytest.mark.parametrize("kind,A,LW", RAW, ids=[f"{k}_{a}" for k, a, _ in RAW])
def test_raw_entry_points_on_hand_made_legal_words(dq, torch_mod, kind, A, LW):
    legal = hand_made_legal(A, seed=A)
    q = adversarial_q(legal, seed=A + 1)
    wide = kind == "wide"
    seen = set()
    for masked in (False, True):
        for t in (0, 1, 7, (1 << 33) + 5):
            cases = [(None, 1.0), (q, 1.0), (q, 0.0)]
            for qq, eps in cases:
                got = raw_select(torch_mod, A, LW, qq, legal, eps, masked, t, wide)
                want = rule(dq, qq, legal, eps, masked, t)
                assert np.array_equal(got, want), (kind, A, masked, t, eps, np.flatnonzero(got != want)[:8], got[got != want][:8], want[got != want][:8])
                seen.update(np.unique(got).tolist())
        # a mixed step on the non-empty sets: some lattices explore, the others take their first maximum
        some = legal.any(axis=1)
        got = raw_select(torch_mod, A, LW, q[some], legal[some], 0.5, masked, 3, wide, base=11)
        want = rule(dq, q[some], legal[some], 0.5, masked, 3, base=11)
        assert np.array_equal(got, want), (kind, A, masked, np.flatnonzero(got != want)[:8])
    assert -1 in seen and NO_CANDIDATE in seen                                # the two answers for an empty set were both exercised
    # the greedy answers are np.argmax's, stated without the rule's code: first maximum, over the legal set when masked
    rows = legal.any(axis=1)
    over_legal = np.where(legal, q, -np.inf)
    first = np.where(np.isneginf(over_legal.max(axis=1)), legal.argmax(axis=1), over_legal.argmax(axis=1))   # all -inf: the lowest legal index
    got = raw_select(torch_mod, A, LW, q, legal, 0.0, True, 0, wide)
    assert np.array_equal(got[rows], first[rows])
    got = raw_select(torch_mod, A, LW, q, legal, 0.0, False, 0, wide)
    assert np.array_equal(got, q.argmax(axis=1))


def test_wide_on_two_words_is_the_narrow_selection(dq, torch_mod):
    legal = hand_made_legal(76, seed=76)
    q = adversarial_q(legal, seed=77)
    for masked in (False, True):
        for qq, eps in ((None, 1.0), (q, 0.0), (q, 1.0)):
            for t in (0, 5):
                a = raw_select(torch_mod, 76, 2, qq, legal, eps, masked, t, wide=False)
                b = raw_select(torch_mod, 76, 2, qq, legal, eps, masked, t, wide=True)
                assert np.array_equal(a, b), (masked, eps, t)


FUSED = {
    "narrow_d3": dict(d=3, error_model="DP", use_Y=False, volume_depth=3),
    "narrow_d5": dict(d=5, error_model="DP", use_Y=True, volume_depth=5),     # 76 actions: both legal words in use
    "wide_d9": dict(d=9, error_model="DP", use_Y=False, volume_depth=3),      # 163 actions, LW = 3
}


@pytest.mark.parametrize("name", sorted(FUSED))
def test_fused_forms_on_the_environments_own_legal_words(dq, torch_mod, name):
    """select_actions, guided_select / guided_select_wide without a teacher's share, and act_step: the rule's actions on adversarial Q rows built for the
    lattices' own legal sets after a few uniform steps, masked and unmasked."""
    torch = torch_mod
    cfg = FUSED[name]
    wide = name.startswith("wide")
    kw = dict(backend="wide") if wide else dict(referee="lut")
    env = dq.VectorEnv(n_envs=N, p_phys=0.02, p_meas=0.02, seed=SEED, **cfg, **kw)
    if wide:
        ev = dq.WideEvaluator(env.d, env.error_model, window=env.volume_depth, chunk=N, device=env.device)
    else:
        ev = dq.decoder.Evaluator(cfg["d"], cfg["error_model"], cfg["use_Y"], cfg["volume_depth"], chunk=N, device=env.device)
    try:
        env.reset()
        for t in range(4):
            env.act_step(t, q=None, auto_reset=True)
        t = 4
        for masked in (False, True):
            for eps in (0.0, 0.5):
                legal = from_words(env.legal.cpu().numpy(), env.num_actions)
                assert legal.any(axis=1).all() and len({r.tobytes() for r in legal}) > N // 4          # the sets differ
                q = adversarial_q(legal, seed=100 * t + len(name))
                want = rule(dq, q, legal, eps, masked, t)
                qd = torch.from_numpy(q).to(env.device)
                got = env.select_actions(t, q=qd, eps=eps, masked_greedy=masked).cpu().numpy()
                assert np.array_equal(got, want), (name, "select_actions", masked, eps, np.flatnonzero(got != want)[:8])
                guided = torch.full((N,), 7, dtype=torch.uint8, device=env.device)
                select = env.guided_select_wide if wide else env.guided_select
                got = select(ev, t, q=qd, eps=eps, guide_share=0.0, masked_greedy=masked, out_guided=guided).cpu().numpy()
                assert np.array_equal(got, want) and not guided.any(), (name, "guided_select", masked, eps, np.flatnonzero(got != want)[:8])
                got = env.act_step(t, q=qd, eps=eps, masked_greedy=masked, auto_reset=True).cpu().numpy()      # (moves the lattices on)
                assert np.array_equal(got, want), (name, "act_step", masked, eps, np.flatnonzero(got != want)[:8])
                t += 1
    finally:
        ev.close()
        env.close()


@pytest.mark.parametrize("A", [26, 76, 244])
def test_td_target_reads_q_target_at_the_first_maximum(dq, torch_mod, A):
    """dq_td_target and dq_td_step, B = 8 rows of q_online with equal maxima: y = r + gamma (1 - terminal) q_target[first maximum].  gamma = 1/2 and
    every value a multiple of 1/8: the expression is exact in float32 however it is contracted."""
    torch = torch_mod
    Q = import_module("deepq-decoding_amd.qnet")
    B, gamma = 8, 0.5
    rng = np.random.RandomState(A)
    q_online = adversarial_q(np.ones((B, A), dtype=bool), seed=A + 2)
    q_online[np.isneginf(q_online)] = -4.0                                    # (the all-legal "-inf on every legal action" row: one value instead)
    assert ((q_online == q_online.max(axis=1, keepdims=True)).sum(axis=1) >= 2).all()          # every row's maximum is a tie
    q_target = (rng.permutation(B * A).reshape(B, A) / 8.0).astype(np.float32)         # all different: a wrong index shows
    reward = (rng.randint(0, 9, size=B) / 8.0).astype(np.float32)
    terminal = (np.arange(B) % 4 == 3).astype(np.uint8)
    want = (reward + np.where(terminal != 0, 0.0, gamma * q_target[np.arange(B), q_online.argmax(axis=1)])).astype(np.float32)
    cu = lambda x: torch.from_numpy(x).cuda()
    qo, qt, r, term = cu(q_online), cu(q_target), cu(reward), cu(terminal)
    y = Q.td_target(qo, qt, r, term, gamma).cpu().numpy()
    assert np.array_equal(y, want), (A, y, want)
    q_s0 = cu((rng.randint(-8, 9, size=(B, A)) / 8.0).astype(np.float32))
    action = cu(rng.randint(0, A, size=B).astype(np.int32))
    for delta_clip in (np.inf, 1.0):                                          # dq_td_update and dq_td_step: the same kernel
        y_out = torch.full((B,), -99.0, dtype=torch.float32, device="cuda")
        metrics = torch.zeros(Q.TD_METRICS_FLOATS, dtype=torch.float32, device="cuda")
        Q.td_update(qo, qt, q_s0, r, term, action, gamma, y=y_out, metrics=metrics, delta_clip=delta_clip)
        assert np.array_equal(y_out.cpu().numpy(), want), (A, delta_clip)
