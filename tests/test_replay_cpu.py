"""replay.ReplayRing on CPU tensors: the one owner of the replay ring's fields (slot arithmetic, pickled form, copies, the scratch
ring of an evaluation).  Both ring forms construct without a GPU: env.patch_to_obs / obs_to_patch are pure torch."""
import functools
import importlib
import pickle
import types

import numpy as np
import pytest
import torch

D, DEPTH, LAYERS = 5, 5, 2
OBS_SHAPE = (DEPTH + LAYERS, 2 * D + 1, 2 * D + 1)


@pytest.fixture(scope="module")
def mods():
    return importlib.import_module("deepq-decoding_amd.replay"), importlib.import_module("deepq-decoding_amd.env")


def make(mods, T=5, N=3, compact=False):
    replay, env = mods
    stride = env.patch_stride_words(D)
    return replay.ReplayRing(T, N, OBS_SHAPE, functools.partial(env.patch_to_obs, d=D, depth=DEPTH, layers=LAYERS),
                             functools.partial(env.obs_to_patch, d=D, depth=DEPTH, layers=LAYERS, stride=stride), stride if compact else None)


def fill(ring, seed, cur=2, filled=4):
    """Random transitions; the observations are images the environment can produce (decoded from random patch words)."""
    g = torch.Generator().manual_seed(seed)
    words = torch.zeros((ring.T, ring.N, ring.patch_stride or 32), dtype=torch.int32)
    words[..., :D * D] = torch.randint(0, 1 << (4 * DEPTH + LAYERS), (ring.T, ring.N, D * D), generator=g).to(torch.int32)
    if ring.compact:
        ring.store.copy_(words)
    else:
        ring.store.copy_(ring.patch_to_obs(words))
    ring.action.copy_(torch.randint(0, 51, (ring.T, ring.N), generator=g).to(torch.int32))
    ring.reward.copy_(torch.rand((ring.T, ring.N), generator=g))
    ring.terminal.copy_(torch.randint(0, 2, (ring.T, ring.N), generator=g).to(torch.uint8))
    ring.cur, ring.filled = cur, filled
    return ring


def same(a, b):
    return (torch.equal(a.obs[:], b.obs[:]) and torch.equal(a.action, b.action) and torch.equal(a.reward, b.reward)
            and torch.equal(a.terminal, b.terminal) and (a.cur, a.filled, a.T, a.N) == (b.cur, b.filled, b.T, b.N))


def test_slot_arithmetic_wraps(mods):
    ring = make(mods, T=4)
    assert (ring.cur, ring.filled, ring.nb_entries) == (0, 0, 0) and ring.next_slot() == 1 and ring.next_slot(-1) == 3
    seen = []
    for _ in range(6):
        nxt, after = ring.next_slot(), ring.filled_after()
        ring.advance()
        assert (ring.cur, ring.filled) == (nxt, after)
        seen.append((ring.cur, ring.filled))
    assert seen == [(1, 1), (2, 2), (3, 3), (0, 4), (1, 4), (2, 4)]
    ring.cur = 3
    assert ring.next_slot() == 0 and ring.next_slot(2) == 1 and ring.next_slot(-1) == 2 and ring.filled_after(2) == 4
    assert ring.nb_entries == 4 * ring.N


@pytest.mark.parametrize("compact", [False, True])
def test_state_pickle_roundtrip(mods, compact):
    src = fill(make(mods, compact=compact), 1)
    s = src.state()
    assert list(s) == ["obs_shape", "action", "reward", "terminal", "cur", "filled", "patch" if compact else "obs"]
    assert s["obs_shape"] == (5, 3) + OBS_SHAPE and all(isinstance(s[k], np.ndarray) for k in ("action", "reward", "terminal"))
    dst = make(mods, compact=compact)
    dst.presampled = (1, 2, 3)
    assert dst.load_state(pickle.loads(pickle.dumps(s))) is True
    assert same(src, dst) and torch.equal(src.store, dst.store) and dst.presampled is None


def test_patch_state_decodes_into_a_uint8_ring(mods):
    src = fill(make(mods, compact=True), 2)
    dst = make(mods, compact=False)
    assert dst.load_state(pickle.loads(pickle.dumps(src.state())))
    assert dst.store.dtype == torch.uint8 and torch.equal(dst.store, src.patch_to_obs(src.store)) and same(src, dst)
    back = make(mods, compact=True)                     # and the uint8 pickle encodes into a compact ring: the same images (random words
    assert back.load_state(dst.state()) and same(back, dst)     # are not ones the environment writes: only their decoded form round-trips)


def test_copy_from_refuses_another_shape(mods):
    src = fill(make(mods, T=5, N=3), 3)
    for other in (make(mods, T=5, N=4), make(mods, T=6, N=3)):
        fill(other, 4, cur=1, filled=3)
        before = (other.store.clone(), other.action.clone(), other.reward.clone(), other.terminal.clone(), other.cur, other.filled)
        assert other.copy_from(src) is False and other.load_state(src.state()) is False
        assert all(torch.equal(a, b) for a, b in zip(before[:4], (other.store, other.action, other.reward, other.terminal)))
        assert (other.cur, other.filled) == before[4:]
    for compact in (False, True):
        dst = make(mods, compact=compact)
        assert dst.copy_from(src) is True and same(src, dst)
    assert make(mods, compact=True).load_state(None) is False


def test_eval_swap_restores_every_field_even_an_unknown_one(mods):
    """DQNCore.begin_eval / end_eval on a stand-in core: the evaluation runs on a three-slot scratch ring and the training ring comes
    back as the same object -- every field, one added later included (the failure a hand-written field tuple invited)."""
    core_mod = importlib.import_module("deepq-decoding_amd.core")
    for compact in (False, True):
        ring = fill(make(mods, compact=compact), 5)
        ring.presampled = (7, 3, 4)
        ring.priority = torch.arange(ring.T * ring.N).reshape(ring.T, ring.N)       # a made-up extra attribute
        want = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in vars(ring).items()}
        core = types.SimpleNamespace(ring=ring, started=True, _train_ring=None, _flush_stats=lambda: None, _join_env=lambda: None,
                                     env=types.SimpleNamespace(disarm_patch_output=lambda: None))
        core_mod.DQNCore.begin_eval(core)
        s = core.ring
        assert s is not ring and (s.T, s.N, s.cur, s.filled, s.presampled, s.compact) == (3, ring.N, 0, 0, None, compact)
        assert s.store.shape[1:] == ring.store.shape[1:] and s.store.dtype == ring.store.dtype and not hasattr(s, "priority")
        s.advance(); s.action.fill_(9); s.store.fill_(1); s.presampled = (1, 1, 1)      # what an evaluation does to its ring
        with pytest.raises(AssertionError):
            core_mod.DQNCore.begin_eval(core)                                           # (no evaluation inside an evaluation)
        core_mod.DQNCore.end_eval(core)
        assert core.ring is ring and core._train_ring is None and core.started is False
        got = vars(ring)
        assert set(got) == set(want)
        assert all(torch.equal(got[k], v) if torch.is_tensor(v) else got[k] == v for k, v in want.items())


def test_a_parent_format_state_dict_loads(mods):
    """The pickled form is pinned: the dict SequentialMemory wrote before ReplayRing existed, built by hand key by key."""
    T, N = 4, 2
    g = np.random.default_rng(6)
    obs = g.integers(0, 2, (T, N) + OBS_SHAPE).astype(np.uint8)
    old = dict(obs_shape=(T, N) + OBS_SHAPE, action=g.integers(0, 51, (T, N)).astype(np.int32), reward=g.random((T, N)).astype(np.float32),
               terminal=g.integers(0, 2, (T, N)).astype(np.uint8), cur=3, filled=4, obs=np.packbits(obs, axis=None))
    ring = make(mods, T=T, N=N)
    assert ring.load_state(pickle.loads(pickle.dumps(old)))
    assert np.array_equal(ring.store.numpy(), obs) and np.array_equal(ring.action.numpy(), old["action"])
    assert np.array_equal(ring.reward.numpy(), old["reward"]) and np.array_equal(ring.terminal.numpy(), old["terminal"])
    assert (ring.cur, ring.filled, ring.nb_entries) == (3, 4, 8)
    new = ring.state()
    assert list(new) == list(old) and all(np.array_equal(new[k], old[k]) for k in old)
    words = g.integers(0, 1 << 22, (T, N, 32)).astype(np.int32)
    words[..., D * D:] = 0
    old_patch = dict(old, patch=words)
    del old_patch["obs"]
    compact = make(mods, T=T, N=N, compact=True)
    assert compact.load_state(old_patch) and np.array_equal(compact.store.numpy(), words)
    assert list(compact.state()) == list(old_patch) and np.array_equal(compact.state()["patch"], words)
    # and through SequentialMemory, as an unpickled memory.p reaches a new core
    agent = importlib.import_module("deepq-decoding_amd.agent")
    mem = agent.SequentialMemory(limit=100)
    mem.__setstate__(dict(limit=100, window_length=1, _saved=old))
    assert mem.nb_entries == 8
    fresh = make(mods, T=T, N=N)
    assert mem._restore_into(types.SimpleNamespace(ring=fresh)) and np.array_equal(fresh.store.numpy(), obs)
    mem._core = types.SimpleNamespace(ring=fresh)
    st = mem.__getstate__()
    assert list(st) == ["limit", "window_length", "_saved"] and list(st["_saved"]) == list(old) and mem.nb_entries == 8
