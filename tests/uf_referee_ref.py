"""The union-find referee (include/deepq_hip.h dq_uf_referee_decode / dq_envb_set_referee / dq_wide_uf_verdict_refereed_uf; csrc/uf_plane_dev.h; DESIGN.md
section 29) in numpy / Python, for tests/test_uf_referee_cpu.py and tests/test_uf_referee_gpu.py.

The rule.  The union-find referee's class for component c of a perfect syndrome s: nodes are c's plaquettes in lattice.typed_order (the look-up and matching
referee's index order, match_st_ref.Component's); s is decoded with section 20's closed component decode on a one-round window -- only the d^2 space edges are
alive and edge id = qubit id; growth, min-labels and the lowest-edge-id peeling are closed_uf_ref.window_edges' --; the class is the parity of the logical bits
(Component.logical) of the correction's qubits.  The empty syndrome gives class 0.  Under the X model only component 0 is asked.  `inexact` is always 0."""
import functools

import numpy as np

import closed_uf_ref as CU
import verdict_wide_ref as V
from match_st_ref import Component

REFEREE_MATCHING, REFEREE_UNION_FIND = 0, 1


def classify(d, comp, syndrome):
    """The class bit of component comp for the 0/1 syndrome [n] in the component's node order."""
    C = Component(d, comp)
    rows = np.asarray(syndrome).astype(np.int64).reshape(1, C.n)
    edges, _ = CU.window_edges(d, comp, rows, 1, closed=True)
    assert all(e < d * d for e in edges)                                              # the window's time edges are not alive
    return int(C.logical[edges].sum() & 1) if edges else 0


def bits_of(d, words):
    """0/1 [n] of a component's two defect words (bit i = node i)."""
    n = (d * d - 1) // 2
    return np.array([(int(words[j >> 6]) >> (j & 63)) & 1 for j in range(n)], dtype=np.int64)


def words_of(syndromes):
    """uint64 [N, 2] defect words of 0/1 rows [N, n]."""
    s = np.asarray(syndromes).astype(np.uint64)
    out = np.zeros((len(s), 2), dtype=np.uint64)
    for j in range(s.shape[1]):
        out[:, j >> 6] |= s[:, j] << np.uint64(j & 63)
    return out


def classify_words(d, error_model, defects):
    """defects: uint64 [N, 2 components, 2 words] (MatchingReferee.pack's layout) -> class uint8 [N] = X part + 2 * Z part."""
    defects = np.asarray(defects, dtype=np.uint64).reshape(-1, 2, 2)
    out = np.zeros(len(defects), dtype=np.uint8)
    for i, row in enumerate(defects):
        c = classify(d, 0, bits_of(d, row[0]))
        if error_model != "X":
            c += 2 * classify(d, 1, bits_of(d, row[1]))
        out[i] = c
    return out


def error_syndrome(d, comp, errors):
    """(0/1 syndromes [N, n], the errors' class bits [N]) of 0/1 component errors [N, d^2]."""
    C = Component(d, comp)
    e = np.asarray(errors).astype(np.int64).reshape(-1, d * d)
    return (e @ C.H) & 1, (e @ C.logical) & 1


def sample_defects(d, p, n, seed):
    """Defect words uint64 [n, 2, 2] of i.i.d. component errors at rate p, and the errors' classes uint8 [n] (X part + 2 * Z part)."""
    rng = np.random.default_rng(seed)
    out = np.zeros((n, 2, 2), dtype=np.uint64)
    cls = np.zeros(n, dtype=np.uint8)
    for comp in range(2):
        s, c = error_syndrome(d, comp, rng.random((n, d * d)) < p)
        out[:, comp] = words_of(s)
        cls += ((1 + comp) * c).astype(np.uint8)
    return out, cls


class Restatement(V.Restatement):
    """verdict_wide_ref.Restatement with the classifier swapped: the union-find referee, no flags (and no C matching oracle behind it)."""

    def __init__(self, d, error_model):
        from oracle import lattice
        self.d, self.error_model, self.masks = d, error_model, lattice.Masks(d)
        m = self.masks
        self.qubits = [[q for q in range(d * d) if (m.stab_qmask[s] >> q) & 1] for s in range(m.n_stab)]
        self.col0 = np.array([(m.col0_mask >> q) & 1 for q in range(d * d)], dtype=bool)
        self.row0 = np.array([(m.row0_mask >> q) & 1 for q in range(d * d)], dtype=bool)

    def verdict(self, hidden, frame=None):
        x, z = V.planes(hidden, frame)
        syn = self.syndrome(x, z)
        in_code = ~syn.any(axis=1)
        cls = ((x & self.col0).sum(axis=1) & 1) + 2 * ((z & self.row0).sum(axis=1) & 1)
        bits = np.stack([self.defect_words(syn, 3), self.defect_words(syn, 1)], axis=1)
        dec = classify_words(self.d, self.error_model, bits).astype(np.int64)
        assert not dec[in_code].any()
        success = in_code & (cls == 0)
        out = (in_code * V.IN_CODESPACE) | (cls << V.CLASS_SHIFT) | (success * V.SUCCESS) | ((success | (dec == cls)) * V.ALIVE) | (dec << V.DECODED_SHIFT)
        return dict(byte=out.astype(np.uint8), bits=bits)


@functools.lru_cache(maxsize=None)
def restatement(d, error_model):
    return Restatement(d, error_model)


def step_rule_batch(d, error_model, use_Y, x, z, actions, done_before):
    """Environments.py:139-151 with this referee and sticky done: x, z 0/1 [N, d^2] planes before the step, the action index of each lattice.  Returns
    (reward float32 [N], done uint8 [N]).  The action is applied whatever done_before says (the step without auto-reset does)."""
    d2 = d * d
    layers = 1 if error_model == "X" else (3 if use_Y else 2)
    x, z = np.array(x, dtype=bool).reshape(-1, d2), np.array(z, dtype=bool).reshape(-1, d2)
    for i, a in enumerate(np.asarray(actions).reshape(-1).tolist()):
        if a == layers * d2:
            continue
        layer, q = divmod(int(a), d2)
        pauli = 1 if error_model == "X" else (layer + 1 if use_Y else (1 if layer == 0 else 3))
        x[i, q] ^= pauli != 3
        z[i, q] ^= pauli != 1
    b = restatement(d, error_model).verdict(V.codes(x, z).reshape(-1, d, d))["byte"]
    reward = ((b & V.SUCCESS) != 0).astype(np.float32)
    done = (np.asarray(done_before).reshape(-1) != 0) | ((b & V.ALIVE) == 0)           # (alive includes success: the reward never ends an episode)
    return reward, done.astype(np.uint8)


def step_rule(d, error_model, use_Y, x, z, action, done_before):
    """step_rule_batch on one lattice: (reward, done)."""
    r, dn = step_rule_batch(d, error_model, use_Y, np.asarray(x)[None], np.asarray(z)[None], [action], [done_before])
    return float(r[0]), bool(dn[0])


def state_planes(state, d):
    """(x, z) 0/1 [N, d^2] of VectorEnv.export_state() rows on the wide backend (x[W] z[W] ... ; bit q of word q >> 6)."""
    W = (d * d + 63) // 64
    words = np.asarray(state).view(np.uint64)
    q = np.arange(d * d)
    plane = lambda o: ((words[:, o + (q >> 6)] >> (q & 63).astype(np.uint64)) & np.uint64(1)).astype(np.int64)
    return plane(0), plane(W)


def grids_of(d, defects):
    """uint8 [N, d+1, d+1] syndrome grids of defect words uint64 [N, 2, 2] (the inverse of MatchingReferee.pack)."""
    defects = np.asarray(defects, dtype=np.uint64).reshape(-1, 2, 2)
    out = np.zeros((len(defects), d + 1, d + 1), dtype=np.uint8)
    for comp in range(2):
        for j, (a, b) in enumerate(Component(d, comp).cells):
            out[:, a, b] = ((defects[:, comp, j >> 6] >> np.uint64(j & 63)) & np.uint64(1)).astype(np.uint8)
    return out


def frame_class(d, frame):
    """X part + 2 * Z part of frames in hidden_state codes [N, d, d]: the parity of the X plane on column 0 and of the Z plane on row 0."""
    f = np.asarray(frame).reshape(-1, d, d)
    x, z = (f == 1) | (f == 2), f >= 2
    return ((x[:, :, 0].sum(axis=1) & 1) + 2 * (z[:, 0, :].sum(axis=1) & 1)).astype(np.uint8)
