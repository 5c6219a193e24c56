"""The refereed verdict in numpy (include/deepq_hip.h dq_wide_uf_verdict_refereed): what the step decides on the residual hidden XOR
frame (the reference's Environments.py:139-151), any odd d in 3 .. 15.  The residual, its true syndrome and its class come from oracle/lattice.py's Masks --
`verdict_one` calls syndrome_word / referee_index / col0_mask / row0_mask on Python integers, `Restatement` does the same sums on arrays built from the same
tables (tests/test_verdict_wide_cpu.py holds the two against each other) -- and the decoded class and the fallback flags from oracle/c_oracle.py's
CWideMatch.classify_bits.  Also the inputs the CPU and the GPU tests share, so that the conditions asserted on the restatement are conditions on what the
device is given."""
import functools

import numpy as np

from oracle import c_oracle, lattice

IN_CODESPACE, CLASS_SHIFT, SUCCESS, ALIVE, DECODED_SHIFT = 1, 1, 8, 16, 5


def planes(hidden, frame=None):
    """(x, z) bool [N, d^2] of the residual: codes 1, 2 carry an X component, codes 2, 3 a Z component; the product of two Paulis is the XOR of the components."""
    h = np.asarray(hidden).reshape(len(hidden), -1)
    x, z = (h == 1) | (h == 2), h >= 2
    if frame is not None:
        f = np.asarray(frame).reshape(len(frame), -1)
        x, z = x ^ ((f == 1) | (f == 2)), z ^ (f >= 2)
    return x, z


def codes(x, z):
    """hidden_state codes uint8 of the planes: X = 1, Y = 2, Z = 3."""
    return np.where(x, np.where(z, 2, 1), np.where(z, 3, 0)).astype(np.uint8)


def byte(in_code, cls, decoded):
    success = in_code and cls == 0
    return (IN_CODESPACE if in_code else 0) | (cls << CLASS_SHIFT) | (SUCCESS if success else 0) | (ALIVE if success or decoded == cls else 0) | (decoded << DECODED_SHIFT)


def verdict_one(masks, error_model, xmask, zmask, classify):
    """The byte of one residual given as plane integers; classify(component, index) is the referee's class of a component's look-up index.  A residual in
    the code space is not sent to the referee (decoded = 0)."""
    w = masks.syndrome_word(xmask, zmask)
    cls = (bin(xmask & masks.col0_mask).count("1") & 1) + 2 * (bin(zmask & masks.row0_mask).count("1") & 1)
    dec = 0
    if w:
        dec = classify(0, masks.referee_index(w, 3))
        if error_model != "X":
            dec += 2 * classify(1, masks.referee_index(w, 1))
    return byte(w == 0, cls, dec)


class Restatement:
    """verdict(hidden, frame) -> dict(byte, inexact uint8 [N], flags uint8 [N, 2] as CWideMatch reports them, bits uint64 [2][N, 2] the defect words)."""

    def __init__(self, d, error_model):
        self.d, self.error_model, self.masks = d, error_model, lattice.Masks(d)
        m = self.masks
        self.qubits = [[q for q in range(d * d) if (m.stab_qmask[s] >> q) & 1] for s in range(m.n_stab)]
        self.col0 = np.array([(m.col0_mask >> q) & 1 for q in range(d * d)], dtype=bool)
        self.row0 = np.array([(m.row0_mask >> q) & 1 for q in range(d * d)], dtype=bool)
        self.match = c_oracle.CWideMatch(d)

    def syndrome(self, x, z):
        """bool [N, n_stab]: Masks.syndrome_word's bits."""
        m = self.masks
        return np.stack([(x if m.stab_type[s] == 3 else z)[:, self.qubits[s]].sum(axis=1) & 1 for s in range(m.n_stab)], axis=1).astype(bool)

    def defect_words(self, syn, typ):
        """uint64 [N, 2]: Masks.referee_index of the component as two words."""
        m = self.masks
        bits = np.zeros((len(syn), 2), dtype=np.uint64)
        for s in range(m.n_stab):
            if m.stab_type[s] == typ:
                j = m.ref_bit[s]
                bits[:, j >> 6] |= syn[:, s].astype(np.uint64) << np.uint64(j & 63)
        return bits

    def verdict(self, hidden, frame=None):
        x, z = planes(hidden, frame)
        syn = self.syndrome(x, z)
        in_code = ~syn.any(axis=1)
        cls = ((x & self.col0).sum(axis=1) & 1) + 2 * ((z & self.row0).sum(axis=1) & 1)
        bits = [self.defect_words(syn, 3), self.defect_words(syn, 1)]
        c0, _, f0 = self.match.classify_bits(0, bits[0])
        dec, flags = c0.astype(np.int64), np.stack([f0, np.zeros_like(f0)], axis=1)
        if self.error_model != "X":
            c1, _, f1 = self.match.classify_bits(1, bits[1])
            dec, flags[:, 1] = dec + 2 * c1, f1
        assert not dec[in_code].any() and not flags[in_code].any()     # the referee's answer to the empty syndrome: what the early exit writes
        success = in_code & (cls == 0)
        out = (in_code * IN_CODESPACE) | (cls << CLASS_SHIFT) | (success * SUCCESS) | ((success | (dec == cls)) * ALIVE) | (dec << DECODED_SHIFT)
        return dict(byte=out.astype(np.uint8), inexact=(flags != 0).any(axis=1).astype(np.uint8), flags=flags, bits=bits)


@functools.lru_cache(maxsize=None)
def restatement(d, error_model):
    return Restatement(d, error_model)


def kinds(b):
    """The four kinds of volumes a sparse case must hold, as counts."""
    b = np.asarray(b)
    return dict(success=int(((b & SUCCESS) != 0).sum()), in_code_wrong_class=int((((b & IN_CODESPACE) != 0) & ((b & SUCCESS) == 0)).sum()),
                alive_outside=int((((b & ALIVE) != 0) & ((b & IN_CODESPACE) == 0)).sum()), dead=int(((b & ALIVE) == 0).sum()))


# ---- inputs --------------------------------------------------------------------------------------------------------------------------------------------
def iid_hidden(d, n, density, rng):
    """Every component of every qubit drawn independently at `density`."""
    return codes(rng.random((n, d * d)) < density, rng.random((n, d * d)) < density).reshape(n, d, d)


def logical_planes(d):
    """(an X string that flips the class bit 1, a Z string that flips the class bit 2) as bool [d^2], both in the code space: X along row 0 meets column 0 once,
    Z along column 0 meets row 0 once."""
    lx, lz = np.zeros((d, d), dtype=bool), np.zeros((d, d), dtype=bool)
    lx[0, :] = True
    lz[:, 0] = True
    return lx.reshape(-1), lz.reshape(-1)


SPARSE_N, SPARSE_DENSITY = 257, 0.02
SPARSE_CASES = [(d, model) for d in (5, 7, 9, 11, 13, 15) for model in ("X", "DP", "IIDXZ")]
NARROW_CASES = [(d, model) for d in (3, 5, 7) for model in ("X", "DP")]


@functools.lru_cache(maxsize=None)
def sparse_case(d, error_model):
    """(hidden, frame) uint8 [257, d, d] of the sparse and cancelled residuals: hidden iid at density 0.02 per component; frame by thirds zeros (what NULL
    means), hidden times a random product of stabilizers and, on every other volume of that third, a logical operator, and hidden with one to three
    qubits changed.  Read-only."""
    R = restatement(d, error_model)
    m, n = R.masks, SPARSE_N
    rng = np.random.default_rng(1000 * d + {"X": 0, "DP": 1, "IIDXZ": 2}[error_model])
    hidden = iid_hidden(d, n, SPARSE_DENSITY, rng)
    frame = np.zeros_like(hidden)
    a, b = n // 3, 2 * (n // 3)
    lx, lz = logical_planes(d)
    for i in range(a, b):
        x, z = planes(hidden[i:i + 1])
        x, z = x[0].copy(), z[0].copy()
        for s in np.flatnonzero(rng.random(m.n_stab) < 0.5):           # a type-3 plaquette reads the X plane, so as an operator it is a product of Z's
            mask = np.zeros(d * d, dtype=bool)
            mask[R.qubits[s]] = True
            if m.stab_type[s] == 3:
                z ^= mask
            else:
                x ^= mask
        if (i - a) % 2:
            which = 1 + (i - a) // 2 % 3                                # X, Z, both in turn
            if which & 1:
                x ^= lx
            if which & 2:
                z ^= lz
        frame[i] = codes(x, z).reshape(d, d)
    for i in range(b, n):
        f = hidden[i].reshape(-1).copy()
        for q in rng.choice(d * d, size=1 + (i - b) % 3, replace=False):
            f[q] = (f[q] + rng.integers(1, 4)) & 3
        frame[i] = f.reshape(d, d)
    hidden.setflags(write=False)
    frame.setflags(write=False)
    return hidden, frame


@functools.lru_cache(maxsize=None)
def sparse_expected(d, error_model):
    hidden, frame = sparse_case(d, error_model)
    return restatement(d, error_model).verdict(hidden, frame)


def exhaustive_d3(error_model):
    """Every hidden state of d = 3: 4^9 for DP, the 2^9 X patterns for X."""
    if error_model == "X":
        k = np.arange(512)
        return ((k[:, None] >> np.arange(9)) & 1).astype(np.uint8).reshape(-1, 3, 3)
    k = np.arange(1 << 18)
    return ((k[:, None] >> (2 * np.arange(9))) & 3).astype(np.uint8).reshape(-1, 3, 3)


POOL_CASE = dict(d=9, error_model="DP", n=256, density=0.12, seed=907)          # clusters of 15 .. 20 defects: the scratch-pool path
FALLBACK_CASE = dict(d=15, error_model="DP", n=64, density=0.06, seed=1506)     # clusters beyond 20, lists beyond 32: the flagged fallbacks


@functools.lru_cache(maxsize=None)
def dense_case(name):
    c = dict(pool=POOL_CASE, fallback=FALLBACK_CASE)[name]
    hidden = iid_hidden(c["d"], c["n"], c["density"], np.random.default_rng(c["seed"]))
    hidden.setflags(write=False)
    return hidden, restatement(c["d"], c["error_model"]).verdict(hidden)


def listed_defects(d, typ, words):
    from oracle import matching_referee
    return [j for j in range((d * d - 1) // 2) if (int(words[j >> 6]) >> (j & 63)) & 1][:matching_referee.MAX_LIST]


def cluster_sizes(d, typ, words):
    """The sizes of the clusters of one component's defects, ordered by their lowest member: oracle/matching_referee.py ComponentGraph.clusters over the
    first 32 listed, with the `connected` rule evaluated on arrays (the CPU tests hold it against that method)."""
    from oracle.matching_referee import BIG, INF
    g = _graph(d, typ)
    D = np.array(listed_defects(d, typ, words), dtype=np.int64)
    if not len(D):
        return []
    b = np.where(g.distB[D] == INF, BIG, g.distB[D].astype(np.int64))
    dist = g.dist[np.ix_(D, D)].astype(np.int64)
    bound = [np.minimum(b[:, None, 0] + b[None, :, cp], b[:, None, 1] + b[None, :, 1 ^ cp]) for cp in (0, 1)]
    adj = ((dist[..., 0] != INF) & (dist[..., 0] < bound[0])) | ((dist[..., 1] != INF) & (dist[..., 1] < bound[1]))
    np.fill_diagonal(adj, False)
    label = np.arange(len(D))
    while True:
        new = np.minimum(label, np.where(adj, label[None, :], len(D)).min(axis=1))
        if np.array_equal(new, label):
            break
        label = new
    return [int((label == r).sum()) for r in range(len(D)) if label[r] == r]


@functools.lru_cache(maxsize=None)
def _graph(d, typ):
    from oracle import matching_referee
    return matching_referee.ComponentGraph(d, typ)
