"""Two independent checkers of the space-time matching decoder (include/deepq_hip.h dq_decode_match), for
tests/test_match_st_cpu.py and tests/test_match_st_gpu.py.

Checker 1, `BfsTable`: the exhaustive minimum by breadth-first search over FAULT HISTORIES of one Pauli component -- no matching, no distances.
State = (defect bits of all rounds, measurement-error bits of the last round m_last, class bit); generators = the single faults: a data error on
qubit q in round t flips its plaquettes' defects in slice t and XORs the qubit's logical bit into the class; a measurement error at (s, t) flips the
defects (s, t) and (s, t + 1), in the last round (s, t) and m_last[s].  The search depth is the minimum number of faults.  Feasible at d = 3.

Checker 2, `dp_open` / `dp_history`: a plain class-aware subset DP over ALL the defects (no clusters), distances = oracle/matching_referee.py's
component graph plus |t1 - t2|.  open: the future boundary (class 0, depth - t) among the boundary options, minimum over both classes = W_min.
history(m_last, c): the last round's measurement errors GIVEN (their defects XOR-ed into the last slice, no future boundary) at |m_last| faults,
class c: the lightest fault history with that class and those last-round measurement errors -- what BfsTable.history tabulates.

The certificate (`certify`): a frame F with reported weight W is accepted iff  W = W_min  and  history(m_last = sigma(F) xor S_last, class(F)) = W:
some fault history of exactly the minimum weight reproduces the volume and has a net data error equivalent to F.  No tie-break is replicated."""
import numpy as np

from oracle import lattice, matching_referee, referee

BIG = 1 << 20
TYP = (3, 1)                                  # component 0: type-3 plaquettes (X errors), component 1: type-1 (Z errors)


class Component:
    """One Pauli component of the distance-d lattice: node j = the j-th plaquette of lattice.typed_order (LatticeHost::typed)."""
    _cache = {}

    def __new__(cls, d, comp):
        key = (d, comp)
        if key not in cls._cache:
            self = super().__new__(cls)
            self.d, self.comp, self.typ = d, comp, TYP[comp]
            self.cells = lattice.typed_order(d, self.typ)
            self.n, deltas = referee.component_deltas(d, self.typ)
            self.deltas = deltas                                                       # per qubit: node bits | logical bit << n
            self.H = np.array([[(dl >> j) & 1 for j in range(self.n)] for dl in deltas], dtype=np.int64)      # [d2, n]
            self.logical = np.array([(dl >> self.n) & 1 for dl in deltas], dtype=np.int64)
            self.graph = matching_referee.ComponentGraph(d, self.typ)
            cls._cache[key] = self
        return cls._cache[key]

    def syndromes(self, volumes):
        """S int64 [N, depth, n] of volumes uint8 [N, depth, d+1, d+1]."""
        v = np.asarray(volumes)
        return np.stack([v[:, :, a, b] for (a, b) in self.cells], axis=-1).astype(np.int64)

    def defects(self, volumes):
        s = self.syndromes(volumes)
        dd = s.copy()
        dd[:, 1:] ^= s[:, :-1]
        return dd

    def plane(self, frame):
        """The component's plane int64 [N, d2] of frames in hidden_state codes: X part (codes 1, 2) for component 0, Z part (2, 3) for 1."""
        c = np.asarray(frame).astype(np.int64).reshape(len(frame), -1)
        return ((c == 1) | (c == 2)).astype(np.int64) if self.comp == 0 else (c >= 2).astype(np.int64)

    def frame_syndrome_class(self, frame):
        p = self.plane(frame)
        return (p @ self.H) & 1, (p @ self.logical) & 1


def bits(rows):
    """0/1 arrays [..., k] -> integers (bit i = entry i)."""
    rows = np.asarray(rows).astype(np.int64)
    return (rows << np.arange(rows.shape[-1], dtype=np.int64)).sum(axis=-1)


class BfsTable:
    _cache = {}

    def __new__(cls, d, comp, depth):
        key = (d, comp, depth)
        if key in cls._cache:
            return cls._cache[key]
        self = super().__new__(cls)
        C = Component(d, comp)
        n = C.n
        self.n, self.depth, self.nd = n, depth, n * depth
        gens = []
        for t in range(depth):
            for dl in C.deltas:
                gens.append(((dl & ((1 << n) - 1)) << (t * n)) | (((dl >> n) & 1) << (self.nd + n)))
            for s in range(n):
                other = (1 << ((t + 1) * n + s)) if t + 1 < depth else (1 << (self.nd + s))
                gens.append((1 << (t * n + s)) | other)
        gens = np.array(sorted(set(g for g in gens if g)), dtype=np.int64)
        dist = np.full(1 << (self.nd + n + 1), -1, dtype=np.int16)
        dist[0] = 0
        frontier = np.zeros(1, dtype=np.int64)
        w = 0
        while frontier.size:
            w += 1
            nxt = np.unique((frontier[:, None] ^ gens[None, :]).ravel())
            nxt = nxt[dist[nxt] < 0]
            dist[nxt] = w
            frontier = nxt
        assert dist.min() >= 0                                                         # every (defects, m_last, class) has a history
        self.dist = dist.reshape(2, 1 << n, 1 << self.nd)                              # [class][m_last][defects]
        self.open = self.dist.min(axis=(0, 1))                                         # [defects]: W_min
        cls._cache[key] = self
        return self

    def history(self, defects, m_last, c):
        return self.dist[c, m_last, defects]


def _subset_dp(pd, pb):
    """f[all][c] of the class-aware subset DP; pd int [k, k, 2], pb int [k, 2] with BIG = none.  Level by level of the highest member."""
    k = len(pb)
    f = np.full((1 << k, 2), BIG, dtype=np.int64)
    f[0, 0] = 0
    for h in range(k):
        base = 1 << h
        r = np.arange(base)
        g0, g1 = f[:base, 0], f[:base, 1]
        best0, best1 = np.minimum(g0 + pb[h, 0], g1 + pb[h, 1]), np.minimum(g1 + pb[h, 0], g0 + pb[h, 1])
        for v in range(h):
            has = (r >> v) & 1 == 1
            rr = r ^ (1 << v)
            q0, q1 = f[rr, 0], f[rr, 1]
            d0, d1 = pd[h, v, 0], pd[h, v, 1]
            best0 = np.where(has, np.minimum(best0, np.minimum(q0 + d0, q1 + d1)), best0)
            best1 = np.where(has, np.minimum(best1, np.minimum(q1 + d0, q0 + d1)), best1)
        f[base:2 * base, 0], f[base:2 * base, 1] = np.minimum(best0, BIG), np.minimum(best1, BIG)
    return int(f[-1, 0]), int(f[-1, 1])


def _tables(C, nodes, ts, depth, future):
    g = C.graph
    k = len(nodes)
    nodes, ts = np.asarray(nodes, dtype=np.int64), np.asarray(ts, dtype=np.int64)
    pd = g.dist[nodes[:, None], nodes[None, :], :].astype(np.int64).reshape(k, k, 2)
    pd = np.where(pd == matching_referee.INF, BIG, pd + np.abs(ts[:, None] - ts[None, :])[:, :, None])
    pb = g.distB[nodes, :].astype(np.int64).reshape(k, 2)
    pb = np.where(pb == matching_referee.INF, BIG, pb)
    if future:
        pb[:, 0] = np.minimum(pb[:, 0], depth - ts)
    return pd, pb


def dp_open(C, defect_rows, depth):
    """W_min of the defects int [depth, n]: the lightest matching over both classes, future boundary open."""
    ts, nodes = np.nonzero(np.asarray(defect_rows))
    return min(_subset_dp(*_tables(C, nodes, ts, depth, True)))


def dp_history(C, defect_rows, m_last, c, depth):
    """The lightest fault history of class c whose last-round measurement errors are m_last (0/1 [n])."""
    rows = np.array(defect_rows, dtype=np.int64)
    m_last = np.asarray(m_last, dtype=np.int64)
    rows[depth - 1] ^= m_last
    ts, nodes = np.nonzero(rows)
    w = _subset_dp(*_tables(C, nodes, ts, depth, False))
    return min(w[c], w[c ^ 1] + C.graph.w10) + int(m_last.sum())


def certify(d, comp, volume, frame, weight, depth, w_min=None):
    """(ok, W_min, history weight) of ONE volume's component: frame [d, d] codes, weight the reported one."""
    C = Component(d, comp)
    rows = C.defects(volume[None])[0]
    s_last = C.syndromes(volume[None])[0, depth - 1]
    sig, cls = C.frame_syndrome_class(np.asarray(frame)[None])
    if w_min is None:
        w_min = dp_open(C, rows, depth)
    hist = dp_history(C, rows, sig[0] ^ s_last, int(cls[0]), depth)
    return (int(weight) == w_min and hist == int(weight)), w_min, hist
