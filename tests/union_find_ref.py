"""The union-find decoder (include/deepq_hip.h dq_decode_uf) in plain numpy / Python over match_st_ref.Component, for
tests/test_union_find_cpu.py and tests/test_union_find_gpu.py.  An independent statement of the algorithm: clusters are kept in a disjoint-set forest
with per-cluster attributes, the peeling walks explicit adjacency lists.

Graph of one Pauli component with n nodes per round: node (u, t) = t n + u, the boundary node B = depth n (spatial and future boundary merged); edges
of round t have ids t (d^2 + n) + k: k = q < d^2 the space edge of qubit q (its two plaquettes of the component in slice t, or its one plaquette and B),
k = d^2 + u the time edge (u, t) -- (u, t + 1), in the last round (u, t) -- B.  Unit weights.

Growth in synchronous rounds: every edge carries g in {0, 1, 2}; a cluster is active when it holds an odd number of defects and not B; in a round every
edge gains 1 per endpoint that lies in an active cluster (capped at 2), then the ends of every edge with g = 2 are united; until no cluster is active.
Peeling over the full edges: roots (level 0) are B and the lowest node of every cluster without B, levels by breadth-first search, the parent edge of a node
is the lowest edge id that joins it to the previous level; from the deepest level down, a node with an odd number of defects in its subtree puts its
parent edge into the correction."""
import numpy as np

from match_st_ref import Component


class Graph:
    _cache = {}

    def __new__(cls, d, comp, depth):
        key = (d, comp, depth)
        if key not in cls._cache:
            self = super().__new__(cls)
            C = Component(d, comp)
            n, d2 = C.n, d * d
            self.C, self.n, self.d2, self.depth, self.per_round, self.B = C, n, d2, depth, d2 + n, depth * n
            ends, qubit = [], []
            for t in range(depth):
                for q in range(d2):
                    nodes = np.flatnonzero(C.H[q])
                    assert len(nodes) in (1, 2)                                        # every qubit has one or two plaquettes per component
                    ends.append((t * n + int(nodes[0]), t * n + int(nodes[1]) if len(nodes) == 2 else self.B))
                    qubit.append(q)
                for u in range(n):
                    ends.append((t * n + u, (t + 1) * n + u if t + 1 < depth else self.B))
                    qubit.append(-1)
            self.ends = np.array(ends, dtype=np.int64)
            self.qubit = qubit
            self.bound = 2 * depth * (d2 + n)
            cls._cache[key] = self
        return cls._cache[key]


def decode_component(d, comp, rows, depth):
    """rows: 0/1 [depth, n] defects.  Returns (M: qubit mask of the correction's space edges, W: its edges, ndef, rounds)."""
    G = Graph(d, comp, depth)
    B, ends = G.B, G.ends
    defect = np.zeros(B + 1, dtype=bool)
    defect[:B] = np.asarray(rows).reshape(-1) != 0
    ndef = int(defect.sum())
    up = list(range(B + 1))

    def find(x):
        r = x
        while up[r] != r:
            r = up[r]
        while up[x] != r:
            up[x], x = r, up[x]
        return r

    g = np.zeros(len(ends), dtype=np.int64)
    rounds = 0
    while True:
        root = np.array([find(x) for x in range(B + 1)])
        odd = (np.bincount(root[defect], minlength=B + 1) & 1).astype(bool)
        odd[root[B]] = False                                                           # a cluster that holds B is never active
        act = odd[root]
        if not act.any():
            break
        assert rounds < G.bound
        rounds += 1
        before = int(g.sum())
        g = np.minimum(2, g + act[ends[:, 0]] + act[ends[:, 1]])
        assert int(g.sum()) > before                                                   # an active cluster always has an edge that is not full
        for e in np.flatnonzero(g == 2):
            a, b = find(int(ends[e, 0])), find(int(ends[e, 1]))
            if a != b:
                up[a] = b
    # ---- peeling ----------------------------------------------------------------------------------------------------------------------------
    full = [int(e) for e in np.flatnonzero(g == 2)]
    adj = {}
    for e in full:                                                                     # ascending edge ids
        a, b = int(ends[e, 0]), int(ends[e, 1])
        adj.setdefault(a, []).append((e, b))
        adj.setdefault(b, []).append((e, a))
    root = [find(x) for x in range(B + 1)]
    lowest = {}
    for x in range(B + 1):
        lowest.setdefault(root[x], x)
    roots = [B] + [x for r, x in lowest.items() if r != root[B]]
    level = {x: 0 for x in roots}
    parent = {}
    order = [list(roots)]
    while order[-1]:
        nxt = {}
        for x in order[-1]:
            for e, y in adj.get(x, ()):
                if y not in level and (y not in nxt or e < nxt[y][0]):
                    nxt[y] = (e, x)
        for y, ex in nxt.items():
            level[y] = len(order)
            parent[y] = ex
        order.append(sorted(nxt))
    assert len(level) == B + 1                                                         # every node hangs on a root
    par = defect.astype(np.int64)
    correction = []
    for nodes in reversed(order[1:]):
        for y in nodes:
            if par[y] & 1:
                e, x = parent[y]
                correction.append(e)
                par[x] ^= 1
    for x in roots:
        assert x == B or par[x] % 2 == 0                                               # every root but B ends even
    M = 0
    for e in correction:
        q = G.qubit[e]
        if q >= 0:
            M ^= 1 << q
    return M, len(correction), ndef, rounds


_memo = {}


def decode(d, volumes, depth):
    """volumes uint8 [N, depth, d+1, d+1] -> (frame uint8 [N, d, d] hidden_state codes, weight, n_defects, rounds: int32 [N, 2]).  A component's result
    is computed once per distinct defect pattern."""
    v = np.asarray(volumes)
    N, d2 = len(v), d * d
    out = np.zeros((N, 2, 4), dtype=np.int64)                                          # M, W, ndef, rounds
    for c in range(2):
        rows = Component(d, c).defects(v).astype(np.uint8)
        pats, inverse = np.unique(rows.reshape(N, -1), axis=0, return_inverse=True)
        table = np.zeros((len(pats), 4), dtype=np.int64)
        for k, pat in enumerate(pats):
            key = (d, c, depth, pat.tobytes())
            if key not in _memo:
                _memo[key] = decode_component(d, c, pat.reshape(depth, -1), depth)
            table[k] = _memo[key]
        out[:, c] = table[np.asarray(inverse).reshape(-1)]
    q = np.arange(d2, dtype=np.int64)
    x, z = (out[:, 0, 0, None] >> q) & 1, (out[:, 1, 0, None] >> q) & 1
    frame = np.where(x & z, 2, np.where(x, 1, np.where(z, 3, 0))).astype(np.uint8).reshape(N, d, d)
    return frame, out[:, :, 1].astype(np.int32), out[:, :, 2].astype(np.int32), out[:, :, 3].astype(np.int32)


def hand_cases():
    """(name, d, comp, depth, defect rows [depth, n], expected) of hand-made component patterns at d = 5 and 7; expected: a dict with any of M (qubit
    mask), W, rounds -- what can be said without running the algorithm.  The two dense patterns carry no expectation: they are for comparisons."""
    for d, depth in ((5, 5), (7, 7), (7, 16)):
        for comp in (0, 1):
            C = Component(d, comp)
            n = C.n
            distB = np.asarray(C.graph.distB).reshape(n, 2).astype(np.int64)
            near = distB.min(axis=1)
            zero = lambda: np.zeros((depth, n), dtype=np.int64)
            yield f"d{d}_{depth}_c{comp}_none", d, comp, depth, zero(), dict(M=0, W=0, rounds=0)
            for u in range(n):
                for t in sorted({0, depth // 2, depth - 1}):
                    rows = zero()
                    rows[t, u] = 1
                    want = dict(W=int(min(near[u], depth - t)))
                    if depth - t < near[u]:
                        want["M"] = 0                                                  # the future boundary is strictly nearer: time edges only
                    if t == depth - 1:
                        # one edge either way; where the spatial boundary is one edge away too, the lower edge id wins: the space edge
                        want["W"] = 1
                        if near[u] == 1:
                            q = min(q for q in range(d * d) if C.H[q].sum() == 1 and C.H[q, u])
                            want["M"] = 1 << q
                    yield f"d{d}_{depth}_c{comp}_lone_u{u}_t{t}", d, comp, depth, rows, want
            u = int(np.argmax(near))
            rows = zero()
            rows[1, u] = rows[2, u] = 1
            yield f"d{d}_{depth}_c{comp}_time_pair", d, comp, depth, rows, dict(M=0, W=1, rounds=1)
            q = next(q for q in range(d * d) if C.H[q].sum() == 2)
            a, b = np.flatnonzero(C.H[q])
            rows = zero()
            rows[depth // 2, a] = rows[depth // 2, b] = 1
            yield f"d{d}_{depth}_c{comp}_space_pair", d, comp, depth, rows, dict(M=1 << q, W=1, rounds=1)
            if d == 7:
                u = next(j for j, cell in enumerate(C.cells) if tuple(cell) in ((3, 4), (4, 4)))      # the central plaquette: three edges from the boundary
                rows = zero()
                rows[0, u] = 1
                yield f"d7_{depth}_c{comp}_central", d, comp, depth, rows, dict(W=3, rounds=6)
            rows = zero()
            rows[depth // 2, :] = 1
            yield f"d{d}_{depth}_c{comp}_full_slice", d, comp, depth, rows, {}
            yield f"d{d}_{depth}_c{comp}_everything", d, comp, depth, np.ones((depth, n), dtype=np.int64), {}
