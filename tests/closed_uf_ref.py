"""Union-find stream decoding with a perfect final round (include/deepq_hip.h dq_stream_decode_uf_closed / dq_stream_run_uf_closed /
dq_wide_uf_decode_closed / dq_wide_uf_run_closed) in numpy / Python, for tests/test_closed_uf_cpu.py and tests/test_closed_uf_gpu.py.

`window_edges(d, comp, rows, depth, closed)` states section 16's component decode on a graph built here: node (u, t) = t n + u, B = depth n, edge ids
t (d^2 + n) + k with k = q < d^2 the space edge of qubit q and k = d^2 + u the time edge (u, t) -- (u, t + 1), in the last round (u, t) -- B.  With
`closed` the time edges of the last round do not exist: they keep their ids, never grow, are never full and never in the correction.  Growth, min-labels
and the lowest-edge-id peeling are stream_uf_ref.window_edges' (with closed=False every result equals its).

`stream_component` is section 17's window schedule with Python integers for M, for any odd d and a window of up to 32 rounds; only the final window (the
one with a + w >= T) is decoded closed.  `sample_streams` is decode_eval_ref.sample_volumes' rule; closed, the measurement flips of round T - 1 are not
applied (the same Philox words are drawn)."""
import numpy as np

import decode_eval_ref as E
from match_st_ref import Component
from oracle import lattice, philox

MAX_WINDOW = 32
_graphs = {}


def graph(d, comp, depth, closed):
    """(ea, eb: int64 [NE] ends, alive: bool [NE], B)."""
    key = (d, comp, depth, bool(closed))
    if key not in _graphs:
        C = Component(d, comp)
        n, d2 = C.n, d * d
        B = depth * n
        ea, eb, alive = [], [], []
        for t in range(depth):
            for q in range(d2):
                nodes = np.flatnonzero(C.H[q])
                assert len(nodes) in (1, 2)
                ea.append(t * n + int(nodes[0]))
                eb.append(t * n + int(nodes[1]) if len(nodes) == 2 else B)
                alive.append(True)
            for u in range(n):
                ea.append(t * n + u)
                eb.append((t + 1) * n + u if t + 1 < depth else B)
                alive.append(not (closed and t + 1 == depth))
        _graphs[key] = (np.array(ea, dtype=np.int64), np.array(eb, dtype=np.int64), np.array(alive, dtype=bool), B)
    return _graphs[key]


def _roots(up):
    while True:
        nxt = up[up]
        if np.array_equal(nxt, up):
            return up
        up = nxt


def window_edges(d, comp, rows, depth, closed):
    """rows: 0/1 [depth, n] defects of one window.  Returns (the correction's edge ids, ascending; growth rounds)."""
    ea, eb, alive, B = graph(d, comp, depth, closed)
    defect = np.zeros(B + 1, dtype=bool)
    defect[:B] = np.asarray(rows).reshape(-1) != 0
    if not defect.any():
        return [], 0
    up = np.arange(B + 1)
    g = np.zeros(len(ea), dtype=np.int64)
    rounds = 0
    while True:
        up = _roots(up)
        odd = (np.bincount(up[defect], minlength=B + 1) & 1).astype(bool)
        odd[up[B]] = False                                                             # a cluster that holds B is never active
        act = odd[up]
        if not act.any():
            break
        assert rounds < 2 * len(ea)
        rounds += 1
        g1 = np.where(alive, np.minimum(2, g + act[ea] + act[eb]), 0)
        fresh = np.flatnonzero((g1 == 2) & (g != 2))
        assert (g1 != g).any()                                                         # an active cluster always has a living edge that is not full
        g = g1
        for e in fresh:
            a, b = int(ea[e]), int(eb[e])
            while up[a] != a:
                a = int(up[a])
            while up[b] != b:
                b = int(up[b])
            if a != b:
                up[a] = b
    # ---- peeling: breadth-first levels from B and from the lowest node of every other cluster, parent = the lowest edge id to the previous level ----
    adj = {}
    for e in np.flatnonzero(g == 2):                                                   # ascending edge ids
        a, b = int(ea[e]), int(eb[e])
        adj.setdefault(a, []).append((int(e), b))
        adj.setdefault(b, []).append((int(e), a))
    root_of_B = int(up[B])
    lowest = {}
    for x in sorted(adj):                                                              # (an untouched node is a root of its own: no defect, no edge)
        lowest.setdefault(int(up[x]), x)
    roots = [B] + [x for r, x in sorted(lowest.items(), key=lambda kv: kv[1]) if r != root_of_B]
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
    par = defect.astype(np.int64)
    correction = []
    for nodes in reversed(order[1:]):
        for y in nodes:
            if par[y] & 1:
                e, x = parent[y]
                correction.append(e)
                par[x] ^= 1
    for x in np.flatnonzero(defect):
        assert int(x) in level                                                         # every defect hangs on a root
    for x in roots:
        assert x == B or par[x] % 2 == 0                                               # every root but B ends even
    assert all(alive[e] for e in correction)
    return sorted(correction), rounds


def n_windows(T, w, c):
    return 1 if w >= T else -(-(T - w) // c) + 1


def stream_component(d, comp, rows, w, c, closed):
    """rows: 0/1 [T, n] defects of one stream's component.  Returns dict(M: a Python integer, bit q = qubit q; W, ndef, rounds, windows, last: the 0/1 [n]
    set of nodes whose last-round time edge to B the final window committed -- empty when closed)."""
    rows = np.asarray(rows).astype(np.int64)
    T, n = rows.shape
    T, w, c = int(T), int(w), int(c)
    if not (T >= 1 and 1 <= w <= MAX_WINDOW and 1 <= c <= w):
        raise ValueError(f"stream schedule: T = {T} >= 1, 1 <= window = {w} <= {MAX_WINDOW}, 1 <= commit = {c} <= window")
    d2 = d * d
    per_round = d2 + n
    carry = np.zeros(n, dtype=np.int64)
    last = np.zeros(n, dtype=np.int64)
    M = W = rounds = windows = 0
    a = 0
    while True:
        final = a + w >= T
        l = T - a if final else w
        win = rows[a:a + l].copy()
        win[0] ^= carry
        edges, r = window_edges(d, comp, win, l, closed and final)
        rounds += r
        windows += 1
        carry = np.zeros(n, dtype=np.int64)
        for e in edges:
            t, k = divmod(int(e), per_round)
            if not final and t >= c:
                continue
            W += 1
            if k < d2:
                M ^= 1 << k
            elif not final and t == c - 1:
                carry[k - d2] = 1
            elif final and t == l - 1:
                last[k - d2] = 1
        if final:
            break
        a += c
    assert windows == n_windows(T, w, c)
    return dict(M=M, W=W, ndef=int(rows.sum()), rounds=rounds, windows=windows, last=last)


def decode(d, syndromes, w, c, closed):
    """syndromes uint8 [N, T, d+1, d+1] -> (frame uint8 [N, d, d] hidden_state codes, weight, n_defects, rounds: int32 [N, 2], windows, last: a list of two
    0/1 arrays [N, n] per component)."""
    v = np.asarray(syndromes)
    N, d2 = len(v), d * d
    planes = np.zeros((N, 2, d2), dtype=np.int64)
    out = np.zeros((N, 2, 3), dtype=np.int64)
    last = []
    for comp in range(2):
        rows = Component(d, comp).defects(v)
        ls = np.zeros((N, rows.shape[2]), dtype=np.int64)
        for i in range(N):
            r = stream_component(d, comp, rows[i], w, c, closed)
            planes[i, comp] = [(r["M"] >> q) & 1 for q in range(d2)]
            out[i, comp] = r["W"], r["ndef"], r["rounds"]
            ls[i] = r["last"]
        last.append(ls)
    x, z = planes[:, 0], planes[:, 1]
    frame = np.where(x & z, 2, np.where(x, 1, np.where(z, 3, 0))).astype(np.uint8).reshape(N, d, d)
    return frame, out[:, :, 0].astype(np.int32), out[:, :, 1].astype(np.int32), out[:, :, 2].astype(np.int32), n_windows(v.shape[1], w, c), last


def sample_streams(d, error_model, T, n, p_phys, p_meas, seed, env_id_base=0, closed=False):
    """decode_eval_ref.sample_volumes at depth T; closed: the measurement flips of round T - 1 are dropped.  Returns (grids uint8 [n, T, d+1, d+1], hidden
    codes uint8 [n, d, d], trivial uint8 [n] of the syndromes as drawn)."""
    m = lattice.Masks(d)
    d2, ns = d * d, m.n_stab
    ids = ((int(env_id_base) + np.arange(n, dtype=np.uint64)) & np.uint64(philox.MASK)).astype(np.uint32)
    tp, tm = E._thresholds(p_phys, n)[:, None], E._thresholds(p_meas, n)[:, None]
    lanes = np.arange(d2, dtype=np.uint32)[None, :]
    x = np.zeros((n, d2), dtype=np.int64)
    z = np.zeros((n, d2), dtype=np.int64)
    grids = np.zeros((n, T, d + 1, d + 1), dtype=np.uint8)
    for j in range(T):
        w0, w1, w2, _ = philox.philox4x32_np(np.uint32(j), np.uint32(0), ids[:, None], lanes, seed)
        w0, w1, w2 = w0.astype(np.uint64), w1.astype(np.uint64), w2.astype(np.uint64)
        hit = w0 < tp
        if error_model == "IIDXZ":
            ex, ez = hit, w1 < tp
        elif error_model == "X":
            ex, ez = hit, np.zeros_like(hit)
        else:
            typ = 1 + ((w1 * np.uint64(3)) >> np.uint64(32))
            ex, ez = hit & (typ != 3), hit & (typ != 1)
        flips = (w2[:, :ns] < tm).astype(np.int64)
        if closed and j == T - 1:
            flips[:] = 0
        x ^= ex.astype(np.int64)
        z ^= ez.astype(np.int64)
        grids[:, j] = E.bits_to_grids(d, E.syndrome_bits(d, x, z) ^ flips)
    trivial = (grids.reshape(n, -1).max(axis=1) == 0).astype(np.uint8)
    return grids, E.xz_to_codes(d, x, z), trivial


def gf2_rank(rows):
    """The rank over GF(2) of 0/1 rows [k, m]."""
    words = [sum(int(b) << i for i, b in enumerate(r)) for r in np.asarray(rows).astype(np.int64)]
    rank = 0
    while words:
        p = max(words)
        if p == 0:
            break
        top = p.bit_length() - 1
        words = [x ^ p if (x >> top) & 1 else x for x in words if x != p]
        rank += 1
    return rank


class Stabilizers:
    """Whether a plane of one component is a product of stabilizers: the stabilizers that act on component comp are the plaquettes of the OTHER component,
    whose supports are the columns of its H; membership is a rank comparison, no decoder is asked."""
    _cache = {}

    def __new__(cls, d, comp):
        if (d, comp) not in cls._cache:
            self = super().__new__(cls)
            self.gens = Component(d, 1 - comp).H.T.copy()                              # [n, d2]
            self.rank = gf2_rank(self.gens)
            cls._cache[(d, comp)] = self
        return cls._cache[(d, comp)]

    def trivial(self, plane):
        return gf2_rank(np.vstack([self.gens, np.asarray(plane).reshape(1, -1)])) == self.rank


def fault_rows(d, comp, T, data, meas, closed=True):
    """A fault set of one component: data = [(round, qubit)] errors that stay, meas = [(round, node)] misreadings.  Returns (defect rows int64 [T, n], the
    accumulated error plane int64 [d2], the last syndrome int64 [n])."""
    C = Component(d, comp)
    err = np.zeros((T, d * d), dtype=np.int64)
    for j, q in data:
        err[j:, q] ^= 1
    s = (err @ C.H) & 1
    for j, u in meas:
        assert not (closed and j == T - 1)
        s[j, u] ^= 1
    rows = s.copy()
    rows[1:] ^= s[:-1]
    return rows, err[-1], s[-1]
