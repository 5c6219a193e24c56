"""The sliding-window union-find decoder (include/deepq_hip.h dq_stream_decode_uf / dq_stream_run_uf) in numpy / Python, for
tests/test_stream_uf_cpu.py and tests/test_stream_uf_gpu.py.

`window_edges` is a second statement of section 16's component decode (union_find_ref.decode_component states the first) that returns the
correction's EDGES: the same graph, the same synchronous growth, the same lowest-edge-id peeling.  It keeps the clusters in a parent array resolved by
pointer jumping, so that a growth round is a few vector operations and only the newly full edges are visited one by one.

`stream_component` is the window schedule.  The stream's defects are D_t = S_t xor S_{t-1} (S_-1 = 0), t = 0 .. T - 1; window k starts at round
a = k c, is final iff a + w >= T, and has l = T - a rounds when final, else w.  Its defect rows are D_a xor carry, D_{a+1}, ..., D_{a+l-1}; it is decoded on
the depth-l graph.  With t = e // (d^2 + n) the round of an edge: the final window commits every edge of its correction and carries nothing; any other
window commits the edges with t < c, and the new carry is the set of u whose time edge of round c - 1 is in the correction (for c = w that edge is
(u, w - 1) -- B).  A committed space edge XORs its qubit into M, every committed edge adds 1 to W."""
import numpy as np

from match_st_ref import Component
from union_find_ref import Graph


def _roots(up):
    while True:
        nxt = up[up]
        if np.array_equal(nxt, up):
            return up
        up = nxt


def window_edges(d, comp, rows, depth):
    """rows: 0/1 [depth, n] defects of one window.  Returns (the correction's edge ids, ascending; growth rounds)."""
    G = Graph(d, comp, depth)
    B, ends = G.B, G.ends
    defect = np.zeros(B + 1, dtype=bool)
    defect[:B] = np.asarray(rows).reshape(-1) != 0
    if not defect.any():
        return [], 0
    ea, eb = ends[:, 0], ends[:, 1]
    up = np.arange(B + 1)
    g = np.zeros(len(ends), dtype=np.int64)
    rounds = 0
    while True:
        up = _roots(up)
        odd = (np.bincount(up[defect], minlength=B + 1) & 1).astype(bool)
        odd[up[B]] = False                                                             # a cluster that holds B is never active
        act = odd[up]
        if not act.any():
            break
        assert rounds < G.bound
        rounds += 1
        g1 = np.minimum(2, g + act[ea] + act[eb])
        fresh = np.flatnonzero((g1 == 2) & (g != 2))
        assert (g1 != g).any()                                                         # an active cluster always has an edge that is not full
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
    full = np.flatnonzero(g == 2)
    adj = {}
    for e in full:                                                                     # ascending edge ids
        a, b = int(ea[e]), int(eb[e])
        adj.setdefault(a, []).append((int(e), b))
        adj.setdefault(b, []).append((int(e), a))
    touched = sorted(adj)
    root_of_B = int(up[B])
    lowest = {}
    for x in touched:                                                                  # (an untouched node is a root of its own: no defect, no edge)
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
    return sorted(correction), rounds


def n_windows(T, w, c):
    return 1 if w >= T else -(-(T - w) // c) + 1


def check_schedule(T, w, c):
    if not (T >= 1 and 1 <= w <= 16 and 1 <= c <= w):
        raise ValueError(f"stream schedule: T = {T} >= 1, 1 <= window = {w} <= 16, 1 <= commit = {c} <= window")


def stream_component(d, comp, rows, w, c):
    """rows: 0/1 [T, n] defects of one stream's component.  Returns dict(M, W, ndef, rounds, windows, last): last = the 0/1 [n] set of nodes whose last-round
    time edge to B the final window committed."""
    rows = np.asarray(rows).astype(np.int64)
    T, n = rows.shape
    check_schedule(T, w, c)
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
        edges, r = window_edges(d, comp, win, l)
        rounds += r
        windows += 1
        carry = np.zeros(n, dtype=np.int64)
        for e in edges:
            t, k = divmod(e, per_round)
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


def decode(d, syndromes, w, c):
    """syndromes uint8 [N, T, d+1, d+1] -> (frame uint8 [N, d, d] hidden_state codes, weight, n_defects, rounds: int32 [N, 2], windows, last: a list of two
    0/1 arrays [N, n] per component)."""
    v = np.asarray(syndromes)
    N, d2 = len(v), d * d
    out = np.zeros((N, 2, 4), dtype=np.int64)
    last = []
    windows = n_windows(v.shape[1], w, c)
    for comp in range(2):
        rows = Component(d, comp).defects(v)
        ls = np.zeros((N, rows.shape[2]), dtype=np.int64)
        for i in range(N):
            r = stream_component(d, comp, rows[i], w, c)
            out[i, comp] = r["M"], r["W"], r["ndef"], r["rounds"]
            ls[i] = r["last"]
        last.append(ls)
    q = np.arange(d2, dtype=np.int64)
    x, z = (out[:, 0, 0, None] >> q) & 1, (out[:, 1, 0, None] >> q) & 1
    frame = np.where(x & z, 2, np.where(x, 1, np.where(z, 3, 0))).astype(np.uint8).reshape(N, d, d)
    return frame, out[:, :, 1].astype(np.int32), out[:, :, 2].astype(np.int32), out[:, :, 3].astype(np.int32), windows, last


def sample_component_rows(d, comp, T, p, rng, model="DP"):
    """Defect rows int [T, n] of one component of a sampled stream (data errors accumulate, measurement faults do not): for the restatement's own tests."""
    C = Component(d, comp)
    rate = 2 * p / 3 if model == "DP" else (p if comp == 0 else 0.0)                   # depolarising: two of the three Paulis flip a component
    data = rng.random((T, d * d)) < rate
    meas = rng.random((T, C.n)) < p
    s = (((np.cumsum(data, axis=0) % 2) @ C.H) % 2) ^ meas
    rows = s.copy()
    rows[1:] ^= s[:-1]
    return rows.astype(np.int64), s.astype(np.int64)
