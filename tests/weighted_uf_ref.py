"""Weighted union-find stream decoding (include/deepq_hip.h dq_wide_uf_decode_weighted / dq_wide_uf_run_weighted) in numpy / Python, for
tests/test_weighted_uf_cpu.py and tests/test_weighted_uf_gpu.py.

The graph is closed_uf_ref.graph's: node (u, t) = t n + u, B = depth n, edge ids t (d^2 + n) + k with k = q < d^2 the space edge of qubit q and
k = d^2 + u the time edge (u, t) -- (u, t + 1), in the last round (u, t) -- B; closed, the last round's time edges are dead.  An edge of weight w -- w_space
for k < d^2, w_time for k >= d^2 -- is full when its growth reaches 2 w.  `window_edges` grows in UNIT steps: per step every living edge gains 1 per end
that lies in an active cluster (odd defect parity, B not inside), capped at 2 w; the clusters are merged across the edges that became full, and the
activity is looked up again.  The device jumps from one filling edge to the next; this form does not, and `rounds` counts the unit steps.  Peeling: levels
breadth-first from B and from the lowest node of every other cluster over the full edges, the parent edge of a node the lowest edge id to the level
before, the correction read from the deepest level down.  `stream_component` is section 17's window schedule with W the weighted cost of the committed
edges; one (w_space, w_time) holds for every window and both components of a stream."""
import numpy as np

from closed_uf_ref import MAX_WINDOW, graph, n_windows, sample_streams   # noqa: F401  (the samplers are re-exported for the tests)
from match_st_ref import Component

MAX_WEIGHT = 15


def check_weights(w_space, w_time):
    for w in (w_space, w_time):
        if int(w) != w or not 1 <= int(w) <= MAX_WEIGHT:
            raise ValueError(f"weights must be integers in 1..{MAX_WEIGHT}, not {(w_space, w_time)}")
    return int(w_space), int(w_time)


def edge_weights(d, depth, w_space, w_time):
    """int64 [NE]: the weight of every edge id of a window of `depth` rounds."""
    d2 = d * d
    per_round = d2 + (d2 - 1) // 2
    return np.where(np.arange(depth * per_round) % per_round < d2, w_space, w_time).astype(np.int64)


def _find(up, x):
    while up[x] != x:
        up[x] = up[up[x]]
        x = up[x]
    return x


def window_edges(d, comp, rows, depth, closed, w_space, w_time):
    """rows: 0/1 [depth, n] defects of one window.  Returns (the correction's edge ids, ascending; unit growth steps)."""
    ea, eb, alive, B = graph(d, comp, depth, closed)
    NE = len(ea)
    cap = 2 * edge_weights(d, depth, w_space, w_time)
    defect = np.zeros(B + 1, dtype=np.int64)
    defect[:B] = np.asarray(rows).reshape(-1) != 0
    if not defect.any():
        return [], 0
    up = list(range(B + 1))                                                            # a union-find forest over the nodes, B among them
    g = np.zeros(NE, dtype=np.int64)
    steps, act = 0, None
    while True:
        if act is None:                                                                # the clusters moved: look the activity up again
            root = np.array([_find(up, x) for x in range(B + 1)])
            odd = np.bincount(root, weights=defect, minlength=B + 1).astype(np.int64) & 1
            odd[root[B]] = 0
            act = odd[root]
            if not act.any():
                break
        assert steps < int(cap.sum()) + 1
        steps += 1
        g1 = np.where(alive, np.minimum(cap, g + act[ea] + act[eb]), 0)
        assert (g1 != g).any()                                                         # an active cluster always has a living edge that is not full
        filled = np.flatnonzero((g1 == cap) & (g != cap) & alive)
        g = g1
        for e in filled:
            a, b = _find(up, int(ea[e])), _find(up, int(eb[e]))
            if a != b:
                up[a] = b
        if len(filled):
            act = None
    full = np.flatnonzero((g == cap) & alive)                                          # ascending edge ids
    root = np.array([_find(up, x) for x in range(B + 1)])
    touched = np.zeros(B + 1, dtype=bool)
    touched[ea[full]] = touched[eb[full]] = True
    touched |= defect != 0
    level = np.full(B + 1, -1, dtype=np.int64)
    level[B] = 0
    seen_root = {int(root[B])}
    for x in np.flatnonzero(touched):                                                  # ascending: the first node met of a cluster is its lowest
        if int(root[x]) not in seen_root:
            seen_root.add(int(root[x]))
            level[x] = 0
    parent = np.full(B + 1, -1, dtype=np.int64)
    lev = 0
    while True:
        lev += 1
        reached = False
        for e in full:                                                                 # ascending: the first edge that reaches a node is its lowest
            a, b = int(ea[e]), int(eb[e])
            for x, y in ((a, b), (b, a)):
                if level[x] == lev - 1 and level[y] == -1 and parent[y] == -1:
                    parent[y] = e
                    reached = True
        level[(level == -1) & (parent != -1)] = lev
        if not reached:
            break
    par = defect.copy()
    correction = []
    for l in range(lev - 1, 0, -1):
        for y in np.flatnonzero(level == l):
            if par[y] & 1:
                e = int(parent[y])
                correction.append(e)
                par[int(ea[e]) if int(eb[e]) == y else int(eb[e])] ^= 1
    assert (level[defect != 0] >= 0).all()                                             # every defect hangs on a root
    assert all(x == B or par[x] % 2 == 0 for x in np.flatnonzero(level == 0))          # every root but B ends even
    return sorted(correction), steps


def stream_component(d, comp, rows, w, c, closed, w_space, w_time):
    """rows: 0/1 [T, n] defects of one stream's component.  Returns dict(M: a Python integer, bit q = qubit q; W: the weighted cost of the committed edges;
    ndef, rounds, windows)."""
    rows = np.asarray(rows).astype(np.int64)
    T, n = rows.shape
    T, w, c = int(T), int(w), int(c)
    w_space, w_time = check_weights(w_space, w_time)
    if not (T >= 1 and 1 <= w <= MAX_WINDOW and 1 <= c <= w):
        raise ValueError(f"stream schedule: T = {T} >= 1, 1 <= window = {w} <= {MAX_WINDOW}, 1 <= commit = {c} <= window")
    d2 = d * d
    per_round = d2 + n
    carry = np.zeros(n, dtype=np.int64)
    M = W = rounds = windows = 0
    a = 0
    while True:
        final = a + w >= T
        l = T - a if final else w
        win = rows[a:a + l].copy()
        win[0] ^= carry
        edges, r = window_edges(d, comp, win, l, closed and final, w_space, w_time)
        rounds += r
        windows += 1
        carry = np.zeros(n, dtype=np.int64)
        for e in edges:
            t, k = divmod(int(e), per_round)
            if not final and t >= c:
                continue
            if k < d2:
                W += w_space
                M ^= 1 << k
            else:
                W += w_time
                if not final and t == c - 1:
                    carry[k - d2] = 1
        if final:
            break
        a += c
    assert windows == n_windows(T, w, c)
    return dict(M=M, W=W, ndef=int(rows.sum()), rounds=rounds, windows=windows)


def decode(d, syndromes, w, c, closed, weights):
    """syndromes uint8 [N, T, d+1, d+1]; weights: a pair (w_space, w_time) or an integer array [N, 2] -> (frame uint8 [N, d, d] hidden_state codes, weight,
    n_defects, rounds: int32 [N, 2], windows)."""
    v = np.asarray(syndromes)
    N, d2 = len(v), d * d
    pairs = [check_weights(*pr) for pr in np.broadcast_to(np.asarray(weights).reshape(-1, 2), (N, 2))]
    planes = np.zeros((N, 2, d2), dtype=np.int64)
    out = np.zeros((N, 2, 3), dtype=np.int64)
    for comp in range(2):
        rows = Component(d, comp).defects(v)
        for i in range(N):
            r = stream_component(d, comp, rows[i], w, c, closed, *pairs[i])
            planes[i, comp] = [(r["M"] >> q) & 1 for q in range(d2)]
            out[i, comp] = r["W"], r["ndef"], r["rounds"]
    x, z = planes[:, 0], planes[:, 1]
    frame = np.where(x & z, 2, np.where(x, 1, np.where(z, 3, 0))).astype(np.uint8).reshape(N, d, d)
    return frame, out[:, :, 0].astype(np.int32), out[:, :, 1].astype(np.int32), out[:, :, 2].astype(np.int32), n_windows(v.shape[1], w, c)
