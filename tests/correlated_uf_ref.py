"""Correlated union-find stream decoding (include/deepq_hip.h dq_wide_uf_decode_correlated / dq_wide_uf_run_correlated) in numpy /
Python, for tests/test_correlated_uf_cpu.py and tests/test_correlated_uf_gpu.py.

The graph is closed_uf_ref.graph's: node (u, t) = t n + u, B = depth n, edge ids t (d^2 + n) + k with k = q < d^2 the space edge of qubit q and
k = d^2 + u the time edge; closed, the last round's time edges are dead.  `window_edges` is the weighted decode of one window with ONE WEIGHT PER EDGE: an
edge of weight w is full when its growth reaches 2 w, growth goes in UNIT steps (every living edge gains 1 per end in an active cluster, capped), peeling
takes the lowest edge id to the level before.  The device jumps from one filling edge to the next; this form does not.

`stream` is the rule of section 25 for one stream, per window, inside section 17's schedule:
  pass 0  component 0 on the window's rows (carry applied) with (w_space, w_time), dry: nothing is committed; mask A = the space edges (t, q) of its
          correction, every round of the window, committed or not
  pass 1  component 1; a space edge weighs w_corr where A has it, else w_space; committed (frame, carry, weight = the sum of the weights used, rounds);
          mask B = the space edges of its whole correction
  pass 2  component 0 on pass 0's rows with B in A's place, committed
`rounds` and `weight` count passes 1 and 2."""
import numpy as np

from closed_uf_ref import MAX_WINDOW, graph, n_windows, sample_streams   # noqa: F401  (the samplers are re-exported for the tests)
from match_st_ref import Component

MAX_WEIGHT = 15


def check_weights(w_space, w_time, w_corr):
    for w in (w_space, w_time, w_corr):
        if int(w) != w or not 1 <= int(w) <= MAX_WEIGHT:
            raise ValueError(f"weights must be integers in 1..{MAX_WEIGHT}, not {(w_space, w_time, w_corr)}")
    if int(w_corr) > int(w_space):
        raise ValueError(f"w_corr = {w_corr} must not exceed w_space = {w_space}")
    return int(w_space), int(w_time), int(w_corr)


def edge_weights(d, depth, w_space, w_time, w_corr=None, mask=None):
    """int64 [NE]: the weight of every edge id of a window of `depth` rounds; mask: 0/1 [depth, d^2], the space edges that weigh w_corr."""
    d2 = d * d
    n = (d2 - 1) // 2
    w = np.empty((depth, d2 + n), dtype=np.int64)
    w[:, :d2] = w_space
    w[:, d2:] = w_time
    if mask is not None:
        w[:, :d2][np.asarray(mask)[:depth] != 0] = w_corr
    return w.reshape(-1)


def _find(up, x):
    while up[x] != x:
        up[x] = up[up[x]]
        x = up[x]
    return x


def window_edges(d, comp, rows, depth, closed, weight):
    """rows: 0/1 [depth, n] defects of one window; weight: int [NE] per edge.  Returns (the correction's edge ids, ascending; unit growth steps)."""
    ea, eb, alive, B = graph(d, comp, depth, closed)
    NE = len(ea)
    cap = 2 * np.asarray(weight, dtype=np.int64)
    assert cap.shape == (NE,) and cap.min() >= 2
    defect = np.zeros(B + 1, dtype=np.int64)
    defect[:B] = np.asarray(rows).reshape(-1) != 0
    if not defect.any():
        return [], 0
    up = list(range(B + 1))
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
        steps += 1                                                                     # one UNIT step
        g1 = np.where(alive, np.minimum(cap, g + act[ea] + act[eb]), 0)
        assert (g1 != g).any()
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
    assert (level[defect != 0] >= 0).all()
    assert all(x == B or par[x] % 2 == 0 for x in np.flatnonzero(level == 0))
    return sorted(correction), steps


def space_mask(d, depth, edges):
    """0/1 [depth, d^2]: the space edges among the edge ids."""
    d2 = d * d
    per_round = d2 + (d2 - 1) // 2
    m = np.zeros((depth, d2), dtype=np.int64)
    for e in edges:
        t, k = divmod(int(e), per_round)
        if k < d2:
            m[t, k] = 1
    return m


def stream(d, rows0, rows1, w, c, closed, w_space, w_time, w_corr):
    """rows0, rows1: 0/1 [T, n] defects of one stream's two components.  Returns a list of two dict(M: a Python integer, bit q = qubit q; W: the weighted
    cost of the committed edges; ndef, rounds, windows), one per component."""
    rows = [np.asarray(rows0).astype(np.int64), np.asarray(rows1).astype(np.int64)]
    T, n = rows[0].shape
    T, w, c = int(T), int(w), int(c)
    w_space, w_time, w_corr = check_weights(w_space, w_time, w_corr)
    if not (T >= 1 and 1 <= w <= MAX_WINDOW and 1 <= c <= w):
        raise ValueError(f"stream schedule: T = {T} >= 1, 1 <= window = {w} <= {MAX_WINDOW}, 1 <= commit = {c} <= window")
    d2 = d * d
    per_round = d2 + n
    carry = [np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)]
    out = [dict(M=0, W=0, ndef=int(rows[k].sum()), rounds=0, windows=0) for k in range(2)]
    a = 0
    while True:
        final = a + w >= T
        l = T - a if final else w
        win = []
        for k in range(2):
            x = rows[k][a:a + l].copy()
            x[0] ^= carry[k]
            win.append(x)
        carry = [np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)]

        def commit(k, edges, weight, steps):
            r = out[k]
            r["rounds"] += steps
            for e in edges:
                t, kk = divmod(int(e), per_round)
                if not final and t >= c:
                    continue
                r["W"] += int(weight[e])
                if kk < d2:
                    r["M"] ^= 1 << kk
                elif not final and t == c - 1:
                    carry[k][kk - d2] = 1

        # pass 0: component 0, dry
        edges, _ = window_edges(d, 0, win[0], l, closed and final, edge_weights(d, l, w_space, w_time))
        A = space_mask(d, l, edges)
        # pass 1: component 1 under A
        weight = edge_weights(d, l, w_space, w_time, w_corr, A)
        edges, steps = window_edges(d, 1, win[1], l, closed and final, weight)
        commit(1, edges, weight, steps)
        B = space_mask(d, l, edges)
        # pass 2: component 0 under B
        weight = edge_weights(d, l, w_space, w_time, w_corr, B)
        edges, steps = window_edges(d, 0, win[0], l, closed and final, weight)
        commit(0, edges, weight, steps)
        for k in range(2):
            out[k]["windows"] += 1
        if final:
            break
        a += c
    assert out[0]["windows"] == n_windows(T, w, c)
    return out


def decode(d, syndromes, w, c, closed, weights):
    """syndromes uint8 [N, T, d+1, d+1]; weights: a triple (w_space, w_time, w_corr) or an integer array [N, 3] -> (frame uint8 [N, d, d] hidden_state
    codes, weight, n_defects, rounds: int32 [N, 2], windows)."""
    v = np.asarray(syndromes)
    N, d2 = len(v), d * d
    triples = [check_weights(*tr) for tr in np.broadcast_to(np.asarray(weights).reshape(-1, 3), (N, 3))]
    rows = [Component(d, comp).defects(v) for comp in range(2)]
    planes = np.zeros((N, 2, d2), dtype=np.int64)
    out = np.zeros((N, 2, 3), dtype=np.int64)
    for i in range(N):
        res = stream(d, rows[0][i], rows[1][i], w, c, closed, *triples[i])
        for comp, r in enumerate(res):
            planes[i, comp] = [(r["M"] >> q) & 1 for q in range(d2)]
            out[i, comp] = r["W"], r["ndef"], r["rounds"]
    x, z = planes[:, 0], planes[:, 1]
    frame = np.where(x & z, 2, np.where(x, 1, np.where(z, 3, 0))).astype(np.uint8).reshape(N, d, d)
    return frame, out[:, :, 0].astype(np.int32), out[:, :, 1].astype(np.int32), out[:, :, 2].astype(np.int32), n_windows(v.shape[1], w, c)


def failures(d, hidden, frame):
    """bool [N, 2]: per component, whether the residual hidden XOR frame has a syndrome or a non-trivial class (closed streams: a logical failure)."""
    out = np.zeros((len(hidden), 2), dtype=bool)
    for comp in range(2):
        C = Component(d, comp)
        res = C.plane(hidden) ^ C.plane(frame)
        out[:, comp] = ((res @ C.H) & 1).any(axis=1) | (((res @ C.logical) & 1) != 0)
    return out
