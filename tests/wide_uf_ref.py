"""The wide sliding-window union-find decoder (include/deepq_hip.h dq_wide_uf_*) in numpy / Python, for tests/test_wide_uf_cpu.py and
tests/test_wide_uf_gpu.py: section 17's window schedule restated on top of stream_uf_ref.window_edges with Python integers for M and the carry, for any odd
d and a window of up to 32 rounds (stream_uf_ref.decode packs M into int64 and its check_schedule stops at 16)."""
import numpy as np

from match_st_ref import Component
from stream_uf_ref import n_windows, window_edges

MAX_WINDOW = 32


def check_schedule(T, w, c):
    if not (T >= 1 and 1 <= w <= MAX_WINDOW and 1 <= c <= w):
        raise ValueError(f"stream schedule: T = {T} >= 1, 1 <= window = {w} <= {MAX_WINDOW}, 1 <= commit = {c} <= window")


def stream_component(d, comp, rows, w, c):
    """rows: 0/1 [T, n] defects of one stream's component.  Returns dict(M: a Python integer, bit q = qubit q; W, ndef, rounds, windows, last: the 0/1 [n]
    set of nodes whose last-round time edge to B the final window committed)."""
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


def decode(d, syndromes, w, c):
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
            r = stream_component(d, comp, rows[i], w, c)
            planes[i, comp] = [(r["M"] >> q) & 1 for q in range(d2)]
            out[i, comp] = r["W"], r["ndef"], r["rounds"]
            ls[i] = r["last"]
        last.append(ls)
    x, z = planes[:, 0], planes[:, 1]
    frame = np.where(x & z, 2, np.where(x, 1, np.where(z, 3, 0))).astype(np.uint8).reshape(N, d, d)
    return frame, out[:, :, 0].astype(np.int32), out[:, :, 1].astype(np.int32), out[:, :, 2].astype(np.int32), n_windows(v.shape[1], w, c), last


def classify_none(words):
    """decode_eval_ref.verdict's `classify` of the wide verdict: no referee is consulted; 4 sets no bit of the decoded field and equals no class."""
    return np.full(len(words), 4, dtype=np.int64)


def node_syndromes(d, comp, node_bits):
    """0/1 [N, T, n] syndrome bits per node of one component -> grids uint8 [N, T, d+1, d+1] with every other cell 0."""
    C = Component(d, comp)
    b = np.asarray(node_bits)
    out = np.zeros(b.shape[:2] + (d + 1, d + 1), dtype=np.uint8)
    for j, (a, bb) in enumerate(C.cells):
        out[:, :, a, bb] = b[:, :, j]
    return out
