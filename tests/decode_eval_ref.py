"""Numpy restatement of the decode-scoring kernels (include/deepq_hip.h dq_decode_sample / dq_decode_verdict / dq_decode_count; DESIGN.md
section 12), built from the oracle's Philox, lattice masks and referee: the checker of tests/test_decode_eval_cpu.py and
tests/test_decode_eval_gpu.py.  Vectorised over the volumes, so that thousands of them are restated in well under a second."""
import numpy as np

from oracle import lattice, philox

IN_CODESPACE, CLASS_SHIFT, SUCCESS, ALIVE, DECODED_SHIFT = 1, 1, 8, 16, 5


def _stab_matrices(d):
    """(Sx, Sz) uint8 [n_stab, d*d]: membership of qubit q in stabilizer s, split by the component the stabilizer reads (type 3: X, type 1: Z)."""
    m = lattice.Masks(d)
    member = np.array([[(m.stab_qmask[s] >> q) & 1 for q in range(d * d)] for s in range(m.n_stab)], dtype=np.int64)
    isx = np.array([t == 3 for t in m.stab_type])
    return member * isx[:, None], member * (~isx)[:, None]


def syndrome_bits(d, x, z):
    """Perfect syndrome bits int64 [N, n_stab] (measurement order) of X / Z component planes int [N, d*d] (Function_Library.py:152-174)."""
    sx, sz = _stab_matrices(d)
    return (x @ sx.T + z @ sz.T) & 1


def bits_to_grids(d, bits):
    """Syndrome bits [..., n_stab] -> grids uint8 [..., d+1, d+1]."""
    m = lattice.Masks(d)
    out = np.zeros(bits.shape[:-1] + (d + 1, d + 1), dtype=np.uint8)
    for s, (a, b) in enumerate(m.order):
        out[..., a, b] = bits[..., s]
    return out


def codes_to_xz(codes):
    c = np.asarray(codes).astype(np.int64)
    c = c.reshape(c.shape[0], -1)
    return ((c == 1) | (c == 2)).astype(np.int64), ((c == 2) | (c == 3)).astype(np.int64)


def xz_to_codes(d, x, z):
    return np.where(x & z, 2, np.where(x, 1, np.where(z, 3, 0))).astype(np.uint8).reshape(-1, d, d)


def _thresholds(p, n):
    p = np.broadcast_to(np.asarray(p, dtype=np.float64), (n,))
    return np.array([philox.threshold(float(x)) for x in p], dtype=np.uint64)


def sample_volumes(d, error_model, volume_depth, n, p_phys, p_meas, seed, env_id_base=0):
    """Volume i = volume_depth rounds of OracleEnv._draw_round for lattice (env_id_base + i) mod 2^32 from a clean lattice, without the redraw of
    all-zero volumes.  p_phys / p_meas: scalars or one per volume.  Returns (grids uint8 [n, depth, d+1, d+1], hidden codes uint8 [n, d, d],
    trivial uint8 [n])."""
    m = lattice.Masks(d)
    d2, ns = d * d, m.n_stab
    ids = ((int(env_id_base) + np.arange(n, dtype=np.uint64)) & np.uint64(philox.MASK)).astype(np.uint32)
    tp, tm = _thresholds(p_phys, n)[:, None], _thresholds(p_meas, n)[:, None]
    lanes = np.arange(d2, dtype=np.uint32)[None, :]
    x = np.zeros((n, d2), dtype=np.int64)
    z = np.zeros((n, d2), dtype=np.int64)
    grids = np.zeros((n, volume_depth, d + 1, d + 1), dtype=np.uint8)
    for j in range(volume_depth):
        w0, w1, w2, _ = philox.philox4x32_np(np.uint32(j), np.uint32(0), ids[:, None], lanes, seed)
        w0, w1, w2 = w0.astype(np.uint64), w1.astype(np.uint64), w2.astype(np.uint64)
        hit = w0 < tp
        if error_model == "IIDXZ":                              # two uniforms per qubit: X flip, then Z flip
            ex, ez = hit, w1 < tp
        elif error_model == "X":
            ex, ez = hit, np.zeros_like(hit)
        else:
            typ = 1 + ((w1 * np.uint64(3)) >> np.uint64(32))    # philox.pauli_type
            ex, ez = hit & (typ != 3), hit & (typ != 1)
        flips = (w2[:, :ns] < tm).astype(np.int64)
        x ^= ex.astype(np.int64)
        z ^= ez.astype(np.int64)
        grids[:, j] = bits_to_grids(d, syndrome_bits(d, x, z) ^ flips)
    trivial = (grids.reshape(n, -1).max(axis=1) == 0).astype(np.uint8)
    return grids, xz_to_codes(d, x, z), trivial


def bits_to_words(bits):
    """Syndrome bits [N, n_stab] -> python ints (bit s = stabilizer s in measurement order)."""
    return [sum(int(b) << s for s, b in enumerate(row)) for row in np.asarray(bits)]


def classify_with(referee):
    """words -> classes through an oracle referee object (`classify_word`)."""
    return lambda words: np.array([referee.classify_word(w) for w in words], dtype=np.int64)


def classify_with_predict(d, predict):
    """words -> classes through a `.predict`-style function of the flattened (d+1)^2 syndromes (only its arg-max is used)."""
    m = lattice.Masks(d)
    return lambda words: np.argmax(np.asarray(predict(np.stack([m.word_to_grid(w).reshape(-1) for w in words]))), axis=1).astype(np.int64)


def verdict(d, hidden, frame, classify):
    """The verdict bytes uint8 [N] for residual = hidden XOR frame (frame None: no correction); classify(words) -> the referee's classes."""
    m = lattice.Masks(d)
    x, z = codes_to_xz(hidden)
    if frame is not None:
        fx, fz = codes_to_xz(frame)
        x, z = x ^ fx, z ^ fz
    bits = syndrome_bits(d, x, z)
    col0 = np.array([(m.col0_mask >> q) & 1 for q in range(d * d)], dtype=np.int64)
    row0 = np.array([(m.row0_mask >> q) & 1 for q in range(d * d)], dtype=np.int64)
    correct = ((x @ col0) & 1) + 2 * ((z @ row0) & 1)
    decoded = np.asarray(classify(bits_to_words(bits))).astype(np.int64)
    in_code = bits.max(axis=1) == 0
    success = in_code & (correct == 0)
    alive = success | (decoded == correct)
    return (in_code * IN_CODESPACE + (correct << CLASS_SHIFT) + success * SUCCESS + alive * ALIVE + ((decoded & 3) << DECODED_SHIFT)).astype(np.uint8)


def flags(v):
    """(success, alive) boolean arrays of verdict bytes."""
    v = np.asarray(v)
    return (v & SUCCESS) != 0, (v & ALIVE) != 0
