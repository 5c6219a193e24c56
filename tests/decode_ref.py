"""Numpy restatement of the batched decode loop (include/deepq_hip.h dq_decode_run; DESIGN.md "Batched decoding") for one volume, with
the Q-function passed in: the checker of tests/test_decode_cpu.py and tests/test_decode_gpu.py."""
import numpy as np

from oracle import env_oracle as E
from oracle import lattice

IDENTITY, REPEAT, STOPPED = 1, 2, 3


def first_max(q, legal=None):
    """np.argmax (the first maximum), over the sorted legal set when one is given (policy_kernel's rule with eps = 0)."""
    if legal is None:
        return int(np.argmax(q))
    cand = sorted(legal)
    return int(cand[int(np.argmax(np.asarray(q)[cand]))])


def initial_legal(d, grids, layers, identity):
    """reset_legal_moves of the summed volume (Environments.py:238-271)."""
    m = lattice.Masks(d)
    summed = np.asarray(grids).sum(0) != 0
    word = sum(1 << s for s, (a, b) in enumerate(m.order) if summed[a, b])
    legal = {identity}
    for q in range(d * d):
        if m.qubit_smask[q] & word:
            legal |= {q + j * d * d for j in range(layers)}
    return legal


def decode_volume(grids, qfun, d, error_model, use_Y, masked_greedy, max_actions=None, action_planes="environment"):
    """grids int [depth, d+1, d+1]; qfun(obs int [C, 2d+1, 2d+1]) -> Q [num_actions].  Returns (corrections, frame codes [d, d], status)."""
    grids = np.asarray(grids)
    depth, d2 = grids.shape[0], d * d
    num_actions, layers = lattice.num_actions(d, error_model, use_Y)
    identity = num_actions - 1
    max_actions = num_actions - 1 if max_actions is None else max_actions
    m = lattice.Masks(d)
    obs = np.zeros((depth + layers, 2 * d + 1, 2 * d + 1), dtype=np.int64)
    for j in range(depth):
        obs[j] = E.padding_syndrome(d, grids[j])
    legal = initial_legal(d, grids, layers, identity)
    corrections, completed, acted = [], set(), set()
    xm = zm = 0
    while True:
        q = qfun(obs.copy())
        a = first_max(q, legal if masked_greedy else None)
        if a == identity:
            status = IDENTITY
            break
        if a in completed:                                      # Environments.py:131
            status = REPEAT
            break
        corrections.append(a)
        completed.add(a)
        layer, qb = divmod(a, d2)
        if qb not in acted:                                     # Environments.py:190-196
            acted.add(qb)
            for j in range(layers):
                legal |= {nb + j * d2 for nb in range(d2) if (m.neigh_qmask[qb] >> nb) & 1}
        pauli = lattice.layer_pauli(error_model, use_Y, layer)
        if pauli in (1, 2):
            xm ^= 1 << qb
        if pauli in (2, 3):
            zm ^= 1 << qb
        if action_planes == "readme":                           # README.md:807: padding_actions(corrections), the LIST of indices
            obs[depth] = E.padding_actions(d, corrections)
        else:                                                   # Environments.py:199-201
            obs[depth + layer, 2 * (qb // d) + 1, 2 * (qb % d) + 1] = 1
        if len(corrections) >= max_actions:
            status = STOPPED
            break
    return corrections, E.masks_to_codes(d, xm, zm), status


def codes_to_xz(codes):
    c = np.asarray(codes)
    return ((c == 1) | (c == 2)).astype(np.int64), ((c == 2) | (c == 3)).astype(np.int64)


def apply_frame(hidden, frame):
    """hidden_state codes with the frame's Pauli applied (obtain_new_error_configuration: XOR of the components)."""
    hx, hz = codes_to_xz(hidden)
    fx, fz = codes_to_xz(frame)
    x, z = hx ^ fx, hz ^ fz
    return np.where(x & z, 2, np.where(x, 1, np.where(z, 3, 0)))


def state_after(grids, prefix, d, error_model, use_Y, action_planes="environment"):
    """Observation and legal set of the decode loop after the actions `prefix` were recorded (the point where two decodes first differ)."""
    grids = np.asarray(grids)
    depth, d2 = grids.shape[0], d * d
    num_actions, layers = lattice.num_actions(d, error_model, use_Y)
    m = lattice.Masks(d)
    obs = np.zeros((depth + layers, 2 * d + 1, 2 * d + 1), dtype=np.int64)
    for j in range(depth):
        obs[j] = E.padding_syndrome(d, grids[j])
    legal, acted = initial_legal(d, grids, layers, num_actions - 1), set()
    for a in prefix:
        layer, qb = divmod(a, d2)
        if qb not in acted:
            acted.add(qb)
            for j in range(layers):
                legal |= {nb + j * d2 for nb in range(d2) if (m.neigh_qmask[qb] >> nb) & 1}
        if action_planes == "readme":
            obs[depth] = E.padding_actions(d, list(prefix))
        else:
            obs[depth + layer, 2 * (qb // d) + 1, 2 * (qb % d) + 1] = 1
    return obs, legal


def words_to_grids(d, words):
    """Syndrome words (bit s = stabilizer s in measurement order; uint64 [..., depth]) -> grids int [..., depth, d+1, d+1]."""
    m = lattice.Masks(d)
    w = np.asarray(words).astype(np.uint64)
    out = np.zeros(w.shape + (d + 1, d + 1), dtype=np.uint8)
    for s, (a, b) in enumerate(m.order):
        out[..., a, b] = ((w >> np.uint64(s)) & np.uint64(1)).astype(np.uint8)
    return out
