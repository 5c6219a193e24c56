"""Helpers of tests/test_decode_wide_cpu.py and tests/test_decode_wide_gpu.py: the action-plane-sensitive network, the supplied Q
rows of the stepping test, and the numpy readers of the multi-word state.  The restatement of the loop itself is tests/decode_ref.py, which is d-generic."""
import numpy as np

import architectures as AR
import decode_ref as R
from oracle import dqn_oracle as O
from oracle import lattice

C_LAYERS, FF_LAYERS = AR.REF_CONV, AR.REF_FF
PLANE_GAIN = 30.0                     # a Glorot network's argmax barely depends on the one action-plane cell a step changes: without the gain almost every
IDENTITY_QUANTILE = 0.10              # volume ends as a repeat after one action; the identity's shift lets 10 % of the volumes stop at once


def spec_of(cfg):
    A, layers = lattice.num_actions(cfg["d"], cfg["error_model"], cfg["use_Y"])
    n = 2 * cfg["d"] + 1
    return O.QNetSpec((cfg["volume_depth"] + layers, n, n), C_LAYERS, FF_LAYERS, A)


def initial_observations(cfg, grids):
    return np.stack([R.state_after(g, [], cfg["d"], cfg["error_model"], cfg["use_Y"])[0] for g in grids])


def sensitive_network(cfg, grids, input_seed=5):
    """Flat float32 parameters: architectures.make_inputs' weights with the action-plane input channels of the first convolution multiplied by PLANE_GAIN
    and the identity's advantage bias raised by the IDENTITY_QUANTILE quantile, over `grids`, of (max Q - Q_identity) at the first forward."""
    spec = spec_of(cfg)
    flat, _, _ = AR.make_inputs(spec, 1, input_seed)
    flat = np.ascontiguousarray(flat, dtype=np.float32)
    w0 = spec.split(flat)[0][0]                                       # (k, k, cin, cout), a view of flat
    assert np.shares_memory(w0, flat)
    w0[:, :, cfg["volume_depth"]:, :] *= PLANE_GAIN
    q = O.forward(spec, flat, initial_observations(cfg, grids))[0]
    flat[-1] += np.float32(np.quantile(q.max(axis=1) - q[:, -1], IDENTITY_QUANTILE))   # the dueling head's last column is the identity's advantage
    return spec, flat


def weights_of(spec, flat):
    """The Keras-order list [kernel, bias, ...] of flat parameters (what ConvQModel.set_weights takes)."""
    return [x.copy() for pair in spec.split(np.asarray(flat, dtype=np.float32)) for x in pair]


def sparse_grids(cfg, n, seed, density=0.02):
    """n volumes with a few live cells anywhere on the (d+1)^2 grid (cells that carry no stabilizer included: the embedding copies them, the legal set
    ignores them); volume 0 is empty and volume 1 has every cell of its last slice set (all grid words full)."""
    d, depth = cfg["d"], cfg["volume_depth"]
    g = (np.random.default_rng(seed).random((n, depth, d + 1, d + 1)) < density).astype(np.uint8)
    g[0] = 0
    g[1, -1] = 1
    return g


class SuppliedQ:
    """Q rows per (volume, iteration), seeded and quantised to multiples of 1/8 so that exact ties occur.  Even volumes prefer a small pool of actions of
    their own (they soon repeat one), odd volumes draw over all actions (they run into max_actions); now and then the identity is raised above everything."""

    def __init__(self, n, n_actions, seed, identity_rate=0.03):
        self.n, self.A, self.seed, self.identity_rate = n, n_actions, seed, identity_rate
        rng = np.random.default_rng([seed, 1 << 20])
        self.pool = np.zeros((n, n_actions), dtype=bool)
        for v in range(0, n, 2):
            self.pool[v, rng.choice(n_actions - 1, size=int(rng.integers(6, 30)), replace=False)] = True
        self._rows = {}

    def rows(self, k):
        """float32 [n, n_actions]: every volume's Q row of iteration k."""
        if k not in self._rows:
            rng = np.random.default_rng([self.seed, k])
            q = rng.integers(0, 32, size=(self.n, self.A)).astype(np.float32) / 8.0
            q[self.pool] += 4.0
            q[rng.random(self.n) < self.identity_rate, self.A - 1] = 9.0
            self._rows[k] = q
        return self._rows[k]

    def qfun(self, v):
        """The Q function decode_ref.decode_volume calls once per iteration for volume v."""
        calls = [0]

        def q(obs):
            calls[0] += 1
            return self.rows(calls[0] - 1)[v]
        return q


def reference_decode(cfg, grids, supplied, masked, max_actions):
    """decode_ref.decode_volume per volume under the supplied Q rows: (correction lists, frames [n, d, d], statuses [n])."""
    out = [R.decode_volume(g, supplied.qfun(v), cfg["d"], cfg["error_model"], cfg["use_Y"], masked, max_actions=max_actions) for v, g in enumerate(grids)]
    return [o[0] for o in out], np.stack([o[1] for o in out]), np.asarray([o[2] for o in out])


def words_to_sets(words):
    """int64 / uint64 [n, LW] -> a list of sets of action indices (bit a of the set = action a)."""
    w = np.ascontiguousarray(np.asarray(words)).astype(np.int64, copy=False).view(np.uint64)
    return [{64 * k + b for k in range(w.shape[1]) for b in range(64) if (int(w[i, k]) >> b) & 1} for i in range(w.shape[0])]


def lists(res):
    return [list(map(int, res.corrections[i, :res.n_corrections[i]])) for i in range(len(res.n_corrections))]
