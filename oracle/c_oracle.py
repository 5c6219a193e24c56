"""ctypes binding of oracle/env_oracle.c (d <= 7) and oracle/env_oracle_wide.c (any odd 3 <= d <= 15, matching referee).
TEST INFRASTRUCTURE ONLY (see oracle/__init__.py)."""
import ctypes
import glob
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "_build", "libenv_oracle.so")
_lib = None

_u8p = ctypes.POINTER(ctypes.c_uint8)
_u32p = ctypes.POINTER(ctypes.c_uint32)
_u64p = ctypes.POINTER(ctypes.c_uint64)
_i32p = ctypes.POINTER(ctypes.c_int32)
_f32p = ctypes.POINTER(ctypes.c_float)
_i64p = ctypes.POINTER(ctypes.c_int64)


def build(force=False):
    """(Re)build the shared object when it is missing or older than any oracle C source or the Makefile."""
    srcs = glob.glob(os.path.join(_HERE, "*.c")) + [os.path.join(_HERE, "Makefile")]
    if force or not os.path.exists(_SO) or os.path.getmtime(_SO) < max(os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["make", "-s", "-C", _HERE] + (["-B"] if force else []))
    return _SO


def lib():
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(build())
        _lib.dqo_env_create.restype = ctypes.c_void_p
        _lib.dqo_env_create.argtypes = [ctypes.c_int] * 5 + [ctypes.c_uint32] * 3
        _lib.dqo_env_destroy.argtypes = [ctypes.c_void_p]
        _lib.dqo_env_set_rates.argtypes = [ctypes.c_void_p, ctypes.c_double, ctypes.c_double]
        _lib.dqo_env_set_referee.argtypes = [ctypes.c_void_p, _u8p, _u8p]
        _lib.dqo_env_num_actions.argtypes = [ctypes.c_void_p]
        _lib.dqo_env_obs_size.argtypes = [ctypes.c_void_p]
        _lib.dqo_env_reset.argtypes = [ctypes.c_void_p, _u8p, _u8p, _u64p, _u32p]
        _lib.dqo_env_step.argtypes = [ctypes.c_void_p, _i32p, ctypes.c_int, _u8p, _f32p, _u8p, _u64p, _u32p, _u8p]
        _lib.dqo_env_export.argtypes = [ctypes.c_void_p, _u64p, _u64p]
        _lib.dqo_env_poke.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int]
        _lib.dqo_policy_uniform_legal.argtypes = [ctypes.c_void_p, ctypes.c_uint64, _u64p, _i32p]
        _lib.dqo_build_lut.argtypes = [ctypes.c_int, ctypes.c_int, _u8p]
        _lib.dqo_philox.argtypes = [_u32p, _u32p, _u32p]
        # wide environment (env_oracle_wide.c)
        _lib.dqw_match_create.restype = ctypes.c_void_p
        _lib.dqw_match_create.argtypes = [ctypes.c_int]
        _lib.dqw_match_destroy.argtypes = [ctypes.c_void_p]
        _lib.dqw_match_tables.argtypes = [ctypes.c_void_p, ctypes.c_int, _u8p, _u8p, _i32p]
        _lib.dqw_match_classify.argtypes = [ctypes.c_void_p, ctypes.c_int, _u64p, ctypes.c_int, _u8p, _i64p, _u8p]
        _lib.dqw_env_create.restype = ctypes.c_void_p
        _lib.dqw_env_create.argtypes = [ctypes.c_int] * 5 + [ctypes.c_uint32] * 3
        _lib.dqw_env_destroy.argtypes = [ctypes.c_void_p]
        _lib.dqw_env_set_rates.argtypes = [ctypes.c_void_p, ctypes.c_double, ctypes.c_double]
        _lib.dqw_env_set_threads.argtypes = [ctypes.c_void_p, ctypes.c_int]
        for f in ("num_actions", "legal_words", "obs_size", "state_words"):
            getattr(_lib, "dqw_env_" + f).argtypes = [ctypes.c_void_p]
        _lib.dqw_env_reset.argtypes = [ctypes.c_void_p, _u8p, _u8p, _u64p, _u32p]
        _lib.dqw_env_step.argtypes = [ctypes.c_void_p, _i32p, ctypes.c_int, _u8p, _f32p, _u8p, _u64p, _u32p, _u8p, _u8p]
        _lib.dqw_env_export.argtypes = [ctypes.c_void_p, _u64p]
        _lib.dqw_policy_uniform_legal.argtypes = [ctypes.c_void_p, ctypes.c_uint64, _u64p, _i32p]
    return _lib


def _p(a, t):
    return None if a is None else a.ctypes.data_as(t)


def build_lut(d, typ):
    n = (d * d - 1) // 2
    out = np.zeros(1 << n, dtype=np.uint8)
    assert lib().dqo_build_lut(d, typ, _p(out, _u8p)) == 0
    return out


_LUTS = {}


def luts(d):
    if d not in _LUTS:
        _LUTS[d] = (build_lut(d, 3), build_lut(d, 1))
    return _LUTS[d]


class COracleEnv:
    """Batched CPU environment with the same call shape as the product's VectorEnv."""

    def __init__(self, d=5, p_phys=0.01, p_meas=0.01, error_model="DP", use_Y=True, volume_depth=3,
                 n_envs=1, env_id_base=0, seed=(0x5EED, 0xD0DEC0DE), lut=None):
        self.L = lib()
        self.d, self.n_envs, self.depth = d, n_envs, volume_depth
        model = {"X": 0, "DP": 1, "IIDXZ": 2}[error_model]
        self.h = self.L.dqo_env_create(d, model, int(use_Y), volume_depth, n_envs, env_id_base, seed[0], seed[1])
        if not self.h:
            raise ValueError("unsupported configuration")
        self.lut_x, self.lut_z = lut if lut is not None else luts(d)
        self.L.dqo_env_set_referee(self.h, _p(self.lut_x, _u8p), _p(self.lut_z, _u8p))
        self.set_rates(p_phys, p_meas)
        self.num_actions = self.L.dqo_env_num_actions(self.h)
        self.obs_size = self.L.dqo_env_obs_size(self.h)
        n = 2 * d + 1
        self.obs_shape = (self.obs_size // (n * n), n, n)
        self.obs = np.zeros((n_envs,) + self.obs_shape, dtype=np.uint8)
        self.reward = np.zeros(n_envs, dtype=np.float32)
        self.done = np.zeros(n_envs, dtype=np.uint8)
        self.legal = np.zeros((n_envs, 2), dtype=np.uint64)
        self.lifetime = np.zeros(n_envs, dtype=np.uint32)
        self.was_reset = np.zeros(n_envs, dtype=np.uint8)

    def __del__(self):
        if getattr(self, "h", None):
            self.L.dqo_env_destroy(self.h)
            self.h = None

    def set_rates(self, p_phys, p_meas):
        self.L.dqo_env_set_rates(self.h, float(p_phys), float(p_meas))

    def reset(self, which=None):
        w = None if which is None else np.ascontiguousarray(which, dtype=np.uint8)
        self.L.dqo_env_reset(self.h, _p(w, _u8p), _p(self.obs, _u8p), _p(self.legal, _u64p), _p(self.lifetime, _u32p))
        if which is None:
            self.done[:] = 0
        else:
            self.done[w != 0] = 0
        return self.obs

    def step(self, action, auto_reset=False, want_obs=True):
        a = np.ascontiguousarray(action, dtype=np.int32)
        self.L.dqo_env_step(self.h, _p(a, _i32p), int(auto_reset), _p(self.obs if want_obs else None, _u8p),
                            _p(self.reward, _f32p), _p(self.done, _u8p), _p(self.legal, _u64p),
                            _p(self.lifetime, _u32p), _p(self.was_reset, _u8p))
        return self.obs, self.reward, self.done

    def export(self):
        st = np.zeros((self.n_envs, 8), dtype=np.uint64)
        vol = np.zeros((self.n_envs, self.depth), dtype=np.uint64)
        self.L.dqo_env_export(self.h, _p(st, _u64p), _p(vol, _u64p))
        return dict(xmask=st[:, 0], zmask=st[:, 1], true_word=st[:, 2], summed=st[:, 3], acted=st[:, 4],
                    round=st[:, 5], completed=st[:, 6:8], volume=vol)

    def poke(self, i, xmask, zmask, done=0):
        self.L.dqo_env_poke(self.h, i, int(xmask), int(zmask), int(done))

    def policy_uniform_legal(self, t):
        a = np.zeros(self.n_envs, dtype=np.int32)
        self.L.dqo_policy_uniform_legal(self.h, int(t), _p(self.legal, _u64p), _p(a, _i32p))
        return a


class CWideMatch:
    """The C matching referee of one lattice (env_oracle_wide.c; oracle/matching_referee.py restated).  Component 0 = type-3 plaquettes
    (X part), 1 = type-1 plaquettes (Z part); a syndrome is the set of its defects' node indices (the look-up referee's index bits)."""
    CLUSTER_FALLBACK, LIST_FALLBACK = 1, 2

    def __init__(self, d):
        self.L = lib()
        self.d = d
        self.h = self.L.dqw_match_create(d)
        if not self.h:
            raise ValueError("unsupported distance")

    def __del__(self):
        if getattr(self, "h", None):
            self.L.dqw_match_destroy(self.h)
            self.h = None

    def tables(self, comp):
        n = (self.d * self.d - 1) // 2
        dist = np.zeros((n, n, 2), dtype=np.uint8)
        distB = np.zeros((n, 2), dtype=np.uint8)
        w10 = np.zeros(1, dtype=np.int32)
        assert self.L.dqw_match_tables(self.h, comp, _p(dist, _u8p), _p(distB, _u8p), _p(w10, _i32p)) == n
        return dist, distB, int(w10[0])

    def classify_bits(self, comp, bits):
        """bits: uint64 [n, 2] (bit i of a row = node i is a defect) -> (class uint8 [n], (w_0, w_1) int64 [n, 2], fallback flags uint8 [n])"""
        bits = np.ascontiguousarray(bits, dtype=np.uint64).reshape(-1, 2)
        n = bits.shape[0]
        cls, w, fl = np.zeros(n, dtype=np.uint8), np.zeros((n, 2), dtype=np.int64), np.zeros(n, dtype=np.uint8)
        self.L.dqw_match_classify(self.h, comp, _p(bits, _u64p), n, _p(cls, _u8p), _p(w, _i64p), _p(fl, _u8p))
        return cls, w, fl

    def weights(self, comp, defects):
        """(w_0, w_1, exact, flags) of one defect list -- ComponentGraph.weights' answer plus which fallback fired."""
        v = 0
        for i in defects:
            v |= 1 << int(i)
        _, w, fl = self.classify_bits(comp, np.array([[v & (2 ** 64 - 1), v >> 64]], dtype=np.uint64))
        return int(w[0, 0]), int(w[0, 1]), int(fl[0]) == 0, int(fl[0])


class COracleWideEnv:
    """Batched CPU restatement of the wide environment (include/deepq_hip.h dq_envb_*), any odd 3 <= d <= 15: legal sets of legal_words
    uint64 per lattice, the matching referee inside the step (inexact per lattice), export in dq_envb_export_state's layout."""

    def __init__(self, d=9, p_phys=0.01, p_meas=0.01, error_model="DP", use_Y=True, volume_depth=3,
                 n_envs=1, env_id_base=0, seed=(0x5EED, 0xD0DEC0DE), threads=None):
        """threads: worker threads of reset / step (lattices are independent: the results do not depend on it); default
        OMP_NUM_THREADS, else min(16, cpu_count)."""
        self.L = lib()
        self.d, self.n_envs, self.depth = d, n_envs, volume_depth
        model = {"X": 0, "DP": 1, "IIDXZ": 2}[error_model]
        self.h = self.L.dqw_env_create(d, model, int(use_Y), volume_depth, n_envs, env_id_base, seed[0], seed[1])
        if not self.h:
            raise ValueError("unsupported configuration")
        self.set_rates(p_phys, p_meas)
        if threads is None:
            threads = int(os.environ.get("OMP_NUM_THREADS", "0") or 0) or min(16, os.cpu_count() or 1)
        self.L.dqw_env_set_threads(self.h, int(threads))
        self.num_actions = self.L.dqw_env_num_actions(self.h)
        self.legal_words = self.L.dqw_env_legal_words(self.h)
        self.state_words = self.L.dqw_env_state_words(self.h)
        self.W = (d * d + 63) // 64
        obs_size = self.L.dqw_env_obs_size(self.h)
        n = 2 * d + 1
        self.obs_shape = (obs_size // (n * n), n, n)
        self.obs = np.zeros((n_envs,) + self.obs_shape, dtype=np.uint8)
        self.reward = np.zeros(n_envs, dtype=np.float32)
        self.done = np.zeros(n_envs, dtype=np.uint8)
        self.legal = np.zeros((n_envs, self.legal_words), dtype=np.uint64)
        self.lifetime = np.zeros(n_envs, dtype=np.uint32)
        self.was_reset = np.zeros(n_envs, dtype=np.uint8)
        self.inexact = np.zeros(n_envs, dtype=np.uint8)

    def __del__(self):
        if getattr(self, "h", None):
            self.L.dqw_env_destroy(self.h)
            self.h = None

    def set_rates(self, p_phys, p_meas):
        self.L.dqw_env_set_rates(self.h, float(p_phys), float(p_meas))

    def reset(self, which=None):
        w = None if which is None else np.ascontiguousarray(which, dtype=np.uint8)
        self.L.dqw_env_reset(self.h, _p(w, _u8p), _p(self.obs, _u8p), _p(self.legal, _u64p), _p(self.lifetime, _u32p))
        if which is None:
            self.done[:] = 0
        else:
            self.done[w != 0] = 0
        return self.obs

    def step(self, action, auto_reset=False, want_obs=True):
        a = np.ascontiguousarray(action, dtype=np.int32)
        assert a.shape == (self.n_envs,)
        self.L.dqw_env_step(self.h, _p(a, _i32p), int(auto_reset), _p(self.obs if want_obs else None, _u8p),
                            _p(self.reward, _f32p), _p(self.done, _u8p), _p(self.legal, _u64p),
                            _p(self.lifetime, _u32p), _p(self.was_reset, _u8p), _p(self.inexact, _u8p))
        return self.obs, self.reward, self.done

    def export_state(self):
        """uint64 [n_envs, state_words] in dq_envb_export_state's layout."""
        st = np.zeros((self.n_envs, self.state_words), dtype=np.uint64)
        self.L.dqw_env_export(self.h, _p(st, _u64p))
        return st

    def export(self):
        """The export split into named fields; every multi-word set as a Python int."""
        st = self.export_state()
        W, LW = self.W, self.legal_words

        def big(row, lo, n):
            return sum(int(row[lo + k]) << (64 * k) for k in range(n))

        out = []
        for row in st:
            meta = int(row[5 * W + 1 + 2 * LW])
            out.append(dict(xmask=big(row, 0, W), zmask=big(row, W, W), true_word=big(row, 2 * W, W), summed=big(row, 3 * W, W),
                            acted=big(row, 4 * W, W), round=int(row[5 * W]), completed=big(row, 5 * W + 1, LW),
                            legal=big(row, 5 * W + 1 + LW, LW), lifetime=meta & 0xFFFFFFFF, done=meta >> 32,
                            volume=[big(row, 5 * W + 2 + 2 * LW + j * W, W) for j in range(self.depth)]))
        return out

    def policy_uniform_legal(self, t):
        a = np.zeros(self.n_envs, dtype=np.int32)
        self.L.dqw_policy_uniform_legal(self.h, int(t), _p(self.legal, _u64p), _p(a, _i32p))
        return a
