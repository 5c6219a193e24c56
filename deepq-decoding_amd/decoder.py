"""Batched on-device decoding of faulty syndrome volumes by a trained agent (include/deepq_hip.h dq_decode_*).

The reference's production use of a trained decoder (README.md:786-829, notebook 3 section 3b) is a Python loop over one volume:

    corrections = []
    while still_decoding:
        action = dqn.forward(input_state)
        if action not in corrections and action != identity: corrections.append(action); update the action plane
        else: still_decoding = False

`BatchDecoder` runs that loop for N volumes at once on the device: one fused forward per iteration over the volumes still decoding, the
greedy choice, the environment's bookkeeping and the action-plane update in HIP kernels (csrc/decode.hip).  Semantics (DESIGN.md
"Batched decoding"): per volume the decode sequence is the sequence of actions a greedy agent takes in the environment on that volume up
to its first identity (or repeated action, which the environment treats as the identity, Environments.py:131).

`action_planes="environment"` marks the acted-on qubit of the action's layer, as Environments.py:199-201 does.  `action_planes="readme"`
(X model only) reproduces the README's `padding_actions(corrections)` call with the LIST of action indices: qubit i is marked iff
corrections[i] != 0 ([21] marks qubit 0).  Both readings are kept as they are.
"""
import ctypes
import math

import numpy as np

STATUS_IDENTITY, STATUS_REPEAT, STATUS_STOPPED = 1, 2, 3          # include/deepq_hip.h DQ_DECODE_*
STATUS_NAMES = {STATUS_IDENTITY: "identity", STATUS_REPEAT: "repeat", STATUS_STOPPED: "stopped"}
PLANES = {"environment": 0, "readme": 1}
OBS_FORMS = {"uint8": 0, "patch": 1}
MODELS = {"X": 0, "DP": 1, "IIDXZ": 2}
DEFAULT_CHUNK = 65536
METHODS = ("matching", "union_find")                             # the baseline decoders: DESIGN.md sections 13 and 16


def check_method(method, who="method"):
    """The baseline decoder's name, validated before any library call."""
    if not isinstance(method, str) or method not in METHODS:
        raise ValueError(f"{who} must be one of {METHODS}, not {method!r}")
    return method


def is_int(x):
    """An integer of Python or numpy that is not a boolean."""
    return isinstance(x, (int, np.integer)) and not isinstance(x, (bool, np.bool_))


def check_positive(x, name):
    if not is_int(x) or x < 1:
        raise ValueError(f"{name} must be a positive integer, not {x!r}")
    return int(x)


def check_chunk(chunk):
    return check_positive(chunk, "chunk")


def action_layers(error_model, use_Y):
    """n_action_layers of Environments.py:55-65 (num_actions = layers d^2 + 1)."""
    if error_model == "X":
        return 1
    if error_model in ("DP", "IIDXZ"):
        return 3 if use_Y else 2
    raise ValueError(f"error model {error_model!r} is not one of X, DP, IIDXZ")


def lattice_of(env):
    """(d, error_model, use_Y, volume_depth) of an environment: the drop-in class, a VectorEnv, or any object with those attributes."""
    v = getattr(env, "_v", env)
    return int(v.d), str(v.error_model), bool(v.use_Y), int(v.volume_depth)


def check_decode_args(d, error_model, use_Y, volume_depth, shape, action_planes="environment", max_actions=None, obs_form=None):
    """Validates a decode request without touching the library.  Returns (n_volumes, single, num_actions, max_actions).
    `shape`: the shape of the syndrome input, [N, depth, d+1, d+1] or one volume [depth, d+1, d+1]."""
    d, volume_depth = int(d), int(volume_depth)
    if d < 3 or d % 2 == 0:
        raise ValueError(f"d = {d}: the surface code lattices have odd d >= 3")
    layers = action_layers(error_model, use_Y)
    num_actions = layers * d * d + 1
    if d > 7 or num_actions > 128:
        raise NotImplementedError(f"decode covers the one-wavefront lattices, d <= 7 and at most 128 actions (d = {d}: {num_actions} actions)")
    if action_planes not in PLANES:
        raise ValueError(f"action_planes must be one of {sorted(PLANES)}, not {action_planes!r}")
    if action_planes == "readme" and layers != 1:
        raise ValueError("action_planes='readme' reproduces the README loop of the X model's single action layer; "
                         f"the {error_model} model has {layers} action layers")
    if obs_form is not None and obs_form not in OBS_FORMS:
        raise ValueError(f"obs_form must be one of {sorted(OBS_FORMS)} or None, not {obs_form!r}")
    if max_actions is None:
        max_actions = num_actions - 1
    max_actions = int(max_actions)
    if not 1 <= max_actions <= num_actions - 1:
        raise ValueError(f"max_actions must be in 1..{num_actions - 1}")
    shape = tuple(int(x) for x in shape)
    grid = (volume_depth, d + 1, d + 1)
    if len(shape) == 3 and shape == grid:
        return 1, True, num_actions, max_actions
    if len(shape) == 4 and shape[1:] == grid and shape[0] >= 1:
        return shape[0], False, num_actions, max_actions
    raise ValueError(f"faulty syndromes must have shape [N, {volume_depth}, {d + 1}, {d + 1}] or [{volume_depth}, {d + 1}, {d + 1}], got {shape}")


def check_binary(x):
    """Raises ValueError unless every cell is 0 or 1 (numpy or torch, on any device)."""
    if hasattr(x, "is_cuda") or type(x).__module__.startswith("torch"):
        bad = bool(((x != 0) & (x != 1)).any().item())
    else:
        a = np.asarray(x)
        if a.dtype.kind not in "biuf":
            raise ValueError(f"faulty syndromes must be numeric, got dtype {a.dtype}")
        bad = bool(((a != 0) & (a != 1)).any())
    if bad:
        raise ValueError("faulty syndrome cells must be 0 or 1")


# ---- scoring a decode: sample -> decode -> verdict -> counts (include/deepq_hip.h dq_decode_sample / _verdict / _count) ----
Z95 = 1.959963984540054                                           # the 97.5 % point of the standard normal distribution
COUNTER_NAMES = ("volumes", "trivial", "in_codespace", "success", "alive", "identity", "repeat", "stopped", "corrections")
VERDICT_IN_CODESPACE, VERDICT_CLASS_SHIFT, VERDICT_SUCCESS, VERDICT_ALIVE, VERDICT_DECODED_SHIFT = 1, 1, 8, 16, 5


def wilson_interval(k, n, z=Z95):
    """Wilson score interval (lo, hi) for k events in n trials, closed form:
    centre = (p + z^2 / 2n) / (1 + z^2 / n), half = z sqrt(p (1 - p) / n + z^2 / 4n^2) / (1 + z^2 / n), p = k / n."""
    k, n = int(k), int(n)
    if n <= 0 or not 0 <= k <= n:
        raise ValueError(f"wilson_interval: {k} events in {n} trials")
    p, z2 = k / n, z * z
    den = 1.0 + z2 / n
    centre = (p + z2 / (2.0 * n)) / den
    half = z * math.sqrt(p * (1.0 - p) / n + z2 / (4.0 * n * n)) / den
    return max(0.0, centre - half), min(1.0, centre + half)


def check_rates(value, n_volumes, name):
    """A scalar rate -> float; a 1-D sequence of n_volumes rates -> a C-contiguous float64 array.  Finite and in [0, 1], else ValueError."""
    if hasattr(value, "detach"):
        value = value.detach().cpu().numpy()
    if isinstance(value, (bool, np.bool_)):
        raise ValueError(f"{name}: a boolean is not an error rate")
    try:
        a = np.asarray(value)
    except ValueError as e:
        raise ValueError(f"{name}: not a scalar or a 1-D sequence of rates ({e})") from None
    if a.dtype == object or a.dtype.kind not in "iuf":
        raise ValueError(f"{name}: rates must be real numbers (got dtype {a.dtype})")
    if a.ndim > 1 or (a.ndim == 1 and a.shape[0] != n_volumes):
        raise ValueError(f"{name}: a scalar or a 1-D sequence of {n_volumes} rates (one per volume), got shape {a.shape}")
    scalar = a.ndim == 0
    a = np.array(a, dtype=np.float64, ndmin=1)                     # (a contiguous copy)
    if not np.all((a >= 0.0) & (a <= 1.0)):                        # (NaN fails both)
        raise ValueError(f"{name}: rates must be finite and in [0, 1]")
    return float(a[0]) if scalar else a


def check_eval_lattice(lattice, env):
    """lattice: (d, error_model, use_Y, volume_depth) of the decoder, or None (the environment's own).  Validates the environment as the supplier of
    the lattice and the referee without touching the library; returns its (d, error_model, use_Y, volume_depth)."""
    if env is None:
        raise ValueError("an environment is needed: it supplies the lattice and the referee")
    got = lattice_of(env)
    d, model, use_Y, depth = got
    check_decode_args(d, model, use_Y, depth, (depth, d + 1, d + 1))                 # odd d, d <= 7, <= 128 actions, known error model
    if getattr(getattr(env, "_v", env), "wide", False):
        raise NotImplementedError("scoring covers the narrow environment's referees: the wide environment (backend='wide' / the matching referee) is not supported")
    if lattice is not None:
        want = (int(lattice[0]), str(lattice[1]), bool(lattice[2]), int(lattice[3]))
        same = got[0] == want[0] and got[1] == want[1] and got[3] == want[3] and (got[1] == "X" or got[2] == want[2])
        if not same:
            raise ValueError(f"the environment's lattice (d, error model, use_Y, volume_depth) = {got} is not the decoder's {want}")
    return got


def check_eval_args(lattice, env, n_volumes, p_phys=None, p_meas=None, seed=None, env_id_base=0, block=None):
    """Validates an evaluate / sample request without touching the library.  Returns (n_volumes, p_phys, p_meas, seed, env_id_base, block): rates as
    floats or per-volume float64 arrays (default: the environment's, p_meas=None with a given p_phys: the same as p_phys), block = volumes per
    block of counters (default: all in one)."""
    check_eval_lattice(lattice, env)
    return check_volume_args(n_volumes, p_phys, p_meas, seed, env_id_base, block, own_rates(env))


def own_rates(env):
    """The (p_phys, p_meas, seed) an environment offers as the defaults of a scoring request, None where it has none."""
    v = getattr(env, "_v", env)
    return getattr(v, "p_phys", None), getattr(v, "p_meas", None), getattr(v, "seed", None)


def check_volume_args(n, p_phys, p_meas, seed, env_id_base, block, own, count="n_volumes", total="n_volumes"):
    """"Which volumes, at which rates" of every scoring entry point, validated without touching the library.  own: the defaults (p_phys, p_meas, seed) of
    the environment, or None when the lattice came as a tuple and has none; count / total: what the messages call n and the number of volumes in all.
    Returns (n, p_phys, p_meas, seed, env_id_base, block): rates as floats or per-volume float64 arrays, block = volumes per block of counters
    (default: all in one)."""
    n = check_positive(n, count)
    if n >= 1 << 31:
        raise ValueError(f"{total} must be below 2^31")
    own = (None, None, None) if own is None else own
    if p_phys is None:
        if p_meas is not None:
            raise ValueError("p_meas without p_phys: give both, p_phys alone (p_meas = p_phys), or neither (the environment's rates)")
        if own[0] is None or own[1] is None:
            raise ValueError("p_phys is required when the lattice is given as (d, error_model)")
        p_phys, p_meas = own[0], own[1]
    elif p_meas is None:
        p_meas = p_phys
    p_phys, p_meas = check_rates(p_phys, n, "p_phys"), check_rates(p_meas, n, "p_meas")
    if isinstance(p_phys, float) != isinstance(p_meas, float):      # one array: the scalar becomes one too
        full = lambda x: np.full(n, x, dtype=np.float64) if isinstance(x, float) else x
        p_phys, p_meas = full(p_phys), full(p_meas)
    if seed is None:
        if own[2] is None:
            raise ValueError("seed is required when the lattice is given as (d, error_model)")
        seed = own[2]
    try:
        ok = len(seed) == 2 and all(is_int(x) and 0 <= x < 1 << 32 for x in seed)
    except (TypeError, IndexError):
        ok = False
    if not ok:
        raise ValueError(f"seed must be a pair of 32-bit words, not {seed!r}")
    if not is_int(env_id_base) or not 0 <= env_id_base < 1 << 32:
        raise ValueError(f"env_id_base must be an integer in 0 .. 2^32 - 1, not {env_id_base!r}")
    return n, p_phys, p_meas, (int(seed[0]), int(seed[1])), int(env_id_base), n if block is None else check_positive(block, "block")


def rate_blocks(n, rates, p_meas, who, count="n_volumes"):
    """rates=[...] of the scoring entry points: n volumes at EACH physical rate, in one evaluation of K n volumes in blocks of n.  p_meas: None (the same
    rates), a scalar, or one per rate.  Returns (total, p_phys, p_meas, block, keys) with per-volume float64 arrays; the rates themselves are for
    check_volume_args to judge."""
    n = check_positive(n, count)
    keys = [float(r) for r in rates]
    K = len(keys)
    if K < 1:
        raise ValueError(f"{who}: no error rates")
    if len(set(keys)) != K:
        raise ValueError(f"{who}: the error rates must be distinct (they key the result)")
    meas = keys if p_meas is None else ([float(p_meas)] * K if np.ndim(p_meas) == 0 else [float(r) for r in p_meas])
    if len(meas) != K:
        raise ValueError(f"{who}: {len(meas)} measurement rates for {K} error rates")
    return n * K, np.repeat(np.asarray(keys, dtype=np.float64), n), np.repeat(np.asarray(meas, dtype=np.float64), n), n, keys


def check_codes(x, d, name, allow_none=False):
    """hidden_state codes [N, d, d] (or [N, d*d]), every cell in 0..3; numpy or torch on any device.  Returns N."""
    if x is None:
        if allow_none:
            return None
        raise ValueError(f"{name} is required")
    shape = tuple(int(k) for k in x.shape)
    if not (len(shape) in (2, 3) and shape[0] >= 1 and int(np.prod(shape[1:])) == d * d and (len(shape) == 2 or shape[1:] == (d, d))):
        raise ValueError(f"{name} must have shape [N, {d}, {d}], got {shape}")
    if hasattr(x, "is_cuda") or type(x).__module__.startswith("torch"):
        bad = bool(((x < 0) | (x > 3)).any().item())
    else:
        a = np.asarray(x)
        if a.dtype.kind not in "biuf":
            raise ValueError(f"{name} must be numeric, got dtype {a.dtype}")
        bad = bool(((a != 0) & (a != 1) & (a != 2) & (a != 3)).any())
    if bad:
        raise ValueError(f"{name} cells must be Pauli codes 0..3")
    return shape[0]


class EvalResult:
    """Counters of scored volumes (COUNTER_NAMES) and what follows from them.  success: the residual error is a stabilizer (in the code space, trivial
    homology class: the step's reward 1); alive: success, or the referee still names the residual's class (the step's done == False).
    failure_rate = 1 - success / volumes is the logical failure probability of decoding one volume; death_rate = 1 - alive / volumes.  With
    return_volumes the per-volume device tensors ride along: volumes, hidden, trivial, decode (a DecodeResult of device tensors), verdict
    (bytes: VERDICT_*).  no_decoder: the same counters for frame = 0 where they were asked for.  inexact: volumes on which the matching baseline
    (score_matching) took its nearest-boundary fallback; 0 for every other decoder."""

    def __init__(self, counters, p_phys=None, p_meas=None, inexact=0):
        self.counters = {k: int(x) for k, x in zip(COUNTER_NAMES, counters)}
        self.p_phys, self.p_meas = p_phys, p_meas
        self.inexact = int(inexact)
        self.volumes = self.hidden = self.trivial = self.decode = self.verdict = None
        self.no_decoder = None

    def __getattr__(self, name):
        if name.startswith("n_") and name[2:] in COUNTER_NAMES:
            return self.counters[name[2:]]
        raise AttributeError(name)

    @property
    def failure_rate(self):
        return 1.0 - self.counters["success"] / self.counters["volumes"]

    @property
    def death_rate(self):
        return 1.0 - self.counters["alive"] / self.counters["volumes"]

    @property
    def failure_interval(self):
        """Wilson 95 % interval of failure_rate."""
        return wilson_interval(self.counters["volumes"] - self.counters["success"], self.counters["volumes"])

    @property
    def death_interval(self):
        return wilson_interval(self.counters["volumes"] - self.counters["alive"], self.counters["volumes"])

    @property
    def trivial_share(self):
        return self.counters["trivial"] / self.counters["volumes"]

    @property
    def mean_corrections(self):
        return self.counters["corrections"] / self.counters["volumes"]

    @property
    def status_histogram(self):
        return {name: self.counters[name] for name in ("identity", "repeat", "stopped")}

    def summary(self):
        """A JSON-ready dict of the counters and the derived figures."""
        out = dict(self.counters)
        out.update(failure_rate=self.failure_rate, failure_interval=list(self.failure_interval), death_rate=self.death_rate,
                   death_interval=list(self.death_interval), trivial_share=self.trivial_share, mean_corrections=self.mean_corrections)
        if self.inexact:
            out["inexact"] = self.inexact
        if self.no_decoder is not None:
            out["no_decoder"] = self.no_decoder.summary()
        return out

    def __repr__(self):
        lo, hi = self.failure_interval
        return f"EvalResult(volumes={self.counters['volumes']}, failure_rate={self.failure_rate:.6g} [{lo:.6g}, {hi:.6g}], death_rate={self.death_rate:.6g})"


def counters_from_arrays(verdict, trivial=None, status=None, n_corrections=None):
    """dq_decode_count's sums on the host, from per-volume arrays (the checker of the device counters)."""
    v = np.asarray(verdict).astype(np.int64)
    zero = np.zeros_like(v)
    st = zero if status is None else np.asarray(status).astype(np.int64)
    return [int(v.size), int(np.asarray(zero if trivial is None else trivial).astype(bool).sum()), int(((v & VERDICT_IN_CODESPACE) != 0).sum()),
            int(((v & VERDICT_SUCCESS) != 0).sum()), int(((v & VERDICT_ALIVE) != 0).sum()), int((st == STATUS_IDENTITY).sum()),
            int((st == STATUS_REPEAT).sum()), int((st == STATUS_STOPPED).sum()),
            int(0 if n_corrections is None else np.asarray(n_corrections).astype(np.int64).sum())]


def _narrow_env(env):
    """The VectorEnv behind `env` (the drop-in class keeps one): the holder of the dq_env handle the kernels read the lattice and the referee from."""
    v = getattr(env, "_v", env)
    if getattr(v, "_h", None) is None or not hasattr(v, "device"):
        raise TypeError("env must be a VectorEnv (or the drop-in environment class): its handle supplies the lattice tables and the referee")
    return v


class Counting:
    """dq_decode_count on the library and the stream of a handle: what Evaluator and decoder_wide.WideEvaluator share."""

    def count_into(self, verdict, trivial, status, n_corr, m, first, block, counters):
        from . import _lib
        _lib.check(self.L.dq_decode_count(_lib.ptr(verdict), _lib.ptr(trivial), _lib.ptr(status), _lib.ptr(n_corr), m, first, block,
                                          counters.shape[0], _lib.ptr(counters), self._stream()))


class Evaluator(Counting):
    """Owns a dq_decode_eval handle for chunks of at most `chunk` volumes of one lattice: the sampler, the verdict and the counters."""

    def __init__(self, d, error_model, use_Y, volume_depth, chunk=DEFAULT_CHUNK, device=None):
        import torch
        from . import _lib
        check_decode_args(d, error_model, use_Y, volume_depth, (volume_depth, d + 1, d + 1))
        self.d, self.error_model, self.use_Y, self.volume_depth, self.chunk = int(d), error_model, bool(use_Y), int(volume_depth), int(chunk)
        if self.chunk < 1:
            raise ValueError("chunk must be >= 1")
        self.L = _lib.lib()
        _lib.require_gpu()
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        cfg = _lib.DecodeCfg(d=self.d, volume_depth=self.volume_depth, error_model=MODELS[error_model], use_Y=int(self.use_Y), masked_greedy=0,
                             max_actions=1, action_planes=0, obs_form=0)
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(self.L.dq_decode_eval_create(ctypes.byref(cfg), self.chunk, ctypes.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self.L.dq_decode_eval_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self):
        import torch
        return torch.cuda.current_stream(self.device).cuda_stream

    def sample_into(self, venv, m, lattice_id, seed, p_phys, p_meas, volumes, hidden, trivial):
        """m <= chunk volumes of lattices lattice_id .. lattice_id + m - 1 (mod 2^32) into the given device tensors."""
        from . import _lib
        arr = (ctypes.c_uint32 * 2)(*seed)
        each = not isinstance(p_phys, float)
        _lib.check(self.L.dq_decode_sample(self._h, venv._h, m, lattice_id & 0xFFFFFFFF, arr, 0.0 if each else p_phys, 0.0 if each else p_meas,
                                           p_phys.ctypes.data if each else None, p_meas.ctypes.data if each else None, _lib.ptr(volumes),
                                           _lib.ptr(hidden), _lib.ptr(trivial), self._stream()))

    def match_into(self, volumes, m, frame, weight=None, n_defects=None, inexact=None):
        """The matching baseline (dq_decode_match) on m <= chunk volumes already on the device."""
        from . import _lib
        _lib.check(self.L.dq_decode_match(self._h, _lib.ptr(volumes), m, _lib.ptr(frame), _lib.ptr(weight), _lib.ptr(n_defects), _lib.ptr(inexact),
                                          self._stream()))

    def uf_into(self, volumes, m, frame, weight=None, n_defects=None, rounds=None):
        """The union-find baseline (dq_decode_uf) on m <= chunk volumes already on the device."""
        from . import _lib
        _lib.check(self.L.dq_decode_uf(self._h, _lib.ptr(volumes), m, _lib.ptr(frame), _lib.ptr(weight), _lib.ptr(n_defects), _lib.ptr(rounds),
                                       self._stream()))

    def stream_uf_into(self, syndromes, m, T, commit, frame, weight=None, n_defects=None, rounds=None, final_round="faulty"):
        """The sliding-window union-find decode (dq_stream_decode_uf) of m <= chunk streams of T rounds already on the device; the window is volume_depth.
        final_round="perfect": dq_stream_decode_uf_closed."""
        from . import _lib
        fn = self.L.dq_stream_decode_uf_closed if check_final_round(final_round) else self.L.dq_stream_decode_uf
        _lib.check(fn(self._h, _lib.ptr(syndromes), m, T, commit, _lib.ptr(frame), _lib.ptr(weight), _lib.ptr(n_defects),
                      _lib.ptr(rounds), self._stream()))

    def stream_run_into(self, venv, m, T, commit, lattice_id, seed, p_phys, p_meas, hidden, trivial, frame, weight=None, n_defects=None, rounds=None,
                        syndromes=None, final_round="faulty"):
        """m <= chunk streams of T rounds of lattices lattice_id .. lattice_id + m - 1 (mod 2^32), sampled and decoded in one kernel (dq_stream_run_uf).
        final_round="perfect": dq_stream_run_uf_closed."""
        from . import _lib
        fn = self.L.dq_stream_run_uf_closed if check_final_round(final_round) else self.L.dq_stream_run_uf
        arr = (ctypes.c_uint32 * 2)(*seed)
        each = not isinstance(p_phys, float)
        _lib.check(fn(self._h, venv._h, m, T, commit, lattice_id & 0xFFFFFFFF, arr, 0.0 if each else p_phys, 0.0 if each else p_meas,
                      p_phys.ctypes.data if each else None, p_meas.ctypes.data if each else None, _lib.ptr(hidden), _lib.ptr(trivial),
                      _lib.ptr(frame), _lib.ptr(weight), _lib.ptr(n_defects), _lib.ptr(rounds), _lib.ptr(syndromes), self._stream()))

    def verdict_into(self, venv, hidden, frame, m, out):
        from . import _lib
        _lib.check(self.L.dq_decode_verdict(self._h, venv._h, _lib.ptr(hidden), _lib.ptr(frame), m, _lib.ptr(out), self._stream()))


def score_chunks(ev, dev, n, ph, pm, blk, draw, rows, uncorrected=None, keep=False, decode=None, phases=("sample", "decode"), setup=None, timings=None):
    """The one chunk loop of every scoring entry point -- BatchDecoder.evaluate and score_matching (through score_sampled), memory_experiment, and
    decoder_wide's memory_experiment_wide and score_decode_wide: cuts n volumes into chunks of at most ev.chunk, and per chunk of m volumes, the first
    being volume s, runs draw -> decode -> one verdict and one dq_decode_count per row, on the device; the host reads the counters once, at the end.
    The caller owns the per-volume buffers and addresses them with the slice sl the loop hands out: rows s .. s + m with keep (all n volumes stay),
    else rows 0 .. m (one chunk is resident).
      draw(m, s, sl, p_phys, p_meas) fills the chunk's buffers; the rates are the chunk's share, scalars where it holds one rate pair.
      decode(m, sl), optional, decodes what was drawn.
      rows, and uncorrected where the frame = 0 counts are asked for: each row(m, sl) writes its verdict bytes and returns what count_into takes and
      the loop sums per block of blk volumes -- (verdict, trivial, status or None, n_corr or None, uint8 flags or None: one per volume in their first m cells).
    timings, where given, receives the wall seconds of the phases -- setup (where named: the wait for the previous chunk), phases[0] for draw,
    phases[1] for decode, "verdict" for the rows -- each closed by a synchronisation; without it nothing synchronises before the final read.
    Returns, per row of `rows`, one EvalResult per block, inexact = the row's flagged volumes, no_decoder = the uncorrected row's counts."""
    import time
    import torch
    each = not isinstance(ph, float)
    every = list(rows) + ([uncorrected] if uncorrected is not None else [])
    n_blocks = -(-n // blk)
    counters = torch.zeros((len(every), n_blocks, len(COUNTER_NAMES)), dtype=torch.int64, device=dev)
    flagged = torch.zeros((len(every), n_blocks), dtype=torch.int64, device=dev)

    def phase(name, t0):
        if timings is None:
            return t0
        torch.cuda.current_stream(dev).synchronize()
        t1 = time.perf_counter()
        timings[name] = timings.get(name, 0.0) + (t1 - t0)
        return t1

    for s in range(0, n, ev.chunk):
        m = min(ev.chunk, n - s)
        o = s if keep else 0
        sl = slice(o, o + m)
        t = time.perf_counter()
        if setup is not None:
            t = phase(setup, t)
        a, b = (ph[s:s + m], pm[s:s + m]) if each else (ph, pm)
        if each and (a == a[0]).all() and (b == b[0]).all():   # one rate pair in this chunk: the scalar form (the same thresholds, no table upload)
            a, b = float(a[0]), float(b[0])
        draw(m, s, sl, a, b)
        t = phase(phases[0], t)
        if decode is not None:
            decode(m, sl)
            t = phase(phases[1], t)
        for k, row in enumerate(every):
            verdict, trivial, status, n_corr, flags = row(m, sl)
            ev.count_into(verdict, trivial, status, n_corr, m, s, blk, counters[k])
            if flags is not None:                               # (dq_decode_count's block rule)
                flagged[k].index_add_(0, torch.div(torch.arange(s, s + m, device=dev), blk, rounding_mode="floor"), flags[:m].to(torch.int64))
        t = phase("verdict", t)
    host, sums = counters.cpu().numpy(), flagged.cpu().numpy()
    host0, sums0 = (host[-1], sums[-1]) if uncorrected is not None else (None, None)
    return [block_results(host[k], sums[k], host0, sums0, blk, ph, pm) for k in range(len(rows))]


def block_results(host, flagged, host0, flagged0, blk, ph, pm):
    """One EvalResult per block of a row's counters and flag sums (score_chunks' host read); host0 / flagged0: those of the uncorrected row, or None."""
    each = not isinstance(ph, float)
    results = []
    for k in range(len(host)):
        lo = k * blk
        r = EvalResult(host[k], ph[lo] if each else ph, pm[lo] if each else pm, inexact=flagged[k])
        if host0 is not None:
            r.no_decoder = EvalResult(host0[k], r.p_phys, r.p_meas, inexact=flagged0[k])
        results.append(r)
    return results


def keyed(results, keys):
    """A scoring call's answer from its EvalResults per block: the one result, or {rate: result} for rates=[...]."""
    return results[0] if keys is None else dict(zip(keys, results))


def corrected_cells(frame):
    """The non-zero cells of each frame [m, d, d] as int32 [m]: the corrections a baseline decoder's volume is counted with."""
    import torch
    return (frame != 0).reshape(frame.shape[0], -1).sum(dim=1, dtype=torch.int32)


def score_sampled(ev, venv, dev, n, ph, pm, seed, base, blk, decode, decode_phase, keep=False, no_decoder=False, timings=None):
    """What BatchDecoder.evaluate and score_matching hand to score_chunks: sample -> decode -> verdict -> counts, so that two decoders scored with the
    same (n, rates, seed, base) see the same volumes whatever their chunk sizes.  decode(vol, m, o) decodes the m volumes `vol` (rows o .. o + m of the
    caller's per-volume buffers) and returns (frame, status, n_corr, extra) device tensors, `extra` an optional uint8 flag per volume summed per
    block; its wall time is reported as timings[decode_phase].  keep: the per-volume tensors of all n volumes stay (else one chunk is resident).
    Returns (one EvalResult per block, tensors = dict(volumes, hidden, trivial, verdict))."""
    import torch
    d, depth = ev.d, ev.volume_depth
    rows = n if keep else min(ev.chunk, n)
    vol = torch.empty((rows, depth, d + 1, d + 1), dtype=torch.uint8, device=dev)
    hid = torch.empty((rows, d, d), dtype=torch.uint8, device=dev)
    triv = torch.empty(rows, dtype=torch.uint8, device=dev)
    verd = torch.empty(rows, dtype=torch.uint8, device=dev)
    verd0 = torch.empty(min(ev.chunk, n), dtype=torch.uint8, device=dev) if no_decoder else None
    decoded = None

    def sample(m, s, sl, a, b):
        ev.sample_into(venv, m, base + s, seed, a, b, vol[sl], hid[sl], triv[sl])

    def decode_chunk(m, sl):
        nonlocal decoded
        decoded = decode(vol[sl], m, sl.start)

    def corrected(m, sl):
        frame, status, n_corr, extra = decoded
        ev.verdict_into(venv, hid[sl], frame, m, verd[sl])
        return verd[sl], triv[sl], status, n_corr, extra

    def uncorrected(m, sl):
        ev.verdict_into(venv, hid[sl], None, m, verd0[:m])
        return verd0[:m], triv[sl], None, None, None

    results, = score_chunks(ev, dev, n, ph, pm, blk, sample, [corrected], uncorrected if no_decoder else None, keep=keep, decode=decode_chunk,
                            phases=("sample", decode_phase), setup="setup", timings=timings)
    return results, dict(volumes=vol, hidden=hid, trivial=triv, verdict=verd)


def sample_volumes(env, n_volumes, p_phys=None, p_meas=None, seed=None, env_id_base=0, chunk=DEFAULT_CHUNK, to_host=False):
    """n_volumes independent memory experiments from a clean lattice, drawn on the device: volume i is volume_depth rounds of (error, faulty
    syndrome measurement) of lattice env_id_base + i under the environment's random-number convention, all-zero volumes included (the
    environment's reset redraws those; this is the unbiased sample a failure rate needs).  env: the lattice (a VectorEnv or the drop-in class);
    rates: scalars or one per volume, default the environment's; seed: default the environment's.  Returns (volumes uint8 [N, depth, d+1, d+1]
    -- decode's input --, hidden uint8 [N, d, d] the accumulated error as hidden_state codes, trivial uint8 [N]: 1 where the volume is all zero),
    device tensors unless to_host."""
    import torch
    n, ph, pm, seed, base, _ = check_eval_args(None, env, n_volumes, p_phys, p_meas, seed, env_id_base)
    venv = _narrow_env(env)
    d, model, use_Y, depth = lattice_of(venv)
    dev = venv.device
    ev = Evaluator(d, model, use_Y, depth, chunk=min(int(chunk), n), device=dev)
    try:
        vol = torch.empty((n, depth, d + 1, d + 1), dtype=torch.uint8, device=dev)
        hid = torch.empty((n, d, d), dtype=torch.uint8, device=dev)
        triv = torch.empty(n, dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            for s in range(0, n, ev.chunk):
                m = min(ev.chunk, n - s)
                each = not isinstance(ph, float)
                ev.sample_into(venv, m, base + s, seed, ph[s:s + m] if each else ph, pm[s:s + m] if each else pm, vol[s:s + m], hid[s:s + m],
                               triv[s:s + m])
            torch.cuda.current_stream(dev).synchronize()
    finally:
        ev.close()
    out = (vol, hid, triv)
    return tuple(x.cpu().numpy() for x in out) if to_host else out


def verdict(hidden, frame, env, chunk=DEFAULT_CHUNK, to_host=False):
    """What the environment's step decides on the residual error hidden XOR frame of each volume (hidden, frame: Pauli codes 0..3 [N, d, d], numpy
    or torch; frame=None: no correction, the "no decoder" baseline), with the referee installed on `env`.  Returns (bytes uint8 [N] -- VERDICT_*:
    in code space, class of the residual, success, alive, the referee's class --, EvalResult of their counts)."""
    import torch
    d, model, use_Y, depth = check_eval_lattice(None, env)
    n = check_codes(hidden, d, "hidden")
    if frame is not None and check_codes(frame, d, "frame") != n:
        raise ValueError(f"hidden has {n} volumes, frame {int(frame.shape[0])}")
    venv = _narrow_env(env)
    dev = venv.device
    on = lambda x: (x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(x)))).to(device=dev, dtype=torch.uint8).reshape(n, d, d).contiguous()
    hid, frm = on(hidden), None if frame is None else on(frame)
    ev = Evaluator(d, model, use_Y, depth, chunk=min(int(chunk), n), device=dev)
    try:
        out = torch.empty(n, dtype=torch.uint8, device=dev)
        counters = torch.zeros((1, len(COUNTER_NAMES)), dtype=torch.int64, device=dev)
        with torch.cuda.device(dev):
            for s in range(0, n, ev.chunk):
                m = min(ev.chunk, n - s)
                ev.verdict_into(venv, hid[s:s + m], None if frm is None else frm[s:s + m], m, out[s:s + m])
                ev.count_into(out[s:s + m], None, None, None, m, s, n, counters)
            res = EvalResult(counters.cpu().numpy()[0])
    finally:
        ev.close()
    return (out.cpu().numpy() if to_host else out), res


# ---- the space-time matching baseline (include/deepq_hip.h dq_decode_match; csrc/match_st.hip) ----------------------------
class MatchResult:
    """Per-volume results of matching_decode, in input order: frame uint8 [N, d, d] (the matching's net correction as hidden_state codes 0..3, what
    verdict() takes), weight int32 [N, 2] (the matching's weight per Pauli component: 0 = X errors / type-3 plaquettes, 1 = Z errors / type-1),
    n_defects int32 [N, 2], inexact uint8 [N] (1: a cluster beyond 14 defects or defects beyond the first 32 took the nearest-boundary fallback; all 0
    for method="union_find", which has none), rounds int32 [N, 2] (union-find: growth rounds per component; None for matching)."""

    def __init__(self, frame, weight, n_defects, inexact, rounds=None):
        self.frame, self.weight, self.n_defects, self.inexact, self.rounds = frame, weight, n_defects, inexact, rounds

    def __repr__(self):
        return f"MatchResult(volumes={int(self.frame.shape[0])})"


def check_match_args(env, volumes, chunk=DEFAULT_CHUNK):
    """Validates a matching_decode request without touching the library.  Returns (d, error_model, use_Y, volume_depth, n_volumes)."""
    d, model, use_Y, depth = check_eval_lattice(None, env)
    check_chunk(chunk)
    if not hasattr(volumes, "shape") or not hasattr(volumes, "dtype"):
        raise ValueError("volumes must be a numpy array or a torch tensor")
    if str(volumes.dtype).replace("torch.", "") != "uint8":
        raise ValueError(f"volumes must be uint8 (sample_volumes' format), got dtype {volumes.dtype}")
    shape = tuple(int(x) for x in volumes.shape)
    if len(shape) != 4 or shape[0] < 1 or shape[1:] != (depth, d + 1, d + 1):
        raise ValueError(f"volumes must have shape [N, {depth}, {d + 1}, {d + 1}], got {shape}")
    check_binary(volumes)
    return d, model, use_Y, depth, shape[0]


def matching_decode(volumes, env, chunk=DEFAULT_CHUNK, to_host=False, evaluator=None, method="matching"):
    """Minimum-weight matching on the space-time volume, unit weights, both Pauli components independently.  volumes: uint8
    [N, volume_depth, d+1, d+1] with 0/1 cells (sample_volumes' output, decode's input), numpy or torch; env supplies the lattice (d <= 7, the narrow
    environment).  Returns a MatchResult of device tensors (numpy arrays with to_host).  The result of a volume does not depend on the batch
    around it or on `chunk`.  evaluator: an Evaluator of this lattice to run on (its chunk is used and it stays open, so that repeated calls build
    the matching tables once); default: one for this call.  method="union_find": the union-find decoder of DESIGN.md section 16 on the same graph
    (weight = edges of its correction, inexact all 0, rounds = its growth rounds per component)."""
    import torch
    check_method(method)
    d, model, use_Y, depth, n = check_match_args(env, volumes, chunk)
    venv = _narrow_env(env)
    dev = venv.device
    vol = (volumes if isinstance(volumes, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(volumes))).to(device=dev).contiguous()
    if evaluator is not None and (evaluator.d, evaluator.error_model, evaluator.use_Y, evaluator.volume_depth) != (d, model, use_Y, depth):
        raise ValueError(f"the evaluator's lattice is not the environment's {(d, model, use_Y, depth)}")
    ev = Evaluator(d, model, use_Y, depth, chunk=min(int(chunk), n), device=dev) if evaluator is None else evaluator
    try:
        frame = torch.empty((n, d, d), dtype=torch.uint8, device=dev)
        weight = torch.empty((n, 2), dtype=torch.int32, device=dev)
        ndef = torch.empty((n, 2), dtype=torch.int32, device=dev)
        uf = method == "union_find"
        inexact = torch.zeros(n, dtype=torch.uint8, device=dev) if uf else torch.empty(n, dtype=torch.uint8, device=dev)
        rounds = torch.empty((n, 2), dtype=torch.int32, device=dev) if uf else None
        with torch.cuda.device(dev):
            for s in range(0, n, ev.chunk):
                m = min(ev.chunk, n - s)
                if uf:
                    ev.uf_into(vol[s:s + m], m, frame[s:s + m], weight[s:s + m], ndef[s:s + m], rounds[s:s + m])
                else:
                    ev.match_into(vol[s:s + m], m, frame[s:s + m], weight[s:s + m], ndef[s:s + m], inexact[s:s + m])
            torch.cuda.current_stream(dev).synchronize()
    finally:
        if evaluator is None:
            ev.close()
    out = (frame, weight, ndef, inexact) + ((rounds,) if uf else ())
    return MatchResult(*(tuple(x.cpu().numpy() for x in out) if to_host else out))


# ---- the matching decoder as a policy of the environment (include/deepq_hip.h dq_env_match_select; csrc/env_match.hip) --------
def frame_to_actions(frame, completed, d, error_model, use_Y):
    """The rule of dq_env_match_select in numpy.  frame: hidden_state codes 0..3 [d, d] (or [d * d]) -- matching_decode's frame F for the lattice's
    current volume, or [2, d, d] 0/1 components (X part, Z part); completed: the action indices in the lattice's completed_actions (any iterable;
    completed_from_words reads them from an exported state), or None.  Returns (wanted, action): wanted = the ascending action indices whose index_to_move XOR to F --
    X model: the X part on the one layer (the Z part is ignored: no action flips it); DP / IIDXZ with use_Y: code 1 / 2 / 3 -> layer 0 / 1 / 2 at
    the qubit; without use_Y: X part -> layer 0, Z part -> layer 1, so a Y cell is the X action and, later, the Z action of its qubit -- and
    action = the lowest wanted index not in `completed`, else the identity (num_actions - 1).  The legal set is not consulted: the environment
    applies any action (Environments.py:131-136)."""
    d = int(d)
    layers = action_layers(error_model, use_Y)
    d2 = d * d
    f = np.asarray(frame)
    if f.size == 2 * d2 and f.ndim >= 2 and f.shape[0] == 2:
        fx, fz = (f[0].reshape(d2) != 0), (f[1].reshape(d2) != 0)
    elif f.size == d2:
        code = f.reshape(d2).astype(np.int64)
        if ((code < 0) | (code > 3)).any():
            raise ValueError("frame cells must be Pauli codes 0..3")
        fx, fz = (code == 1) | (code == 2), (code == 2) | (code == 3)
    else:
        raise ValueError(f"frame must have shape [{d}, {d}] (codes) or [2, {d}, {d}] (components), got {f.shape}")
    if error_model == "X":
        parts = [fx]
    elif use_Y:
        parts = [fx & ~fz, fx & fz, fz & ~fx]
    else:
        parts = [fx, fz]
    wanted = [int(l * d2 + q) for l in range(layers) for q in np.flatnonzero(parts[l])]
    identity = layers * d2
    have = set() if completed is None else {int(x) for x in completed}
    for a in wanted:
        if a not in have:
            return wanted, a
    return wanted, identity


def completed_from_words(w0, w1):
    """The set of action indices in a completed_actions mask (words 6, 7 of dq_env_export_state)."""
    m = int(w0) & (2 ** 64 - 1) | (int(w1) & (2 ** 64 - 1)) << 64
    return {i for i in range(128) if (m >> i) & 1}


def rate_threshold(p):
    """T of csrc/common.h dq_rate_threshold: W / 2^32 < p  <=>  W < T for every 32-bit W, T = ceil(p 2^32) clamped to [0, 2^32]."""
    return max(0, min(math.ceil(float(p) * 4294967296.0), 1 << 32))


def guided_actions(q, legal, teacher_actions, eps, guide_share, masked_greedy, seed, env_id_base, t):
    """The rule of dq_env_guided_select in numpy.  q: float32 [n, num_actions] or None (every lattice explores); legal: the
    lattices' legal sets as two 64-bit words each [n, 2] (VectorEnv.legal; bit a = action a); teacher_actions: int [n], what match_select emits for the
    lattices as they stand; seed: the policy's key (the environment's seed); lattice i has global id env_id_base + i; t: the policy counter.  With
    w[0..3] = Philox4x32-10(counter (t_lo, t_hi, id, STREAM_POLICY << 16), key seed) -- the words select_actions draws -- and T = rate_threshold:
        explore = q is None or w[1] < T(eps);    guided = explore and w[2] < T(guide_share)
        guided: the teacher's action;  else explore: the k-th (0-based, ascending) legal action, k = (w[0] * n_legal) >> 32 (-1 for an empty set);
        else: the first maximum of the Q row, over the legal set when masked_greedy.
    Returns (actions int32 [n], guided_flags uint8 [n]).  The loop itself is decoder_wide.guided_actions_wide's, on the [n, 2] words: the rule is stated once."""
    from .decoder_wide import guided_actions_wide
    for name, v in (("eps", eps), ("guide_share", guide_share)):
        if not 0.0 <= float(v) <= 1.0:
            raise ValueError(f"guided_actions: {name} must lie in [0, 1], not {v!r}")
    words = np.ascontiguousarray(np.asarray(legal)).astype(np.int64, copy=False).reshape(-1, 2)
    n = len(words)
    teacher = np.asarray(teacher_actions).reshape(-1)
    if len(teacher) != n:
        raise ValueError(f"guided_actions: {len(teacher)} teacher actions for {n} legal sets")
    if q is not None:
        q = np.asarray(q, dtype=np.float32)
        if q.ndim != 2 or q.shape[0] != n or not 1 <= q.shape[1] <= 128:
            raise ValueError(f"guided_actions: q must have shape [{n}, num_actions <= 128], got {q.shape}")
    return guided_actions_wide(q, words, teacher, eps, guide_share, masked_greedy, seed, env_id_base, t)


def check_match_policy_args(env, evaluator=None, chunk=DEFAULT_CHUNK):
    """Validates the lattice of a matching-policy evaluation without touching the library: the narrow environment, d <= 7, volume_depth <= 16 (else
    NotImplementedError), an evaluator of the same lattice (else ValueError).  Returns (d, error_model, use_Y, volume_depth)."""
    if env is None:
        raise ValueError("an environment is needed: the policy plays it")
    v = getattr(env, "_v", env)
    d, model, use_Y, depth = lattice_of(v)
    if d < 3 or d % 2 == 0:
        raise ValueError(f"d = {d}: the surface code lattices have odd d >= 3")
    action_layers(model, use_Y)
    if getattr(v, "wide", False) or d > 7:
        raise NotImplementedError(f"the matching policy covers the narrow environment, d <= 7 (d = {d}, wide = {bool(getattr(v, 'wide', False))})")
    if not 1 <= depth <= 16:
        raise NotImplementedError(f"the matching policy covers volume_depth 1..16, not {depth}")
    check_decode_args(d, model, use_Y, depth, (depth, d + 1, d + 1))
    check_chunk(chunk)
    if evaluator is not None:
        theirs = (int(evaluator.d), str(evaluator.error_model), int(evaluator.volume_depth))
        if theirs != (d, model, depth) or (model != "X" and bool(evaluator.use_Y) != use_Y):
            raise ValueError(f"the evaluator's lattice (d, error model, use_Y, volume_depth) = "
                             f"{(theirs[0], theirs[1], bool(evaluator.use_Y), theirs[2])} is not the environment's {(d, model, use_Y, depth)}")
    return d, model, use_Y, depth


class MatchingAgent:
    """Plays the environment with the space-time matching decoder, behind DQNAgent's evaluation surface: per agent step one dq_env_match_select
    launch (the next flip of the matching's frame for the lattice's current volume, then the identity) and one dq_env_step with auto-reset, the
    episode records kept on the device by the loop DQNAgent.test runs (episodes.episode_records).  policy="identity": only ever the identity --
    the "no decoder" row of the same table.  evaluator: an Evaluator of the environment's lattice to run on (it stays open); default: one per
    call.  After a call last_inexact_steps holds the lattice-steps whose volume took the matching's 14 / 32 fallback (summed on the device; per
    rate after test_error_rates: last_inexact_by_rate), last_vector_steps the vector steps made.  method="union_find": the union-find decoder of
    DESIGN.md section 16 plays instead (dq_env_uf_select; it has no fallback, so the inexact counts are 0) -- in test, test_error_rates and, through
    evaluator_for and this attribute, as the guide of a policy in DQNAgent.fit."""

    def __init__(self, evaluator=None, chunk=DEFAULT_CHUNK, policy="matching", method=None):
        if policy not in ("matching", "identity"):
            raise ValueError(f"policy must be 'matching' or 'identity', not {policy!r}")
        if method is not None:
            check_method(method)
            if policy == "identity":
                raise ValueError("policy='identity' plays no decoder: it takes no method")
        self.method = "matching" if method is None else method
        self.evaluator, self.chunk, self.policy = evaluator, check_chunk(chunk), policy
        self.last_inexact_steps, self.last_inexact_by_rate, self.last_vector_steps = 0, {}, 0

    def evaluator_for(self, env):
        """(an Evaluator of env's lattice, whether it was opened here and is the caller's to close): the agent's own where it was given one.  Validates
        like test(): the narrow environment, d <= 7, volume_depth <= 16 (NotImplementedError), an evaluator of the same lattice (ValueError), before any
        library call.  For a caller that plays the matching itself over many steps (DQNAgent.fit with this agent as the policy's guide)."""
        d, model, use_Y, depth = check_match_policy_args(env, self.evaluator, self.chunk)
        if self.evaluator is not None:
            return self.evaluator, False
        venv = _narrow_env(env)
        return Evaluator(d, model, use_Y, depth, chunk=min(self.chunk, int(venv.n_envs)), device=venv.device), True

    def _check_env(self, env):
        """What test() and test_error_rates() require of the environment and the agent's evaluator, before any library call."""
        check_match_policy_args(env, self.evaluator, self.chunk)

    def test(self, env, nb_episodes=1, verbose=1, interval=100, nb_max_episode_steps=None):
        """DQNAgent.test for this policy: the same keys, ceil-share quota and record order (vector step, then lattice).  Returns History."""
        from . import episodes
        from .agent import DQNAgent, History
        self._check_env(env)
        v = getattr(env, "_v", env)
        if not is_int(nb_episodes) or nb_episodes < 0:
            raise ValueError(f"nb_episodes must be a non-negative integer, not {nb_episodes!r}")
        quota = episodes.share_quota(int(v.n_envs), int(nb_episodes))
        episodes.check_step_cap(nb_max_episode_steps, quota)
        if verbose >= 1:
            print(f"Testing for {nb_episodes} episodes ...")
        rec, inexact = self._records(_narrow_env(env), quota, nb_max_episode_steps)
        self.last_inexact_steps, self.last_inexact_by_rate = int(inexact.sum()), {}
        return DQNAgent._history_from_records(rec, verbose >= 2, interval, History())

    def test_error_rates(self, env, error_rates, nb_episodes=1, p_meas=None, verbose=1, interval=100, nb_max_episode_steps=None):
        """DQNAgent.test_error_rates for this policy: the same block layout over the lattices, quotas, keys and record order; the environment's
        previous rates are restored on the way out.  Returns {rate: History}."""
        from . import episodes
        from .agent import DQNAgent
        self._check_env(env)
        v = getattr(env, "_v", env)
        rates, m, ph, pm, quota = episodes.rate_blocks(v.n_envs, error_rates, nb_episodes, p_meas)
        episodes.check_step_cap(nb_max_episode_steps, quota)
        venv = _narrow_env(env)
        if verbose >= 1:
            print(f"Testing for {nb_episodes} episodes at each of {len(rates)} error rates ({m} lattices each) ...")
        previous = venv._rate_forms()
        venv.set_rates(ph, pm)
        try:
            rec, inexact = self._records(venv, quota, nb_max_episode_steps)
        finally:
            venv.set_rates(*previous)
        out = {}
        self.last_inexact_steps, self.last_inexact_by_rate = int(inexact[:len(rates) * m].sum()), {}
        for k, r in enumerate(rates):
            sel = episodes.block_records(rec, k, m)
            out[r] = DQNAgent._history_from_records(sel, verbose >= 2, interval)
            self.last_inexact_by_rate[r] = int(inexact[k * m:(k + 1) * m].sum())
            if verbose >= 1 and len(sel):
                print(f"p = {r}: {len(sel)} episodes, average lifetime {out[r].history['episode_lifetimes_rolling_avg'][-1]:.3f}")
        return out

    def _records(self, venv, quota, nb_max_episode_steps):
        """(records of episodes.episode_records, inexact lattice-steps per lattice int64 [N]) of one evaluation from a reset."""
        import torch
        from . import episodes
        d, model, use_Y, depth = lattice_of(venv)
        dev, N = venv.device, int(venv.n_envs)
        matching = self.policy == "matching"
        ev = self.evaluator
        if matching and ev is None:
            ev = Evaluator(d, model, use_Y, depth, chunk=min(self.chunk, N), device=dev)
        try:
            with torch.cuda.device(dev):
                action = torch.full((N,), int(venv.identity_index), dtype=torch.int32, device=dev)
                flag = torch.zeros(N, dtype=torch.uint8, device=dev)
                inexact = torch.zeros(N, dtype=torch.int64, device=dev)
                steps = [0]

                def step(k):
                    if matching:
                        if self.method == "matching":
                            venv.match_select(ev, out=action, out_inexact=flag)
                            inexact.add_(flag)
                        else:
                            venv.match_select(ev, out=action, method=self.method)
                    venv.step(action, auto_reset=True, write_obs=False)
                    steps[0] = k + 1
                    return venv.done, venv.was_reset, venv.reward, venv.lifetime

                venv.reset(write_obs=False)
                rec = episodes.episode_records(venv.L, dev, venv._stream, N, quota, step, None, nb_max_episode_steps)
                self.last_vector_steps = steps[0]
                return rec, inexact.cpu().numpy()
        finally:
            if matching and self.evaluator is None:
                ev.close()


def expand_rates(lattice, env, n_volumes, rates, p_meas, seed, env_id_base, who):
    """rates=[...] of decode_benchmark / score_matching: n_volumes at EACH physical rate in one evaluation of K n_volumes volumes in blocks of
    n_volumes.  Validates without touching the library; returns (total, p_phys, p_meas, block, keys)."""
    total, ph, pm, blk, keys = rate_blocks(n_volumes, rates, p_meas, who)
    check_eval_args(lattice, env, total, ph, pm, seed, env_id_base, blk)
    return total, ph, pm, blk, keys


def check_rated_args(lattice, env, n, rates, p_phys, p_meas, seed, env_id_base, who):
    """The volumes of score_matching / memory_experiment, with rates=[...] or without.  Returns check_eval_args' tuple and keys (the rates, or None)."""
    block = keys = None
    if rates is not None:
        if p_phys is not None:
            raise ValueError(f"{who}: rates=[...] are the physical rates; p_phys goes without them")
        n, p_phys, p_meas, block, keys = rate_blocks(n, rates, p_meas, who)
    return check_eval_args(lattice, env, n, p_phys, p_meas, seed, env_id_base, block) + (keys,)


def score_matching(env, n_volumes, rates=None, p_phys=None, p_meas=None, seed=None, env_id_base=0, chunk=DEFAULT_CHUNK, no_decoder=False, timings=None,
                   evaluator=None, method="matching"):
    """The matching baseline scored like DQNAgent.decode_benchmark scores the agent, on the SAME volumes for the same env, n_volumes, rates, seed and
    env_id_base (both run score_chunks): sample -> dq_decode_match -> verdict -> counts on the device.  Returns an EvalResult ({rate: EvalResult}
    with rates=[...]; p_meas then as in decode_benchmark; without rates p_phys / p_meas are scalars, default the environment's).  Counters: every
    volume counts as status identity, corrections = the frame's non-zero cells; EvalResult.inexact = volumes that took the fallback.  no_decoder:
    EvalResult.no_decoder counts the verdict for frame = 0.  timings: a dict that receives the wall seconds of the phases (sample / match /
    verdict).  evaluator: an Evaluator of this lattice to run on (its chunk is used, it stays open: its matching tables are built once);
    default: one of `chunk` volumes for this call.  method="union_find": dq_decode_uf in place of dq_decode_match (inexact = 0; the phase key of
    `timings` stays "match")."""
    import torch
    check_method(method)
    lat = check_eval_lattice(None, env)
    check_chunk(chunk)
    n, ph, pm, seed, base, blk, keys = check_rated_args(lat, env, n_volumes, rates, p_phys, p_meas, seed, env_id_base, "score_matching")
    if evaluator is not None and (evaluator.d, evaluator.error_model, evaluator.use_Y, evaluator.volume_depth) != lat:
        raise ValueError(f"the evaluator's lattice is not the environment's {lat}")
    venv = _narrow_env(env)
    d, model, use_Y, depth = lat
    dev = venv.device
    ev = Evaluator(d, model, use_Y, depth, chunk=min(int(chunk), n), device=dev) if evaluator is None else evaluator
    try:
        rows = min(ev.chunk, n)
        frame = torch.empty((rows, d, d), dtype=torch.uint8, device=dev)
        inexact = torch.zeros(rows, dtype=torch.uint8, device=dev)
        status = torch.full((rows,), STATUS_IDENTITY, dtype=torch.uint8, device=dev)

        def decode(vol, m, o):
            if method == "union_find":
                ev.uf_into(vol, m, frame[:m])
            else:
                ev.match_into(vol, m, frame[:m], None, None, inexact[:m])
            return frame[:m], status[:m], corrected_cells(frame[:m]), inexact[:m]

        with torch.cuda.device(dev):
            results, _ = score_sampled(ev, venv, dev, n, ph, pm, seed, base, blk, decode, "match", no_decoder=no_decoder, timings=timings)
    finally:
        if evaluator is None:
            ev.close()
    return keyed(results, keys)


# ---- sliding-window union-find decoding of syndrome streams (include/deepq_hip.h dq_stream_decode_uf / dq_stream_run_uf) --------
STREAM_MAX_ROUNDS = 1 << 20
STREAM_MAX_WINDOW = 16


class StreamResult:
    """Per-stream results of stream_decode, in input order: frame uint8 [N, d, d] (the committed correction as hidden_state codes 0..3, what verdict()
    takes), weight int32 [N, 2] (committed edges per Pauli component), n_defects int32 [N, 2] (the stream's own defects, carries not counted), rounds
    int32 [N, 2] (growth rounds summed over the windows), windows (their number, the same for every stream)."""

    def __init__(self, frame, weight, n_defects, rounds, windows):
        self.frame, self.weight, self.n_defects, self.rounds, self.windows = frame, weight, n_defects, rounds, windows

    def __repr__(self):
        return f"StreamResult(streams={int(self.frame.shape[0])}, windows={self.windows})"


def stream_windows(T, window, commit):
    """The number of windows of a stream of T rounds."""
    return 1 if window >= T else -(-(T - window) // commit) + 1


def check_stream_method(method):
    check_method(method)
    if method != "union_find":
        raise NotImplementedError("stream decoding is union-find only: the matching returns XORs of tabulated paths and not edges per round, so it cannot say "
                                  "which part of a correction lies in the committed rounds")


FINAL_ROUNDS = ("faulty", "perfect")


def check_final_round(final_round):
    """How a stream ends: "faulty", the last round is read like every other one, or "perfect", a last round of reliable syndromes
    as a data-qubit readout gives it (the closed entry points).  Returns whether the stream is closed; ValueError for anything else."""
    if not isinstance(final_round, str) or final_round not in FINAL_ROUNDS:
        raise ValueError(f"final_round must be one of {FINAL_ROUNDS}, not {final_round!r}")
    return final_round == "perfect"


def closed_kw(final_round):
    """The keyword an evaluator's decode / run takes for a closed stream; none for an open one, which is called as ever."""
    return dict(final_round="perfect") if check_final_round(final_round) else {}


def check_stream_schedule(d, rounds, window, commit):
    """(T, window, commit) with the defaults window = min(2 d, 16), commit = (window + 1) // 2; ValueError outside 1 <= commit <= window <= 16, 1 <= T <= 2^20."""
    if window is None:
        window = min(2 * d, STREAM_MAX_WINDOW)
    if not is_int(window) or not 1 <= window <= STREAM_MAX_WINDOW:
        raise ValueError(f"window must be an integer in 1..{STREAM_MAX_WINDOW}, not {window!r}")
    if commit is None:
        commit = (int(window) + 1) // 2
    if not is_int(commit) or not 1 <= commit <= window:
        raise ValueError(f"commit must be an integer in 1..window = {window}, not {commit!r}")
    if not is_int(rounds) or not 1 <= rounds <= STREAM_MAX_ROUNDS:
        raise ValueError(f"a stream has 1..{STREAM_MAX_ROUNDS} rounds, not {rounds!r}")
    return int(rounds), int(window), int(commit)


def check_stream_evaluator(evaluator, d, model, use_Y, window):
    if evaluator is not None:
        got = (evaluator.d, evaluator.error_model, evaluator.volume_depth)
        if got != (d, model, window) or (model != "X" and bool(evaluator.use_Y) != use_Y):
            raise ValueError(f"the evaluator's (d, error model, use_Y, volume_depth) = {got[:2] + (evaluator.use_Y, got[2])} is not the stream's lattice and window "
                             f"{(d, model, use_Y, window)}")


def check_stream_args(env, syndromes, window=None, commit=None, chunk=DEFAULT_CHUNK, evaluator=None, method="union_find"):
    """Validates a stream_decode request without touching the library.  Returns (d, error_model, use_Y, n_streams, single, T, window, commit)."""
    check_stream_method(method)
    d, model, use_Y, _ = check_eval_lattice(None, env)
    check_chunk(chunk)
    if not hasattr(syndromes, "shape") or not hasattr(syndromes, "dtype"):
        raise ValueError("syndromes must be a numpy array or a torch tensor")
    if str(syndromes.dtype).replace("torch.", "") != "uint8":
        raise ValueError(f"syndromes must be uint8, got dtype {syndromes.dtype}")
    shape = tuple(int(x) for x in syndromes.shape)
    single = len(shape) == 3
    if len(shape) not in (3, 4) or shape[-2:] != (d + 1, d + 1) or min(shape[:-2]) < 1:
        raise ValueError(f"syndromes must have shape [N, T, {d + 1}, {d + 1}] or [T, {d + 1}, {d + 1}], got {shape}")
    T, window, commit = check_stream_schedule(d, shape[-3], window, commit)
    check_binary(syndromes)
    check_stream_evaluator(evaluator, d, model, use_Y, window)
    return d, model, use_Y, 1 if single else shape[0], single, T, window, commit


def stream_decode(syndromes, env, window=None, commit=None, chunk=DEFAULT_CHUNK, to_host=False, evaluator=None, method="union_find", final_round="faulty"):
    """Sliding-window union-find decoding of syndrome streams of any length.  syndromes: uint8 [N, T, d+1, d+1] with 0/1 cells, or
    one stream [T, d+1, d+1], numpy or torch; T is free (1 .. 2^20), env supplies the lattice (d <= 7, the narrow environment) and its volume_depth is not
    consulted.  Windows of `window` rounds (default min(2 d, 16)) are decoded by the union-find decoder of section 16; each commits its first `commit`
    rounds (default (window + 1) // 2) and carries the crossing time edges into the next; the last one commits everything.  With window >= T the
    result is matching_decode(method="union_find") at depth T.  Returns a StreamResult of device tensors (numpy arrays with to_host); the result of a
    stream does not depend on the batch around it or on `chunk`.  evaluator: an Evaluator of this lattice with volume_depth = window to run on (its
    chunk is used and it stays open); default: one for this call.  method="matching" raises NotImplementedError.  final_round="perfect": the stream ends on
    a round of reliable syndromes, so the final window has no time edges in its last round; then the frame's syndrome is the
    stream's last syndrome, and T = 1 is code-capacity decoding."""
    import torch
    closed = closed_kw(final_round)
    d, model, use_Y, n, single, T, window, commit = check_stream_args(env, syndromes, window, commit, chunk, evaluator, method)
    venv = _narrow_env(env)
    dev = venv.device
    syn = (syndromes if isinstance(syndromes, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(syndromes))).to(device=dev).reshape(n, T, d + 1, d + 1).contiguous()
    ev = Evaluator(d, model, use_Y, window, chunk=min(int(chunk), n), device=dev) if evaluator is None else evaluator
    try:
        frame = torch.empty((n, d, d), dtype=torch.uint8, device=dev)
        weight, ndef, rounds = (torch.empty((n, 2), dtype=torch.int32, device=dev) for _ in range(3))
        with torch.cuda.device(dev):
            for s in range(0, n, ev.chunk):
                m = min(ev.chunk, n - s)
                ev.stream_uf_into(syn[s:s + m], m, T, commit, frame[s:s + m], weight[s:s + m], ndef[s:s + m], rounds[s:s + m], **closed)
            torch.cuda.current_stream(dev).synchronize()
    finally:
        if evaluator is None:
            ev.close()
    out = (frame, weight, ndef, rounds)
    return StreamResult(*(tuple(x.cpu().numpy() for x in out) if to_host else out), stream_windows(T, window, commit))


def score_streams(ev, dev, n, T, ph, pm, blk, run, verdict, uncorrected=None, flags=None, keep=False, setup=None, timings=None):
    """What memory_experiment and decoder_wide.memory_experiment_wide hand to score_chunks: sample-and-decode in one launch -> verdict -> counts, every
    stream counted as status identity with corrections = the frame's non-zero cells.  run(m, s, p_phys, p_meas, hidden, trivial, frame, syndromes)
    draws and decodes streams s .. s + m of T rounds (syndromes: None unless kept); verdict(hidden, frame, m, out) writes the bytes of the corrected
    residuals and uncorrected(hidden, m, out), where given, those of frame = 0; flags: the uint8 buffer of a chunk in which both leave a flag per
    stream, or None.  keep: the streams of all n stay (else one chunk is resident).  Returns (one EvalResult per block, dict(syndromes, hidden,
    frame, trivial))."""
    import torch
    d, step = ev.d, min(ev.chunk, n)
    rows = n if keep else step
    hid = torch.empty((rows, d, d), dtype=torch.uint8, device=dev)
    frame = torch.empty((rows, d, d), dtype=torch.uint8, device=dev)
    triv = torch.empty(rows, dtype=torch.uint8, device=dev)
    syn = torch.empty((n, T, d + 1, d + 1), dtype=torch.uint8, device=dev) if keep else None
    verd = torch.empty(step, dtype=torch.uint8, device=dev)
    status = torch.full((step,), STATUS_IDENTITY, dtype=torch.uint8, device=dev)

    def draw(m, s, sl, a, b):
        run(m, s, a, b, hid[sl], triv[sl], frame[sl], None if syn is None else syn[sl])

    def corrected(m, sl):
        verdict(hid[sl], frame[sl], m, verd[:m])
        return verd[:m], triv[sl], status[:m], corrected_cells(frame[sl]), flags

    def bare(m, sl):
        uncorrected(hid[sl], m, verd[:m])
        return verd[:m], triv[sl], None, None, flags

    results, = score_chunks(ev, dev, n, ph, pm, blk, draw, [corrected], None if uncorrected is None else bare, keep=keep, phases=("run",), setup=setup,
                            timings=timings)
    return results, dict(syndromes=syn, hidden=hid, frame=frame, trivial=triv)


def memory_experiment(env, n_runs, rounds, window=None, commit=None, rates=None, p_phys=None, p_meas=None, seed=None, env_id_base=0, chunk=DEFAULT_CHUNK,
                      no_decoder=False, timings=None, evaluator=None, return_streams=False, final_round="faulty"):
    """The logical failure of a memory experiment of `rounds` rounds, decoded by the sliding-window union-find decoder: n_runs streams, stream i the first
    `rounds` rounds of lattice env_id_base + i under sample_volumes' convention, sampled and decoded in ONE kernel per chunk (dq_stream_run_uf: the
    syndromes never reach memory), then verdict -> counts on the device as score_matching does.  Returns what score_matching returns: an EvalResult
    ({rate: EvalResult} with rates=[...], n_runs streams per rate, p_meas then as in decode_benchmark), every stream counted as status identity,
    corrections = the frame's non-zero cells, inexact 0; no_decoder: EvalResult.no_decoder counts the verdict for frame = 0.  window / commit: as
    stream_decode.  timings: a dict that receives the wall seconds of the phases run / verdict.  evaluator: an Evaluator of this lattice with
    volume_depth = window.  return_streams: also returns dict(syndromes uint8 [N, rounds, d+1, d+1], hidden, frame uint8 [N, d, d], trivial uint8 [N]) of
    device tensors; otherwise only the counters leave the device.  final_round="perfect": the last round is measured without error (its data errors
    land, its measurement flips are not applied; the same Philox words are drawn) and decoded as stream_decode decodes it; hidden and rounds
    0 .. rounds - 2 are those of the "faulty" run of the same seed and ids, and every residual is in the code space."""
    import torch
    closed = closed_kw(final_round)
    lat = check_eval_lattice(None, env)
    d, model, use_Y, _ = lat
    T, window, commit = check_stream_schedule(d, rounds, window, commit)
    check_chunk(chunk)
    n, ph, pm, seed, base, blk, keys = check_rated_args(lat, env, n_runs, rates, p_phys, p_meas, seed, env_id_base, "memory_experiment")
    check_stream_evaluator(evaluator, d, model, use_Y, window)
    venv = _narrow_env(env)
    dev = venv.device
    ev = Evaluator(d, model, use_Y, window, chunk=min(int(chunk), n), device=dev) if evaluator is None else evaluator
    try:
        def run(m, s, a, b, hid, triv, frame, syn):
            ev.stream_run_into(venv, m, T, commit, base + s, seed, a, b, hid, triv, frame, syndromes=syn, **closed)

        def verdict(hid, frame, m, out):
            ev.verdict_into(venv, hid, frame, m, out)

        with torch.cuda.device(dev):
            results, streams = score_streams(ev, dev, n, T, ph, pm, blk, run, verdict, (lambda hid, m, out: verdict(hid, None, m, out)) if no_decoder else None,
                                             keep=return_streams, setup="setup", timings=timings)
    finally:
        if evaluator is None:
            ev.close()
    return (keyed(results, keys), streams) if return_streams else keyed(results, keys)


class DecodeResult:
    """Per-volume results, in input order.  corrections int32 [N, max_actions] (padded with -1), n_corrections int32 [N], frame uint8
    [N, d, d] (net Pauli frame of the corrections as hidden_state codes 0..3), status uint8 [N] (STATUS_*).  One volume in: the leading
    axis is dropped.  iterations: decode iterations of each chunk."""

    def __init__(self, corrections, n_corrections, frame, status, iterations):
        self.corrections, self.n_corrections, self.frame, self.status = corrections, n_corrections, frame, status
        self.iterations = iterations

    def correction_list(self, i=None):
        """The corrections of volume i (of the one volume when i is None) as a Python list."""
        c, n = (self.corrections, self.n_corrections) if i is None else (self.corrections[i], self.n_corrections[i])
        return [int(a) for a in np.asarray(c)[:int(n)]]

    def __repr__(self):
        return f"DecodeResult(volumes={np.asarray(self.status).size}, iterations={self.iterations})"


class BatchDecoder:
    """Decodes syndrome volumes with a Q-network's weights, in chunks of at most `chunk` volumes.  Owns a QNetwork handle of max_batch =
    chunk (the agent's training handle is not resized) and a dq_decode handle; the weights are packed once per decode() call."""

    def __init__(self, input_shape, c_layers, ff_layers, num_actions, d, error_model, use_Y, volume_depth, dueling=True, masked_greedy=False,
                 max_actions=None, action_planes="environment", obs_form=None, chunk=DEFAULT_CHUNK, device=None):
        import torch
        from . import _lib
        from .env import patch_stride_words
        from .qnet import QNetwork
        _, _, n_act, max_actions = check_decode_args(d, error_model, use_Y, volume_depth, (volume_depth, d + 1, d + 1), action_planes,
                                                     max_actions, obs_form)
        if int(num_actions) != n_act or tuple(input_shape) != (volume_depth + action_layers(error_model, use_Y), 2 * d + 1, 2 * d + 1):
            raise ValueError(f"the network ({tuple(input_shape)} -> {num_actions} actions) does not fit the lattice (d = {d}, {error_model}, "
                             f"volume_depth = {volume_depth})")
        self.d, self.error_model, self.use_Y, self.volume_depth = int(d), error_model, bool(use_Y), int(volume_depth)
        self.masked_greedy, self.max_actions, self.action_planes, self.chunk = bool(masked_greedy), max_actions, action_planes, int(chunk)
        self.net = QNetwork(input_shape, c_layers, ff_layers, num_actions, dueling=dueling, max_batch=self.chunk, device=device)
        self.device = self.net.device
        if obs_form is None:                    # patch words where the network accepts them, uint8 images otherwise
            try:
                self.net.set_patch_input(self.volume_depth, patch_stride_words(self.d))
                obs_form = "patch"
            except _lib.DeepQError:
                obs_form = "uint8"
        elif obs_form == "patch":
            self.net.set_patch_input(self.volume_depth, patch_stride_words(self.d))
        self.obs_form = obs_form
        cfg = _lib.DecodeCfg(d=self.d, volume_depth=self.volume_depth, error_model=MODELS[error_model], use_Y=int(self.use_Y),
                             masked_greedy=int(self.masked_greedy), max_actions=self.max_actions, action_planes=PLANES[action_planes],
                             obs_form=OBS_FORMS[obs_form])
        self.L = _lib.lib()
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(self.L.dq_decode_create(ctypes.byref(cfg), self.chunk, ctypes.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_eval", None) is not None:
            self._eval.close()
            self._eval = None
        if getattr(self, "_h", None):
            self.L.dq_decode_destroy(self._h)
            self._h = None
        if getattr(self, "net", None) is not None:
            self.net.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _input(self, syndromes):
        import torch
        n, single, _, _ = check_decode_args(self.d, self.error_model, self.use_Y, self.volume_depth, tuple(syndromes.shape), self.action_planes,
                                            self.max_actions, self.obs_form)
        check_binary(syndromes)
        t = syndromes if isinstance(syndromes, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(syndromes)))
        t = t.to(device=self.device, dtype=torch.uint8).reshape(n, self.volume_depth, self.d + 1, self.d + 1).contiguous()
        return t, n, single

    def decode(self, params, syndromes, to_host=True):
        """params: float32 device tensor of the network's flat parameters (Keras order).  syndromes: numpy or torch (CPU or device), 0/1
        cells, [N, volume_depth, d+1, d+1] or one volume.  to_host=False leaves the outputs as device tensors."""
        import torch
        from . import _lib
        syn, n, single = self._input(syndromes)
        dev = self.device
        corr = torch.empty((n, self.max_actions), dtype=torch.int32, device=dev)
        ncorr = torch.empty(n, dtype=torch.int32, device=dev)
        frame = torch.empty((n, self.d, self.d), dtype=torch.uint8, device=dev)
        status = torch.empty(n, dtype=torch.uint8, device=dev)
        iters = []
        with torch.cuda.device(dev):
            packed = self.net.pack(params)
            stream = torch.cuda.current_stream(dev).cuda_stream
            it = ctypes.c_int(0)
            for s in range(0, n, self.chunk):
                m = min(self.chunk, n - s)
                _lib.check(self.L.dq_decode_run(self._h, self.net._h, _lib.ptr(params), _lib.ptr(packed), _lib.ptr(syn[s:s + m]), m,
                                                _lib.ptr(corr[s:s + m]), _lib.ptr(ncorr[s:s + m]), _lib.ptr(frame[s:s + m]),
                                                _lib.ptr(status[s:s + m]), ctypes.byref(it), stream))
                iters.append(int(it.value))
        out = [corr, ncorr, frame, status]
        if to_host:
            out = [x.cpu().numpy() for x in out]
        if single:
            out = [x[0] for x in out]
        return DecodeResult(*out, iterations=iters)

    # -- scoring: sample -> decode -> verdict -> counts on the device --------------------------------------------------
    def _decode_into(self, params, packed, syn, m, corr, ncorr, frame, status):
        """One dq_decode_run over m <= chunk volumes already on the device; returns the iterations."""
        import torch
        from . import _lib
        it = ctypes.c_int(0)
        _lib.check(self.L.dq_decode_run(self._h, self.net._h, _lib.ptr(params), _lib.ptr(packed), _lib.ptr(syn), m, _lib.ptr(corr), _lib.ptr(ncorr),
                                        _lib.ptr(frame), _lib.ptr(status), ctypes.byref(it), torch.cuda.current_stream(self.device).cuda_stream))
        return int(it.value)

    def evaluate(self, params, env, n_volumes, p_phys=None, p_meas=None, seed=None, env_id_base=0, return_volumes=False, block=None,
                 no_decoder=False, timings=None):
        """Draws n_volumes volumes (sample_volumes' rule: lattice env_id_base + i, all-zero volumes kept), decodes them with `params`, asks the
        referee installed on `env` for the verdict on hidden XOR frame and sums the flags, all on the device, at most `chunk` volumes resident;
        the host reads the counters once.  Rates: scalars or one per volume; default the environment's.  block: volumes per contiguous block of
        counters (one error rate per block): returns a list of EvalResult, one per block; default one EvalResult for all.  no_decoder: also count
        the verdict for frame = 0 (EvalResult.no_decoder).  return_volumes: the per-volume device tensors ride on the (first) result.  timings:
        a dict that receives the wall seconds of the phases (sample / decode / verdict), each closed by a synchronisation.  The results do not
        depend on the chunk size."""
        import torch
        mine = (self.d, self.error_model, self.use_Y, self.volume_depth)
        n, ph, pm, seed, base, blk = check_eval_args(mine, env, n_volumes, p_phys, p_meas, seed, env_id_base, block)
        venv = _narrow_env(env)
        dev = self.device
        index = lambda x: torch.cuda.current_device() if torch.device(x).index is None else torch.device(x).index
        if index(venv.device) != index(dev):
            raise ValueError(f"the environment lives on {venv.device}, the decoder on {dev}")
        if getattr(self, "_eval", None) is None:
            self._eval = Evaluator(*mine, chunk=self.chunk, device=dev)
        d = self.d
        rows = n if return_volumes else min(self.chunk, n)
        corr = torch.empty((rows, self.max_actions), dtype=torch.int32, device=dev)
        ncorr = torch.empty(rows, dtype=torch.int32, device=dev)
        frame = torch.empty((rows, d, d), dtype=torch.uint8, device=dev)
        status = torch.empty(rows, dtype=torch.uint8, device=dev)
        iters = []
        with torch.cuda.device(dev):
            packed = self.net.pack(params)

            def decode(vol, m, o):
                sl = slice(o, o + m)
                iters.append(self._decode_into(params, packed, vol, m, corr[sl], ncorr[sl], frame[sl], status[sl]))
                return frame[sl], status[sl], ncorr[sl], None

            results, kept = score_sampled(self._eval, venv, dev, n, ph, pm, seed, base, blk, decode, "decode", keep=return_volumes, no_decoder=no_decoder,
                                          timings=timings)
        if return_volumes:
            r = results[0]
            r.volumes, r.hidden, r.trivial, r.verdict = kept["volumes"], kept["hidden"], kept["trivial"], kept["verdict"]
            r.decode = DecodeResult(corr, ncorr, frame, status, iterations=iters)
        return results[0] if block is None else results
