"""Union-find stream decoding for any odd d in 3 .. 15 with a window of up to 32 rounds (include/deepq_hip.h dq_wide_uf_*; csrc/uf_wide.hip; DESIGN.md
section 18): the wide form of decoder.stream_decode / decoder.memory_experiment, which stay as they are and keep refusing d >= 9.

The algorithm and the window schedule are section 17's; for d <= 7 and window <= 16 every field equals decoder.stream_decode's.  The handle
(`WideEvaluator`) owns the lattice tables: no environment is needed.  By default no referee is consulted -- the verdict is "the residual is a stabilizer"
(in the code space, trivial homology class), and EvalResult.death_rate then EQUALS failure_rate by construction and means nothing more.  referee="matching"
(verdict_wide, memory_experiment_wide, DQNAgent.decode_benchmark_wide) sends the residual's true syndrome through the matching referee,
as the wide environment's step does: death_rate is then the share of volumes on which the environment would have ended the episode.  referee="uf"
 asks the union-find referee instead, as VectorEnv(referee="uf")'s step does: no flags, and no launch that has to be sliced.

weights= (stream_decode_wide, memory_experiment_wide) decodes on a weighted graph: an edge of weight w is full at growth 2 w, w_space
for the space edges and w_time for the time edges, so that a misread stabilizer and a flipped qubit cost what their rates say (uf_weights).  None is the
unit-weight launch of before, untouched.  The policy and teacher of the wide environment and decode_benchmark_wide's union-find row take it too (DESIGN.md
section 24): WideUnionFindAgent(weights=...), VectorEnv.uf_select_wide / guided_select_wide(weights=...).  So do they take correlated= (DESIGN.md
section 26): the policy and the teacher decode the lattice's volume in the three correlated passes.

correlated= (stream_decode_wide, memory_experiment_wide, DQNAgent.decode_benchmark_wide) stops decoding the two Pauli components
independently: per window component 0 is decoded dry, component 1 with weight w_corr on the space edges of that correction, component 0 again with
w_corr on the space edges of component 1's (uf_weights_correlated: w_corr = 1 under DP, where a Y error flips one qubit in both).  None is the launch
of before, untouched.

Further down: the union-find decoder as a policy and a teacher of the wide environment (section 19), and batched decoding by a trained agent at these
sizes -- WideBatchDecoder, the wide form of decoder.BatchDecoder, and the scorer behind DQNAgent.decode_benchmark_wide (include/deepq_hip.h
dq_decode_wide_*; csrc/decode_wide.hip).
"""
import ctypes
import math

import numpy as np

from .decoder import (DEFAULT_CHUNK, MODELS, STATUS_IDENTITY, STREAM_MAX_ROUNDS, Counting, MatchingAgent, StreamResult, action_layers, check_binary,
                      check_chunk, check_codes, check_final_round, check_volume_args, closed_kw, corrected_cells, is_int, keyed, lattice_of, own_rates,
                      rate_blocks, rate_threshold, score_chunks, score_streams, stream_windows)

WIDE_MAX_D = 15
WIDE_MAX_WINDOW = 32
WIDE_MAX_WEIGHT = 15


def check_wide_lattice(d, error_model):
    """Odd d in 3 .. 15 and a known error model, else ValueError.  Returns (d, error_model)."""
    if not is_int(d) or d < 3 or d > WIDE_MAX_D or d % 2 == 0:
        raise ValueError(f"d = {d!r}: the wide union-find decoder covers odd d in 3..{WIDE_MAX_D}")
    if error_model not in MODELS:
        raise ValueError(f"error model {error_model!r} is not one of X, DP, IIDXZ")
    return int(d), str(error_model)


def check_wide_schedule(d, rounds, window, commit):
    """(T, window, commit) with the defaults window = min(2 d, 32), commit = (window + 1) // 2; ValueError outside 1 <= commit <= window <= 32,
    1 <= T <= 2^20."""
    if window is None:
        window = min(2 * d, WIDE_MAX_WINDOW)
    if not is_int(window) or not 1 <= window <= WIDE_MAX_WINDOW:
        raise ValueError(f"window must be an integer in 1..{WIDE_MAX_WINDOW}, not {window!r}")
    if commit is None:
        commit = (int(window) + 1) // 2
    if not is_int(commit) or not 1 <= commit <= window:
        raise ValueError(f"commit must be an integer in 1..window = {window}, not {commit!r}")
    if not is_int(rounds) or not 1 <= rounds <= STREAM_MAX_ROUNDS:
        raise ValueError(f"a stream has 1..{STREAM_MAX_ROUNDS} rounds, not {rounds!r}")
    return int(rounds), int(window), int(commit)


REFEREES = ("matching", "uf")


def check_referee(referee):
    """None (no referee: alive := success), "matching" (the matching referee on the residual's true syndrome) or "uf" (the union-find referee on it;
    DESIGN.md section 29), else ValueError.  Returns whether a referee is asked for."""
    if referee is not None and not (isinstance(referee, str) and referee in REFEREES):
        raise ValueError(f"referee must be None, 'matching' or 'uf', not {referee!r}")
    return referee is not None


def uf_weights(p_phys, p_meas, error_model, max_weight=8):
    """The coprime pair (w_space, w_time) in 1 .. max_weight whose ratio is closest, in the logarithm, to L(q_space) / L(q_time), L(q) = ln((1 - q) / q):
    q_space the chance that a qubit flips in one component per round (p_phys for X and IIDXZ, 2 p_phys / 3 for DP), q_time = p_meas, both clamped to
    [1e-12, 0.5 - 1e-12].  Ties go to the smaller sum; equal rates under X give (1, 1)."""
    if error_model not in MODELS:
        raise ValueError(f"error model {error_model!r} is not one of X, DP, IIDXZ")
    if not is_int(max_weight) or not 1 <= max_weight <= WIDE_MAX_WEIGHT:
        raise ValueError(f"max_weight must be an integer in 1..{WIDE_MAX_WEIGHT}, not {max_weight!r}")
    for name, p in (("p_phys", p_phys), ("p_meas", p_meas)):
        if isinstance(p, bool) or not isinstance(p, (int, float, np.integer, np.floating)) or not 0.0 <= float(p) <= 1.0:
            raise ValueError(f"{name} must be a rate in [0, 1], not {p!r}")
    clamp = lambda q: min(max(float(q), 1e-12), 0.5 - 1e-12)
    L = lambda q: math.log((1.0 - q) / q)
    q_space, q_time = clamp(float(p_phys) * (2.0 / 3.0 if error_model == "DP" else 1.0)), clamp(p_meas)
    target = math.log(L(q_space) / L(q_time))
    best = None
    for ws in range(1, int(max_weight) + 1):
        for wt in range(1, int(max_weight) + 1):
            if math.gcd(ws, wt) != 1:
                continue
            err = abs(math.log(ws / wt) - target)
            if best is None or err < best[0] - 1e-12 or (abs(err - best[0]) <= 1e-12 and ws + wt < best[1] + best[2]):
                best = (err, ws, wt)
    return best[1], best[2]


CORRELATED_MIN_SPACE = 4


def uf_weights_correlated(p_phys, p_meas, error_model, max_weight=8):
    """uf_weights' pair with w_corr behind it: the weight of a space edge of one component where the other component's correction
    has the same qubit in the same round.  X and IIDXZ: the components are independent, w_corr = w_space (the weighted decode, unchanged).  DP: given a
    flip in one component the other one has flipped too with chance 1/2, a log-likelihood weight of 0, and the smallest weight the growth bits hold is 1:
    w_corr = 1.  So that 1 is well below w_space, a DP pair with w_space < 4 is multiplied by ceil(4 / w_space) -- by less where the product would pass
    15, the largest weight (with the default max_weight that happens for w_time = 8 alone: (1, 8) stays and w_corr = w_space = 1 changes nothing)."""
    w_space, w_time = uf_weights(p_phys, p_meas, error_model, max_weight)
    if error_model != "DP":
        return w_space, w_time, w_space
    k = max(1, min(-(-CORRELATED_MIN_SPACE // w_space), WIDE_MAX_WEIGHT // max(w_space, w_time)))
    return k * w_space, k * w_time, 1


def check_correlated(correlated, weights, rates=False):
    """correlated= of the wide entry points beside an already validated weights= (check_weights), without touching the library.  None: nothing changes.
    An integer w_corr in 1 .. 15: weights must be an explicit pair or an array of pairs with w_corr <= w_space in each.  With rates, "rates": weights
    must be None or "rates" (uf_weights_correlated of every stream's own rates).  Else ValueError.  Returns None, the integer, or "rates"."""
    if correlated is None:
        return None
    if isinstance(correlated, str):
        if not (rates and correlated == "rates"):
            raise ValueError("correlated must be None" + (", 'rates'" if rates else "") + f" or an integer w_corr in 1..{WIDE_MAX_WEIGHT}, not {correlated!r}")
        if weights is not None and not (isinstance(weights, str) and weights == "rates"):
            raise ValueError(f"correlated='rates' takes its weights from the rates: weights must be None or 'rates', not {weights!r}")
        return correlated
    if not is_int(correlated) or not 1 <= correlated <= WIDE_MAX_WEIGHT:
        raise ValueError("correlated must be None" + (", 'rates'" if rates else "") + f" or an integer w_corr in 1..{WIDE_MAX_WEIGHT}, not {correlated!r}")
    if weights is None or isinstance(weights, str):
        raise ValueError(f"correlated={correlated!r} needs explicit weights=(w_space, w_time) with w_corr <= w_space, not weights={weights!r}")
    w_space = weights[0] if isinstance(weights, tuple) else int(weights[:, 0].min())
    if correlated > w_space:
        raise ValueError(f"correlated: w_corr = {correlated} exceeds w_space = {w_space}")
    return int(correlated)


def with_correlated(weights, correlated):
    """The validated (weights, correlated) as one value for decode_into / run_into: the pair or the uint8 [n, 2] array with w_corr behind it (a triple,
    uint8 [n, 3]); weights itself where correlated is None."""
    if correlated is None:
        return weights
    if isinstance(weights, tuple):
        return weights + (correlated,)
    return np.ascontiguousarray(np.concatenate([weights, np.full((len(weights), 1), correlated, dtype=np.uint8)], axis=1))


def _rate_rows(of_rates, cols, p_phys, p_meas, error_model, n):
    """of_rates(p_phys, p_meas, error_model) of every stream's own rates: one tuple where the rates are scalars, else uint8 [n, cols], every distinct
    rate pair computed once."""
    if isinstance(p_phys, float):
        return of_rates(p_phys, p_meas, error_model)
    out = np.empty((n, cols), dtype=np.uint8)
    seen = {}
    for i, key in enumerate(zip(p_phys.tolist(), p_meas.tolist())):
        if key not in seen:
            seen[key] = of_rates(key[0], key[1], error_model)
        out[i] = seen[key]
    return out


def rate_weights_correlated(p_phys, p_meas, error_model, n):
    """correlated="rates": uf_weights_correlated of every stream's own (p_phys, p_meas).  Returns one triple where the rates are scalars, else uint8 [n, 3]."""
    return _rate_rows(uf_weights_correlated, 3, p_phys, p_meas, error_model, n)


def is_correlated(weights):
    """Whether what decode_into / run_into got as weights= is a triple or an array of triples."""
    if isinstance(weights, tuple):
        return len(weights) == 3
    shape = getattr(weights, "shape", None)
    return shape is not None and len(shape) == 2 and int(shape[1]) == 3


def weights_call(weights):
    """What a validated weights= amounts to for the library, at every call site that hands weights on (WideEvaluator.decode_into / run_into,
    VectorEnv.uf_select_wide / guided_select_wide): (the entry point's suffix, its scalar weights, its per-row device tensor or None).  None: ("", (),
    None), the unit-weight entry point, which takes neither.  A pair or triple: ("_weighted" / "_correlated", the tuple, None).  A uint8 device tensor
    [n, 2] / [n, 3]: (the suffix, ones -- the library wants a valid uniform pair beside an array --, the tensor)."""
    if weights is None:
        return "", (), None
    corr = is_correlated(weights)
    suffix = "_correlated" if corr else "_weighted"
    if isinstance(weights, tuple):
        return suffix, weights, None
    return suffix, (1,) * (3 if corr else 2), weights


def check_weights(weights, n=None, rates=False):
    """weights= of the wide entry points, validated without touching the library: None; a pair (w_space, w_time) of integers in 1 .. 15, returned as a tuple;
    with n, an integer array [n, 2] of such pairs, returned as uint8 [n, 2]; with rates, the string "rates", returned as it is.  Else ValueError."""
    if weights is None:
        return None
    what = "a pair (w_space, w_time)" + (" or 'rates'" if rates else "") + (f" or an integer array [{n}, 2]" if n is not None else "")
    if isinstance(weights, str):
        if rates and weights == "rates":
            return weights
        raise ValueError(f"weights must be None, {what}, not {weights!r}")
    if hasattr(weights, "detach"):                                    # a torch tensor
        weights = weights.detach().cpu().numpy()
    if isinstance(weights, (tuple, list)) and len(weights) == 2 and all(is_int(x) for x in weights):
        a = np.asarray(weights, dtype=np.int64)
    elif isinstance(weights, (tuple, list)) and all(isinstance(r, (tuple, list)) and all(is_int(x) for x in r) for r in weights):
        a = np.asarray([list(r) for r in weights] or [[]], dtype=np.int64)
    elif isinstance(weights, np.ndarray) and weights.dtype.kind in "iu":
        a = weights
    else:
        raise ValueError(f"weights must be None, {what}, of integers in 1..{WIDE_MAX_WEIGHT}, not {weights!r}")
    if a.shape != (2,) and (n is None or a.shape != (n, 2)):
        raise ValueError(f"weights must be None, {what}, not shape {a.shape}")
    if int(a.min()) < 1 or int(a.max()) > WIDE_MAX_WEIGHT:
        raise ValueError(f"weights must lie in 1..{WIDE_MAX_WEIGHT}, not {weights!r}")
    return (int(a[0]), int(a[1])) if a.ndim == 1 else np.ascontiguousarray(a.astype(np.uint8))


def rate_weights(p_phys, p_meas, error_model, n):
    """weights="rates": uf_weights of every stream's own (p_phys, p_meas).  Returns one pair where the rates are scalars, else uint8 [n, 2]."""
    return _rate_rows(uf_weights, 2, p_phys, p_meas, error_model, n)


def check_policy_weights(weights, n=None):
    """weights= of the wide environment's policy and teacher (WideUnionFindAgent, VectorEnv.uf_select_wide's values), validated without touching the
    library: None, a pair, "rates", or one pair per lattice -- an integer array [n, 2], or a uint8 device tensor [n, 2], which is returned as it is; so
    is a uint8 device tensor [n, 3] of triples (w_space, w_time, w_corr), which asks for the correlated decode.
    n=None (the lattices are not known yet): any number of rows.  Else ValueError."""
    if weights is None:
        return None
    if getattr(weights, "is_cuda", False):
        shape = tuple(int(x) for x in weights.shape)
        if str(weights.dtype) != "torch.uint8" or len(shape) != 2 or shape[1] not in (2, 3) or (n is not None and shape[0] != n):
            raise ValueError(f"a device tensor of weights is uint8 [{'n_envs' if n is None else n}, 2 or 3], not {weights.dtype} {shape}")
        return weights
    rows = n
    if rows is None and not isinstance(weights, (str, dict)):
        try:
            shape = np.shape(weights)
        except ValueError:                                            # ragged nesting
            shape = ()
        rows = shape[0] if len(shape) == 2 else None
    return check_weights(weights, rows, rates=True)


def weight_pairs(weights, rates=None, error_model=None, n=None):
    """What a validated weights= amounts to, for a report: None, the pair, or the sorted list of the distinct pairs of the lattices (one pair where all
    agree).  rates: the lattices' (p_phys, p_meas), read for "rates"."""
    if weights is None or isinstance(weights, tuple):
        return weights
    if isinstance(weights, str):
        ph, pm = rates
        pm = ph if pm is None else pm
        if np.ndim(ph) == 0 and np.ndim(pm) == 0:
            return uf_weights(float(ph), float(pm), error_model)
        weights = rate_weights(*(np.broadcast_to(np.asarray(x, dtype=np.float64), (n,)) for x in (ph, pm)), error_model, n)
    if hasattr(weights, "detach"):
        weights = weights.detach().cpu().numpy()
    a = np.asarray(weights)
    pairs = sorted({tuple(int(x) for x in row) for row in np.unique(a.reshape(-1, a.shape[-1]), axis=0)})       # (pairs, or triples with correlated=)
    return pairs[0] if len(pairs) == 1 else pairs


def weights_kw(weights, dev, s=0, m=None):
    """What decode_into / run_into take as weights= for streams s .. s + m: nothing for None (the unweighted call, argument for argument), the pair, or
    the streams' rows of a uint8 device tensor [N, 2]."""
    if weights is None:
        return {}
    return dict(weights=weights if isinstance(weights, tuple) else weights[s:s + m])


def check_wide_evaluator(evaluator, d, error_model, window):
    if evaluator is not None:
        got = (evaluator.d, evaluator.error_model, evaluator.window)
        if got != (d, error_model, window):
            raise ValueError(f"the evaluator's (d, error model, window) = {got} is not the stream's {(d, error_model, window)}")


def lattice_of_wide(lattice):
    """`lattice`: (d, error_model), or an environment of either backend (the drop-in class, a VectorEnv, or any object with d and error_model).  Returns
    (d, error_model, the environment's (p_phys, p_meas, seed) or None)."""
    if isinstance(lattice, (tuple, list)):
        if len(lattice) != 2:
            raise ValueError(f"lattice must be (d, error_model) or an environment, not {lattice!r}")
        d, model = check_wide_lattice(lattice[0], lattice[1])
        return d, model, None
    v = getattr(lattice, "_v", lattice)
    if v is None or not hasattr(v, "d") or not hasattr(v, "error_model"):
        raise ValueError(f"lattice must be (d, error_model) or an environment, not {lattice!r}")
    d, model = check_wide_lattice(int(v.d), str(v.error_model))
    return d, model, own_rates(v)


def check_wide_stream_args(syndromes, d, window=None, commit=None, chunk=DEFAULT_CHUNK, evaluator=None, error_model="DP"):
    """Validates a stream_decode_wide request without touching the library.  Returns (d, n_streams, single, T, window, commit, chunk)."""
    d, error_model = check_wide_lattice(d, error_model if evaluator is None else evaluator.error_model)
    chunk = check_chunk(chunk)
    if not hasattr(syndromes, "shape") or not hasattr(syndromes, "dtype"):
        raise ValueError("syndromes must be a numpy array or a torch tensor")
    if str(syndromes.dtype).replace("torch.", "") != "uint8":
        raise ValueError(f"syndromes must be uint8, got dtype {syndromes.dtype}")
    shape = tuple(int(x) for x in syndromes.shape)
    single = len(shape) == 3
    if len(shape) not in (3, 4) or shape[-2:] != (d + 1, d + 1) or min(shape[:-2]) < 1:
        raise ValueError(f"syndromes must have shape [N, T, {d + 1}, {d + 1}] or [T, {d + 1}, {d + 1}], got {shape}")
    T, window, commit = check_wide_schedule(d, shape[-3], window, commit)
    check_binary(syndromes)
    check_wide_evaluator(evaluator, d, error_model, window)
    return d, 1 if single else shape[0], single, T, window, commit, chunk


def check_wide_experiment_args(lattice, n_runs, rounds, window=None, commit=None, rates=None, p_phys=None, p_meas=None, seed=None, env_id_base=0,
                               chunk=DEFAULT_CHUNK, evaluator=None):
    """Validates a memory_experiment_wide request without touching the library.  Returns (d, error_model, T, window, commit, n, p_phys, p_meas, seed, base,
    block, keys, chunk): n streams in all, rates as floats or per-stream float64 arrays, block = streams per block of counters, keys = the rates of
    rates=[...] or None."""
    d, model, own = lattice_of_wide(lattice)
    T, window, commit = check_wide_schedule(d, rounds, window, commit)
    chunk = check_chunk(chunk)
    n, blk, keys = n_runs, None, None
    if rates is not None:
        if p_phys is not None:
            raise ValueError("memory_experiment_wide: rates=[...] are the physical rates; p_phys goes without them")
        n, p_phys, p_meas, blk, keys = rate_blocks(n_runs, rates, p_meas, "memory_experiment_wide", "n_runs")
    n, p_phys, p_meas, seed, base, blk = check_volume_args(n, p_phys, p_meas, seed, env_id_base, blk, own, "n_runs", "the number of streams")
    check_wide_evaluator(evaluator, d, model, window)
    return d, model, T, window, commit, n, p_phys, p_meas, seed, base, blk, keys, chunk


class WideEvaluator(Counting):
    """Owns a dq_wide_uf handle for chunks of at most `chunk` streams of one lattice and one window: decode, sample-and-decode, verdict, counters.  One host
    thread and one stream at a time."""

    def __init__(self, d, error_model, window=None, chunk=DEFAULT_CHUNK, device=None):
        d, error_model = check_wide_lattice(d, error_model)
        _, window, _ = check_wide_schedule(d, 1, window, None)
        self.d, self.error_model, self.window, self.chunk = d, error_model, window, check_chunk(chunk)
        self._h = self._m = None
        self._open(device)

    def _open(self, device):
        import torch
        from . import _lib
        self.L = _lib.lib()
        _lib.require_gpu()
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(self.L.dq_wide_uf_create(self.d, MODELS[self.error_model], self.window, self.chunk, ctypes.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_m", None):
            self.L.dq_match_destroy(self._m)
            self._m = None
        if getattr(self, "_h", None):
            self.L.dq_wide_uf_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self):
        import torch
        return torch.cuda.current_stream(self.device).cuda_stream

    def _referee(self):
        """The evaluator's own dq_match handle of its d, created at the first refereed verdict and destroyed by close()."""
        import torch
        from . import _lib
        if not self._m:
            m = ctypes.c_void_p()
            with torch.cuda.device(self.device):
                _lib.check(self.L.dq_match_create(self.d, ctypes.byref(m)))
            self._m = m
        return self._m

    def decode_into(self, syndromes, m, T, commit, frame, weight=None, n_defects=None, rounds=None, final_round="faulty", weights=None):
        """The sliding-window decode (dq_wide_uf_decode) of m <= chunk streams of T rounds already on the device.  final_round="perfect":
        dq_wide_uf_decode_closed.  weights: a pair (w_space, w_time) or a uint8 device tensor [m, 2], both validated by the caller (check_weights):
        dq_wide_uf_decode_weighted.  A triple (w_space, w_time, w_corr) or a uint8 device tensor [m, 3] (with_correlated): dq_wide_uf_decode_correlated."""
        from . import _lib
        suffix, w, each = weights_call(weights)
        closed = check_final_round(final_round)
        if suffix:
            fn, mode = getattr(self.L, "dq_wide_uf_decode" + suffix), (int(closed), *w, _lib.ptr(each))
        else:
            fn, mode = self.L.dq_wide_uf_decode_closed if closed else self.L.dq_wide_uf_decode, ()
        _lib.check(fn(self._h, _lib.ptr(syndromes), m, T, commit, *mode, _lib.ptr(frame), _lib.ptr(weight), _lib.ptr(n_defects), _lib.ptr(rounds),
                      self._stream()))

    def run_into(self, m, T, commit, lattice_id, seed, p_phys, p_meas, hidden, trivial, frame, weight=None, n_defects=None, rounds=None, syndromes=None,
                 final_round="faulty", weights=None):
        """m <= chunk streams of T rounds of lattices lattice_id .. lattice_id + m - 1 (mod 2^32), sampled and decoded in one kernel (dq_wide_uf_run).
        final_round="perfect": dq_wide_uf_run_closed.  weights: as decode_into's: dq_wide_uf_run_weighted, dq_wide_uf_run_correlated."""
        from . import _lib
        arr = (ctypes.c_uint32 * 2)(*seed)
        each = not isinstance(p_phys, float)
        suffix, w, w_each = weights_call(weights)
        closed = check_final_round(final_round)
        if suffix:
            fn, mode = getattr(self.L, "dq_wide_uf_run" + suffix), (int(closed), *w, _lib.ptr(w_each))
        else:
            fn, mode = self.L.dq_wide_uf_run_closed if closed else self.L.dq_wide_uf_run, ()
        _lib.check(fn(self._h, m, T, commit, lattice_id & 0xFFFFFFFF, arr, 0.0 if each else p_phys, 0.0 if each else p_meas,
                      p_phys.ctypes.data if each else None, p_meas.ctypes.data if each else None, *mode, _lib.ptr(hidden), _lib.ptr(trivial),
                      _lib.ptr(frame), _lib.ptr(weight), _lib.ptr(n_defects), _lib.ptr(rounds), _lib.ptr(syndromes), self._stream()))

    def verdict_into(self, hidden, frame, m, out, referee=None, inexact=None):
        """The verdict bytes of m <= chunk volumes (frame None: no correction).  referee=None: dq_wide_uf_verdict (alive := success, decoded 0);
        referee="matching": dq_wide_uf_verdict_refereed, with inexact (uint8 [m] or None) receiving the referee's fallback flags; referee="uf":
        dq_wide_uf_verdict_refereed_uf, whose referee has no fallback: inexact (a tensor or None) is zeroed."""
        from . import _lib
        if not check_referee(referee):
            if inexact is not None:
                raise ValueError("inexact flags come from the referee: give referee='matching'")
            _lib.check(self.L.dq_wide_uf_verdict(self._h, _lib.ptr(hidden), _lib.ptr(frame), m, _lib.ptr(out), self._stream()))
            return
        if referee == "uf":
            _lib.check(self.L.dq_wide_uf_verdict_refereed_uf(self._h, _lib.ptr(hidden), _lib.ptr(frame), m, _lib.ptr(out), self._stream()))
            if inexact is not None:
                inexact[:m].zero_()
            return
        _lib.check(self.L.dq_wide_uf_verdict_refereed(self._h, self._referee(), _lib.ptr(hidden), _lib.ptr(frame), m, _lib.ptr(out), _lib.ptr(inexact),
                                                      self._stream()))


def stream_decode_wide(syndromes, d, window=None, commit=None, chunk=DEFAULT_CHUNK, to_host=False, evaluator=None, final_round="faulty", weights=None,
                       correlated=None):
    """decoder.stream_decode for any odd d in 3 .. 15 and a window of up to 32 rounds.  syndromes: uint8 [N, T, d+1, d+1] with 0/1 cells, or one stream
    [T, d+1, d+1], numpy or torch; window defaults to min(2 d, 32), commit to (window + 1) // 2.  Returns a decoder.StreamResult of device tensors (numpy
    arrays with to_host); the result of a stream does not depend on the batch around it or on `chunk`.  evaluator: a WideEvaluator of this d and window to
    run on (its chunk is used and it stays open); default: one for this call.  final_round="perfect": decoder.stream_decode's closed form (DESIGN.md
    section 20).  weights: None (unit weights: the launch of before), a pair (w_space, w_time) of integers in 1 .. 15 for every stream, or an integer
    array [N, 2] with one pair per stream: an edge of weight w is full at growth 2 w, StreamResult.weight is the weighted cost
    of the committed edges and StreamResult.rounds counts unit growth rounds.  correlated: None (the launches of before), or an integer w_corr with
    1 <= w_corr <= w_space beside explicit weights: per window component 0 is decoded dry, component 1 with w_corr on the space
    edges of that correction, and component 0 again with w_corr on the space edges of component 1's; weight and rounds count the last two."""
    import torch
    closed = closed_kw(final_round)
    d, n, single, T, window, commit, chunk = check_wide_stream_args(syndromes, d, window, commit, chunk, evaluator)
    weights = check_weights(weights, n)
    weights = with_correlated(weights, check_correlated(correlated, weights))
    ev = WideEvaluator(d, "DP", window, chunk=min(chunk, n)) if evaluator is None else evaluator
    dev = ev.device
    try:
        syn = (syndromes if isinstance(syndromes, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(syndromes))).to(device=dev)
        syn = syn.reshape(n, T, d + 1, d + 1).contiguous()
        frame = torch.empty((n, d, d), dtype=torch.uint8, device=dev)
        weight, ndef, rounds = (torch.empty((n, 2), dtype=torch.int32, device=dev) for _ in range(3))
        if isinstance(weights, np.ndarray):
            weights = torch.from_numpy(weights).to(device=dev)
        with torch.cuda.device(dev):
            for s in range(0, n, ev.chunk):
                m = min(ev.chunk, n - s)
                ev.decode_into(syn[s:s + m], m, T, commit, frame[s:s + m], weight[s:s + m], ndef[s:s + m], rounds[s:s + m], **closed,
                               **weights_kw(weights, dev, s, m))
            torch.cuda.current_stream(dev).synchronize()
    finally:
        if evaluator is None:
            ev.close()
    out = (frame, weight, ndef, rounds)
    return StreamResult(*(tuple(x.cpu().numpy() for x in out) if to_host else out), stream_windows(T, window, commit))


def check_verdict_wide_args(hidden, frame, d, error_model="DP", referee=None, chunk=DEFAULT_CHUNK, evaluator=None):
    """Validates a verdict_wide request without touching the library.  Returns (d, error_model, n_volumes, refereed, chunk)."""
    refereed = check_referee(referee)
    d, error_model = check_wide_lattice(d, error_model if evaluator is None else evaluator.error_model)
    chunk = check_chunk(chunk)
    n = check_codes(hidden, d, "hidden")
    if frame is not None and check_codes(frame, d, "frame") != n:
        raise ValueError(f"hidden has {n} volumes, frame {int(frame.shape[0])}")
    if evaluator is not None and evaluator.d != d:
        raise ValueError(f"the evaluator's d = {evaluator.d} is not the volumes' {d}")
    return d, error_model, n, refereed, chunk


def verdict_wide(hidden, frame, d, error_model="DP", referee=None, chunk=DEFAULT_CHUNK, evaluator=None, to_host=False):
    """decoder.verdict for any odd d in 3 .. 15, without an environment: what the step decides on the residual hidden XOR frame of each volume (hidden,
    frame: Pauli codes 0..3 [N, d, d], numpy or torch; frame=None: no correction).  referee=None: the bytes of dq_wide_uf_verdict (in code space, class,
    success; alive := success).  referee="matching": dq_decode_verdict's byte with the matching referee -- alive and the decoded class as the wide
    environment's step has them (X model: the referee is asked for component 0 only) -- and the result is (bytes, inexact uint8 [N]: 1 where a
    flagged fallback of the referee fired).  referee="uf": the same byte with the union-find referee, and the flags are all zero.
    evaluator: a WideEvaluator of this d (its error model and chunk are used and it stays open).  Device tensors unless to_host."""
    import torch
    d, error_model, n, refereed, chunk = check_verdict_wide_args(hidden, frame, d, error_model, referee, chunk, evaluator)
    ev = WideEvaluator(d, error_model, 1, chunk=min(chunk, n)) if evaluator is None else evaluator
    dev = ev.device
    try:
        on = lambda x: (x if isinstance(x, torch.Tensor) else torch.from_numpy(np.array(x, order="C"))).to(       # (a copy: read-only arrays are welcome)
            device=dev, dtype=torch.uint8).reshape(n, d, d).contiguous()
        hid, frm = on(hidden), None if frame is None else on(frame)
        out = torch.empty(n, dtype=torch.uint8, device=dev)
        flags = torch.empty(n, dtype=torch.uint8, device=dev) if refereed else None
        with torch.cuda.device(dev):
            for s in range(0, n, ev.chunk):
                m = min(ev.chunk, n - s)
                if refereed and frm is None:
                    refereed_uncorrected_into(ev, hid[s:s + m], m, out[s:s + m], flags[s:s + m], referee)
                else:
                    ev.verdict_into(hid[s:s + m], None if frm is None else frm[s:s + m], m, out[s:s + m], referee=referee,
                                    inexact=flags[s:s + m] if refereed else None)
            torch.cuda.current_stream(dev).synchronize()
    finally:
        if evaluator is None:
            ev.close()
    if to_host:
        out, flags = out.cpu().numpy(), flags.cpu().numpy() if refereed else None
    return (out, flags) if refereed else out


UNCORRECTED_REFEREE_D, UNCORRECTED_REFEREE_SLICE = 13, 2048


def refereed_uncorrected_into(ev, hidden, m, out, flags, referee="matching"):
    """The refereed verdict of m volumes with NO correction (the no_decoder row).  Every error is then still on the lattice: nearly every volume reaches
    the referee, and at d >= 13 a few in a hundred hold a cluster of 15 .. 20 defects that walks 2^15 .. 2^20 subsets in one of the referee's eight
    scratch-pool slots.  Measured at d = 15: 2048 such volumes take 0.24 s in one launch, while one launch of 2^16 did not end within minutes (DESIGN.md
    section 22), and a launch cannot be interrupted.  So at d >= UNCORRECTED_REFEREE_D the volumes go in launches of at most UNCORRECTED_REFEREE_SLICE, the
    size that was measured; the bytes and flags of a volume do not depend on the launch around it.  referee="uf" has no such clusters: one launch."""
    step = UNCORRECTED_REFEREE_SLICE if ev.d >= UNCORRECTED_REFEREE_D and referee == "matching" else m
    for s in range(0, m, step):
        k = min(step, m - s)
        ev.verdict_into(hidden[s:s + k], None, k, out[s:s + k], referee=referee, inexact=flags[s:s + k])


def uncorrected_into(ev, hidden, m, out, flags=None, referee="matching"):
    """The verdict of m volumes with no correction, as a scoring call's no_decoder row asks for it: unrefereed, or with `flags` (uint8 [m]) the refereed
    one of `referee` in its measured launches."""
    if flags is None:
        ev.verdict_into(hidden, None, m, out)
    else:
        refereed_uncorrected_into(ev, hidden, m, out, flags, referee)


def memory_experiment_wide(lattice, n_runs, rounds, window=None, commit=None, rates=None, p_phys=None, p_meas=None, seed=None, env_id_base=0,
                           chunk=DEFAULT_CHUNK, no_decoder=False, timings=None, evaluator=None, return_streams=False, final_round="faulty", referee=None,
                           weights=None, correlated=None):
    """decoder.memory_experiment for any odd d in 3 .. 15 and a window of up to 32 rounds: n_runs streams, stream i the first `rounds` rounds of lattice
    env_id_base + i under sample_volumes' convention, sampled and decoded in ONE kernel per chunk (dq_wide_uf_run), then verdict -> counts on the device.
    lattice: (d, error_model), or an environment of either backend, of which only d, error_model, the rates and the seed are read (the defaults of p_phys /
    p_meas / seed; with a tuple p_phys and seed are required).  Returns what memory_experiment returns: an EvalResult ({rate: EvalResult} with
    rates=[...], n_runs streams per rate), every stream counted as status identity, corrections = the frame's non-zero cells; no_decoder:
    EvalResult.no_decoder counts the verdict for frame = 0.  referee=None: no referee is consulted, alive := success, so death_rate equals failure_rate
    by construction.  referee="matching": every verdict of the call goes through dq_wide_uf_verdict_refereed -- alive is what the
    wide environment's step would decide on the residual, every other counter is unchanged, and EvalResult.inexact (of the no_decoder row too) counts
    the volumes on which a flagged fallback of the referee fired.  referee="uf": the same through dq_wide_uf_verdict_refereed_uf, the
    union-find referee of VectorEnv(referee="uf"); inexact is 0 and no launch is sliced.  With no_decoder the matching-refereed verdict of the uncorrected
    errors is the slow part at
    d >= 13 (refereed_uncorrected_into: launches of at most 2048 volumes, 0.24 s each at d = 15, depth 5, p = 0.006, more at higher rates): keep
    n_runs modest there.
    timings: a dict that receives the wall seconds of the phases run / verdict.  evaluator: a WideEvaluator of this lattice and window.  return_streams:
    also returns dict(syndromes uint8 [N, rounds, d+1, d+1], hidden, frame uint8 [N, d, d], trivial uint8 [N]) of device tensors.  final_round="perfect":
    decoder.memory_experiment's closed form.  weights: None (unit weights: the launches of before), a pair (w_space, w_time) of
    integers in 1 .. 15, or "rates": uf_weights of each stream's own (p_phys, p_meas) under the lattice's error model -- with rates=[...] every rate
    block gets its own pair, in the same launches.  Every EvalResult of the answer then has .weights, the pair its streams were
    decoded with (None without weights); it combines with final_round= and referee= without restriction.  correlated: None (the
    launches of before); an integer w_corr beside an explicit pair, as stream_decode_wide's; or "rates" beside weights None or "rates":
    uf_weights_correlated of each stream's own rates, every rate block its own triple in the same launches.  .weights is then the triple
    (w_space, w_time, w_corr)."""
    import torch
    closed = closed_kw(final_round)
    refereed = check_referee(referee)
    weights = check_weights(weights, rates=True)
    correlated = check_correlated(correlated, weights, rates=True)
    d, model, T, window, commit, n, ph, pm, seed, base, blk, keys, chunk = check_wide_experiment_args(
        lattice, n_runs, rounds, window, commit, rates, p_phys, p_meas, seed, env_id_base, chunk, evaluator)
    if correlated == "rates":
        weights = rate_weights_correlated(ph, pm, model, n)
    elif weights == "rates":
        weights = rate_weights(ph, pm, model, n)
    else:
        weights = with_correlated(weights, correlated)
    used = weights                                                    # None, the pair / triple, or uint8 [n, 2] / [n, 3] on the host
    ev = WideEvaluator(d, model, window, chunk=min(chunk, n)) if evaluator is None else evaluator
    dev = ev.device
    try:
        flags = torch.empty(min(ev.chunk, n), dtype=torch.uint8, device=dev) if refereed else None
        ref_kw = dict(referee=referee, inexact=flags) if refereed else {}     # (no referee: the call of before, argument for argument)

        if isinstance(weights, np.ndarray):
            weights = torch.from_numpy(weights).to(device=dev)

        def run(m, s, a, b, hid, triv, frame, syn):
            ev.run_into(m, T, commit, base + s, seed, a, b, hid, triv, frame, syndromes=syn, **closed, **weights_kw(weights, dev, s, m))

        with torch.cuda.device(dev):
            results, streams = score_streams(ev, dev, n, T, ph, pm, blk, run, lambda hid, frame, m, out: ev.verdict_into(hid, frame, m, out, **ref_kw),
                                             (lambda hid, m, out: uncorrected_into(ev, hid, m, out, flags, referee or "matching")) if no_decoder else None, flags=flags,
                                             keep=return_streams, timings=timings)
    finally:
        if evaluator is None:
            ev.close()
    for k, r in enumerate(results):                                   # (a block of rates=[...] holds one rate pair, so one pair of weights)
        if used is None or isinstance(used, tuple):
            r.weights = used
        else:
            r.weights = weight_pairs(used[k * blk:(k + 1) * blk])
        if r.no_decoder is not None:
            r.no_decoder.weights = None
    return (keyed(results, keys), streams) if return_streams else keyed(results, keys)


# ---- the union-find decoder as a policy and a teacher of the wide environment (include/deepq_hip.h dq_envb_uf_select, dq_envb_guided_select_uf;
# ---- csrc/env_wide_uf.hip) -----------------------------------------------------------------------------------------------------
WIDE_MAX_DEPTH = 16


def completed_from_state(state_row, d, legal_words):
    """The set of action indices in completed_actions of one lattice's row of VectorEnv.export_state() on the wide backend (dq_envb_export_state's layout:
    x[W] z[W] true[W] summed[W] acted[W] round completed[LW] legal[LW] meta volume[depth][W], W = ceil(d^2 / 64))."""
    W, LW = (int(d) * int(d) + 63) // 64, int(legal_words)
    o = 5 * W + 1
    words = [int(x) & (2 ** 64 - 1) for x in np.asarray(state_row).reshape(-1)[o:o + LW].tolist()]
    if len(words) != LW:
        raise ValueError(f"the state row is too short for d = {d} and {LW} legal words")
    return {64 * k + b for k, w in enumerate(words) for b in range(64) if (w >> b) & 1}


def guided_actions_wide(q, legal_words, teacher, eps, guide_share, masked_greedy, seed, env_id_base, t):
    """decoder.guided_actions for legal sets of any number of 64-bit words: the rule of dq_envb_guided_select_uf in numpy.  legal_words: [n, LW] (VectorEnv.legal
    of the wide backend; bit a of the set = action a); teacher: int [n], what uf_select_wide emits for the lattices as they stand; the other arguments and
    the result (actions int32 [n], guided flags uint8 [n]) are guided_actions'.  This loop is the one numpy statement of the selection rule (DESIGN.md
    section 28; on the device: csrc/common.h): decoder.guided_actions is this function on two words.  An empty legal set: an exploring lattice gets -1;
    the first maximum over the legal set (masked_greedy) has no candidate -- the kernels then write the scan's "no candidate" index 0x7fffffff, this
    function raises ValueError; no environment produces such a set (the identity is always legal)."""
    from . import _lib, _philox
    for name, v in (("eps", eps), ("guide_share", guide_share)):
        if not 0.0 <= float(v) <= 1.0:
            raise ValueError(f"guided_actions_wide: {name} must lie in [0, 1], not {v!r}")
    words = np.asarray(legal_words)
    if words.ndim != 2 or words.shape[1] < 1:
        raise ValueError(f"guided_actions_wide: legal_words must have shape [n, LW], got {words.shape}")
    words = np.ascontiguousarray(words).astype(np.int64, copy=False).view(np.uint64)
    n, LW = words.shape
    teacher = np.asarray(teacher).reshape(-1)
    if len(teacher) != n:
        raise ValueError(f"guided_actions_wide: {len(teacher)} teacher actions for {n} legal sets")
    t = int(t)
    ids = (int(env_id_base) + np.arange(n, dtype=np.uint64)) & np.uint64(0xFFFFFFFF)
    w0, w1, w2, _ = _philox.philox4x32(t & 0xFFFFFFFF, t >> 32, ids, _lib.STREAM_POLICY << 16, seed)
    explore = np.ones(n, dtype=bool) if q is None else w1.astype(np.uint64) < np.uint64(rate_threshold(eps))
    guided = explore & (w2.astype(np.uint64) < np.uint64(rate_threshold(guide_share)))
    if q is not None:
        q = np.asarray(q, dtype=np.float32)
        if q.ndim != 2 or q.shape[0] != n or not 1 <= q.shape[1] <= 64 * LW:
            raise ValueError(f"guided_actions_wide: q must have shape [{n}, num_actions <= {64 * LW}], got {q.shape}")
    actions = np.empty(n, dtype=np.int32)
    for i in range(n):
        if guided[i]:
            actions[i] = teacher[i]
            continue
        mask = sum(int(words[i, k]) << (64 * k) for k in range(LW))
        if explore[i]:
            members = [a for a in range(64 * LW) if (mask >> a) & 1]
            k = (int(w0[i]) * len(members)) >> 32
            actions[i] = members[k] if members else -1
        else:
            row = q[i]
            cand = [a for a in range(len(row)) if not masked_greedy or (mask >> a) & 1]
            actions[i] = max(cand, key=lambda a: (row[a], -a))                  # the larger value, the lower index among equals
    return actions, guided.astype(np.uint8)


def check_wide_policy_args(env, evaluator=None, chunk=DEFAULT_CHUNK):
    """Validates the lattice of a wide union-find evaluation without touching the library: a wide handle (else NotImplementedError, naming the narrow agent),
    odd d in 3 .. 15, volume_depth 1 .. 16, an evaluator of the same d and error model whose window covers the volume (else ValueError).  Returns
    (d, error_model, use_Y, volume_depth)."""
    if env is None:
        raise ValueError("an environment is needed: the policy plays it")
    v = getattr(env, "_v", env)
    d, model, use_Y, depth = lattice_of(v)
    if not getattr(v, "wide", False):
        raise NotImplementedError("WideUnionFindAgent plays the wide environment (backend='wide' / d >= 9); on the narrow one use "
                                  "decoder.MatchingAgent(method=\"union_find\")")
    check_wide_lattice(d, model)
    action_layers(model, use_Y)
    if not 1 <= depth <= WIDE_MAX_DEPTH:
        raise NotImplementedError(f"the wide union-find policy covers volume_depth 1..{WIDE_MAX_DEPTH}, not {depth}")
    check_chunk(chunk)
    if evaluator is not None:
        theirs = (getattr(evaluator, "d", None), getattr(evaluator, "error_model", None))
        window = getattr(evaluator, "window", None)
        if window is None or theirs != (d, model):
            raise ValueError(f"the evaluator must be a WideEvaluator of the environment's (d, error model) = {(d, model)}, not {theirs}")
        if int(window) < depth:
            raise ValueError(f"the evaluator's window {window} is below the environment's volume_depth {depth}")
    return d, model, use_Y, depth


class WideUnionFindAgent(MatchingAgent):
    """decoder.MatchingAgent(method="union_find") for the wide environment, any odd d in 3 .. 15: per agent step one dq_envb_uf_select launch (the next flip of
    the union-find frame of the lattice's current volume, then the identity) and one dq_envb_step with auto-reset.  test and test_error_rates return what
    MatchingAgent's return -- the same keys, quotas, block layout, record order and step cap, through episodes.py.  policy="identity": only ever the identity,
    the "no decoder" row on the same handle.  evaluator: a WideEvaluator of the environment's d and error model with window >= volume_depth (it stays
    open); default: one per call.  The decoder has no fallback, so last_inexact_steps is 0.  As a subclass it is accepted by EpsGreedyQPolicy(guide=...):
    DQNAgent.fit then runs DQNCore.guided_act_and_step_wide.  weights: VectorEnv.uf_select_wide's -- None (unit weights, the
    calls of before), a pair, one pair per lattice, or "rates": every select of test / test_error_rates and, as a guide, every guided step of fit
    decodes on the weighted graph; with "rates" test_error_rates gives every rate block its own pair in the same launches.  After a call last_weights
    holds what was used: None, a pair, or the sorted list of the lattices' distinct pairs.  The identity row takes no weights.  correlated (DESIGN.md
    section 26): VectorEnv.uf_select_wide's -- None, an integer w_corr beside a pair or per-lattice pairs, or "rates" beside weights None or "rates":
    every select and every guided step decodes in the three correlated passes; with "rates" test_error_rates gives every rate block its own triple
    (uf_weights_correlated) in the same launches.  last_weights then holds the triple or the sorted list of the distinct triples."""

    def __init__(self, evaluator=None, chunk=DEFAULT_CHUNK, policy="matching", weights=None, correlated=None):
        super().__init__(evaluator=evaluator, chunk=chunk, policy=policy)
        self.method = "union_find"
        self.weights = check_policy_weights(weights)
        if correlated is not None and is_correlated(self.weights):
            raise ValueError("weights are triples already: they take no correlated=")
        self.correlated = check_correlated(correlated, self.weights, rates=True)
        if (self.weights is not None or self.correlated is not None) and policy == "identity":
            raise ValueError("policy='identity' plays no decoder: it takes no weights")
        self.last_weights = None

    def _check_env(self, env):
        check_wide_policy_args(env, self.evaluator, self.chunk)
        check_policy_weights(self.weights, int(getattr(env, "_v", env).n_envs))

    def weights_for(self, env):
        """The agent's weights as VectorEnv.uf_select_wide / guided_select_wide take them on env, for a caller that makes many calls (DQNAgent.fit): None, the
        pair, "rates" (the environment keeps the uploaded array and follows set_rates), or the per-lattice pairs as ONE uint8 device tensor.  Validates the
        rows against env.n_envs (ValueError) before any library call."""
        v = getattr(env, "_v", env)
        w = check_policy_weights(self.weights, int(v.n_envs))
        if isinstance(w, np.ndarray):
            import torch
            w = torch.from_numpy(w).to(v.device)
        return w

    def select_kw(self, env):
        """What VectorEnv.uf_select_wide / guided_select_wide take on env beside their own arguments, for a caller that makes many calls: nothing without
        weights and correlated (the call of before, argument for argument), weights= alone as weights_for gives them, and with correlated= the pair with
        the integer, "rates" as the string (the environment keeps the uploaded triples and follows set_rates), or per-lattice pairs with their w_corr as
        ONE uint8 device tensor [n_envs, 3].  Validates before any library call (ValueError)."""
        w = self.weights_for(env)
        if self.correlated is None:
            return {} if w is None else dict(weights=w)
        if w is None or isinstance(w, (str, tuple)):
            return dict(correlated=self.correlated, **({} if w is None else dict(weights=w)))
        v = getattr(env, "_v", env)
        return dict(weights=v._wide_uf_weights(w, "WideUnionFindAgent", self.correlated))

    def evaluator_for(self, env):
        """(a WideEvaluator(d, error_model, window=volume_depth) of env's lattice, whether it was opened here and is the caller's to close): the agent's own
        where it was given one.  Validates like test(), before any library call."""
        d, model, _, depth = check_wide_policy_args(env, self.evaluator, self.chunk)
        check_policy_weights(self.weights, int(getattr(env, "_v", env).n_envs))
        if self.evaluator is not None:
            return self.evaluator, False
        v = getattr(env, "_v", env)
        return WideEvaluator(d, model, window=depth, chunk=min(self.chunk, int(v.n_envs)), device=v.device), True

    def _records(self, venv, quota, nb_max_episode_steps):
        """(records of episodes.episode_records, zeros int64 [N]) of one evaluation from a reset."""
        import torch
        from . import episodes
        dev, N = venv.device, int(venv.n_envs)
        decode = self.policy == "matching"
        ev, opened = self.evaluator_for(venv) if decode else (None, False)
        try:
            with torch.cuda.device(dev):
                action = torch.full((N,), int(venv.identity_index), dtype=torch.int32, device=dev)
                steps = [0]
                kw = self.select_kw(venv) if decode else {}                   # (no weights: the call of before, argument for argument)
                weights = kw.get("weights")
                if kw.get("correlated") == "rates":
                    ph, pm = venv.rates
                    pm = ph if pm is None else pm
                    scalar = np.ndim(ph) == 0 and np.ndim(pm) == 0
                    weights = rate_weights_correlated(*((float(ph), float(pm)) if scalar else
                                                        (np.broadcast_to(np.asarray(x, dtype=np.float64), (N,)) for x in (ph, pm))), venv.error_model, N)
                elif "correlated" in kw:
                    weights = weights + (kw["correlated"],)
                self.last_weights = weight_pairs(weights, venv.rates, venv.error_model, N) if weights is not None else None

                def step(k):
                    if decode:
                        venv.uf_select_wide(ev, out=action, **kw)
                    venv.step(action, auto_reset=True, write_obs=False)
                    steps[0] = k + 1
                    return venv.done, venv.was_reset, venv.reward, venv.lifetime

                venv.reset(write_obs=False)
                rec = episodes.episode_records(venv.L, dev, venv._stream, N, quota, step, None, nb_max_episode_steps)
                self.last_vector_steps = steps[0]
                return rec, np.zeros(N, dtype=np.int64)
        finally:
            if opened:
                ev.close()


# ---- batched agent decoding for any odd d in 3 .. 15 (include/deepq_hip.h dq_decode_wide_*; csrc/decode_wide.hip) ---------------------
DECODE_WIDE_BUDGET = 4 << 30                                      # device bytes a default chunk may ask for (rows + Q rows + the network's workspaces)
DECODE_WIDE_MIN_CHUNK = 64


def check_decode_wide_args(d, error_model, use_Y, volume_depth, shape, max_actions=None):
    """Validates a decode_wide request without touching the library: odd d in 3 .. 15, volume_depth 1 .. 16, max_actions in 1 .. num_actions - 1, the
    syndromes [N, depth, d+1, d+1] or one volume [depth, d+1, d+1] (else ValueError).  Returns (n_volumes, single, num_actions, max_actions)."""
    d, error_model = check_wide_lattice(d, error_model)
    layers = action_layers(error_model, use_Y)
    if not is_int(volume_depth) or not 1 <= volume_depth <= WIDE_MAX_DEPTH:
        raise ValueError(f"decode_wide covers volume_depth 1..{WIDE_MAX_DEPTH}, not {volume_depth!r}")
    volume_depth = int(volume_depth)
    num_actions = layers * d * d + 1
    if max_actions is None:
        max_actions = num_actions - 1
    if not is_int(max_actions) or not 1 <= max_actions <= num_actions - 1:
        raise ValueError(f"max_actions must be an integer in 1..{num_actions - 1}, not {max_actions!r}")
    shape = tuple(int(x) for x in shape)
    grid = (volume_depth, d + 1, d + 1)
    if len(shape) == 3 and shape == grid:
        return 1, True, num_actions, int(max_actions)
    if len(shape) == 4 and shape[1:] == grid and shape[0] >= 1:
        return shape[0], False, num_actions, int(max_actions)
    raise ValueError(f"faulty syndromes must have shape [N, {volume_depth}, {d + 1}, {d + 1}] or [{volume_depth}, {d + 1}, {d + 1}], got {shape}")


def decode_wide_footprint(input_shape, c_layers, ff_layers, num_actions, dueling=True):
    """Device bytes one volume of a chunk costs: its observation row, its Q row, and the per-layer network's workspaces (csrc/qnet.hip keeps three float
    buffers -- two activations and a gradient -- per layer output)."""
    c, h, w = (int(x) for x in input_shape)
    row, outs = c * h * w, 0
    for cout, k, s in ((int(l[0]), int(l[1]), int(l[2])) for l in c_layers):
        h, w = (h - k) // s + 1, (w - k) // s + 1
        outs += cout * h * w
    outs += sum(int(l[0]) for l in ff_layers) + int(num_actions) + (int(num_actions) + 1 if dueling else 0)
    return row + 4 * int(num_actions) + 12 * outs


def default_decode_wide_chunk(input_shape, c_layers, ff_layers, num_actions, dueling=True):
    """The largest power of two of volumes whose footprint stays within DECODE_WIDE_BUDGET, between DECODE_WIDE_MIN_CHUNK and decoder.DEFAULT_CHUNK."""
    fit = DECODE_WIDE_BUDGET // decode_wide_footprint(input_shape, c_layers, ff_layers, num_actions, dueling)
    chunk = DECODE_WIDE_MIN_CHUNK
    while 2 * chunk <= min(fit, DEFAULT_CHUNK):
        chunk *= 2
    return chunk


class _DeviceView:
    """A typed view of device memory the library owns, for torch.as_tensor (the __cuda_array_interface__ protocol); for reading."""

    def __init__(self, pointer, shape, typestr):
        self.__cuda_array_interface__ = dict(shape=tuple(shape), typestr=typestr, data=(int(pointer), False), version=2, strides=None)


class WideBatchDecoder:
    """decoder.BatchDecoder for any odd d in 3 .. 15: decodes syndrome volumes with a Q-network's weights in chunks of at most `chunk` volumes.  Owns a
    QNetwork handle of max_batch = chunk and a dq_decode_wide handle.  The environment's action planes and uint8 observation rows only.  chunk=None: the
    largest power of two whose rows, Q rows and network workspaces fit DECODE_WIDE_BUDGET (default_decode_wide_chunk).  Scoring is
    DQNAgent.decode_benchmark_wide."""

    def __init__(self, input_shape, c_layers, ff_layers, num_actions, d, error_model, use_Y, volume_depth, dueling=True, masked_greedy=False,
                 max_actions=None, chunk=None, device=None):
        import torch
        from . import _lib
        from .qnet import QNetwork
        _, _, n_act, max_actions = check_decode_wide_args(d, error_model, use_Y, volume_depth, (volume_depth, d + 1, d + 1), max_actions)
        layers = action_layers(error_model, use_Y)
        if int(num_actions) != n_act or tuple(input_shape) != (volume_depth + layers, 2 * d + 1, 2 * d + 1):
            raise ValueError(f"the network ({tuple(input_shape)} -> {num_actions} actions) does not fit the lattice (d = {d}, {error_model}, "
                             f"volume_depth = {volume_depth})")
        chunk = default_decode_wide_chunk(input_shape, c_layers, ff_layers, num_actions, dueling) if chunk is None else check_chunk(chunk)
        self.d, self.error_model, self.use_Y, self.volume_depth = int(d), error_model, bool(use_Y), int(volume_depth)
        self.masked_greedy, self.max_actions, self.chunk, self.num_actions = bool(masked_greedy), max_actions, chunk, n_act
        self._h = None
        self.net = QNetwork(input_shape, c_layers, ff_layers, num_actions, dueling=dueling, max_batch=self.chunk, device=device)
        self.device = self.net.device
        cfg = _lib.DecodeCfg(d=self.d, volume_depth=self.volume_depth, error_model=MODELS[error_model], use_Y=int(self.use_Y),
                             masked_greedy=int(self.masked_greedy), max_actions=self.max_actions, action_planes=_lib.DECODE_PLANES_ENV,
                             obs_form=_lib.DECODE_OBS_UINT8)
        self.L = _lib.lib()
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(self.L.dq_decode_wide_create(ctypes.byref(cfg), self.chunk, ctypes.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self.L.dq_decode_wide_destroy(self._h)
            self._h = None
        if getattr(self, "net", None) is not None:
            self.net.close()
            self.net = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self):
        import torch
        return torch.cuda.current_stream(self.device).cuda_stream

    def _input(self, syndromes):
        import torch
        n, single, _, _ = check_decode_wide_args(self.d, self.error_model, self.use_Y, self.volume_depth, tuple(syndromes.shape), self.max_actions)
        check_binary(syndromes)
        t = syndromes if isinstance(syndromes, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(syndromes)))
        t = t.to(device=self.device, dtype=torch.uint8).reshape(n, self.volume_depth, self.d + 1, self.d + 1).contiguous()
        return t, n, single

    def outputs(self, n):
        """Empty (corrections, n_corrections, frame, status) device tensors for n volumes."""
        import torch
        dev = self.device
        return (torch.empty((n, self.max_actions), dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev),
                torch.empty((n, self.d, self.d), dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.uint8, device=dev))

    def decode_into(self, params, packed, syn, m, corr, ncorr, frame, status):
        """One dq_decode_wide_run over m <= chunk volumes already on the device; returns the iterations."""
        from . import _lib
        it = ctypes.c_int(0)
        _lib.check(self.L.dq_decode_wide_run(self._h, self.net._h, _lib.ptr(params), _lib.ptr(packed), _lib.ptr(syn), m, _lib.ptr(corr), _lib.ptr(ncorr),
                                             _lib.ptr(frame), _lib.ptr(status), ctypes.byref(it), self._stream()))
        return int(it.value)

    def decode(self, params, syndromes, to_host=True):
        """params: float32 device tensor of the network's flat parameters (Keras order).  syndromes: numpy or torch (CPU or device), 0/1 cells,
        [N, volume_depth, d+1, d+1] or one volume.  Returns a decoder.DecodeResult; to_host=False leaves the outputs as device tensors."""
        import torch
        from .decoder import DecodeResult
        syn, n, single = self._input(syndromes)
        corr, ncorr, frame, status = self.outputs(n)
        iters = []
        with torch.cuda.device(self.device):
            packed = self.net.pack(params)
            for s in range(0, n, self.chunk):
                m = min(self.chunk, n - s)
                iters.append(self.decode_into(params, packed, syn[s:s + m], m, corr[s:s + m], ncorr[s:s + m], frame[s:s + m], status[s:s + m]))
        out = [corr, ncorr, frame, status]
        if to_host:
            out = [x.cpu().numpy() for x in out]
        if single:
            out = [x[0] for x in out]
        return DecodeResult(*out, iterations=iters)

    # -- the stepping pair (dq_decode_wide_pack / dq_decode_wide_step): the bookkeeping driven by the caller's Q rows ------------------------------
    def pack(self, syndromes):
        """Starts a decode of n <= chunk volumes; returns the (corrections, n_corrections, frame, status) device tensors the steps write."""
        import torch
        from . import _lib
        syn, n, _ = self._input(syndromes)
        if n > self.chunk:
            raise ValueError(f"pack takes at most chunk = {self.chunk} volumes, not {n}")
        out = self.outputs(n)
        with torch.cuda.device(self.device):
            _lib.check(self.L.dq_decode_wide_pack(self._h, _lib.ptr(syn), n, *(_lib.ptr(x) for x in out), self._stream()))
        self._stepping = (syn,) + out                             # (the handle writes them until the decode ends)
        return out

    def step(self, q):
        """One select + compact with q float32 [n_active, num_actions], rows in active-list order; returns the next active count."""
        import torch
        from . import _lib
        q = torch.as_tensor(q, dtype=torch.float32, device=self.device).contiguous()
        _, n_active = self.active(count_only=True)
        if n_active and tuple(q.shape) != (n_active, self.num_actions):       # (no volume active: the library says so, DQ_ERR_STATE)
            raise ValueError(f"q must have shape {(n_active, self.num_actions)}, got {tuple(q.shape)}")
        nxt = ctypes.c_int(0)
        with torch.cuda.device(self.device):
            _lib.check(self.L.dq_decode_wide_step(self._h, _lib.ptr(q), ctypes.byref(nxt), self._stream()))
        return int(nxt.value)

    def active(self, count_only=False):
        """(the current active list as an int32 device tensor, its length)."""
        import torch
        from . import _lib
        p, n = ctypes.c_void_p(), ctypes.c_int(0)
        _lib.check(self.L.dq_decode_wide_active(self._h, ctypes.byref(p), ctypes.byref(n)))
        if count_only or n.value == 0:
            return None, int(n.value)
        return torch.as_tensor(_DeviceView(p.value, (n.value,), "<i4"), device=self.device), int(n.value)

    def rows(self, n):
        """The observation rows of volumes 0 .. n - 1 as a uint8 device tensor [n, depth + layers, 2d+1, 2d+1] (a view of the handle's buffer)."""
        import torch
        from . import _lib
        p, nb = ctypes.c_void_p(), ctypes.c_int(0)
        _lib.check(self.L.dq_decode_wide_rows(self._h, ctypes.byref(p), ctypes.byref(nb)))
        side = 2 * self.d + 1
        return torch.as_tensor(_DeviceView(p.value, (int(n), nb.value // (side * side), side, side), "|u1"), device=self.device)

    def words(self, n):
        """(legal, completed) words of volumes 0 .. n - 1 as int64 device tensors [n, legal_words] (views; bit a of the set = action a)."""
        import torch
        from . import _lib
        pl, pc, lw = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_int(0)
        _lib.check(self.L.dq_decode_wide_words(self._h, ctypes.byref(pl), ctypes.byref(pc), ctypes.byref(lw)))
        return tuple(torch.as_tensor(_DeviceView(p.value, (int(n), lw.value), "<i8"), device=self.device) for p in (pl, pc))


def decode_lattice_of(lattice):
    """`lattice`: (d, error_model, use_Y, volume_depth), or an environment of either backend.  Returns (d, error_model, use_Y, volume_depth, what
    check_wide_experiment_args takes as its lattice)."""
    if isinstance(lattice, (tuple, list)):
        if len(lattice) != 4:
            raise ValueError(f"lattice must be (d, error_model, use_Y, volume_depth) or an environment, not {lattice!r}")
        d, model = check_wide_lattice(lattice[0], lattice[1])
        return d, model, bool(lattice[2]), lattice[3], (d, model)
    v = getattr(lattice, "_v", lattice)
    if v is None or not all(hasattr(v, k) for k in ("d", "error_model", "use_Y", "volume_depth")):
        raise ValueError(f"lattice must be (d, error_model, use_Y, volume_depth) or an environment, not {lattice!r}")
    d, model = check_wide_lattice(int(v.d), str(v.error_model))
    return d, model, bool(v.use_Y), int(v.volume_depth), lattice


def check_decode_benchmark_wide_args(lattice, n_volumes, rates=None, p_phys=None, p_meas=None, seed=None, env_id_base=0, max_actions=None, chunk=None,
                                     baseline=None, final_round="faulty", referee=None):
    """Validates a decode_benchmark_wide request without touching the library.  Returns (d, error_model, use_Y, depth, max_actions, n, p_phys, p_meas,
    seed, base, block, keys, closed): memory_experiment_wide's conventions for the rates, the seed and the blocks (check_wide_experiment_args with
    rounds = window = commit = volume_depth)."""
    check_referee(referee)
    d, model, use_Y, depth, lat = decode_lattice_of(lattice)
    _, _, _, max_actions = check_decode_wide_args(d, model, use_Y, depth, (depth, d + 1, d + 1), max_actions)
    if baseline is not None and baseline != "union_find":
        raise ValueError(f"decode_benchmark_wide: baseline must be None or 'union_find', not {baseline!r}")
    closed = check_final_round(final_round)
    _, _, _, _, _, n, ph, pm, seed, base, blk, keys, _ = check_wide_experiment_args(
        lat, n_volumes, depth, depth, depth, rates, p_phys, p_meas, seed, env_id_base, DEFAULT_CHUNK if chunk is None else chunk)
    return d, model, use_Y, int(depth), max_actions, n, ph, pm, seed, base, blk, keys, closed


def score_decode_wide(dec, params, n, ph, pm, seed, base, blk, keys, baseline=None, no_decoder=False, final_round="faulty", return_volumes=False,
                      timings=None, referee=None, weights=None, correlated=None):
    """The loop behind DQNAgent.decode_benchmark_wide for a validated request: per chunk ONE dq_wide_uf_run (T = window = commit = volume_depth, with
    syndromes) yields the agent's input, the hidden state and the union-find frame of the same volumes; then dq_decode_wide_run, dq_wide_uf_verdict
    and dq_decode_count with the agent's status and correction count.  referee=None: no referee is consulted, alive := success; referee="matching" or
    "uf" (the union-find referee; no flags): the verdicts of all three rows (the agent's, the union-find baseline's, no_decoder's)
    go through the refereed verdict launch and each row's
    EvalResult.inexact counts its flagged volumes.  weights (validated: None, a pair or "rates"): the sampling launch is
    dq_wide_uf_run_weighted, as memory_experiment_wide's -- the volumes and the hidden state do not depend on the weights, only the union-find frame does, so
    the agent's row keeps its bits; the baseline's EvalResult of every block reports .weights.  correlated (validated: None, an integer or "rates";
    DESIGN.md section 25): dq_wide_uf_run_correlated, and .weights is the triple."""
    import torch
    from .decoder import DecodeResult
    refereed = check_referee(referee)
    d, depth, dev = dec.d, dec.volume_depth, dec.device
    if correlated == "rates":
        weights = rate_weights_correlated(ph, pm, dec.error_model, n)
    elif isinstance(weights, str):                                    # "rates"
        weights = rate_weights(ph, pm, dec.error_model, n)
    else:
        weights = with_correlated(weights, correlated)
    used = weights                                                    # None, the pair / triple, or uint8 [n, 2] / [n, 3] on the host
    if isinstance(weights, np.ndarray):
        weights = torch.from_numpy(weights).to(device=dev)
    step = min(dec.chunk, n)
    ev = WideEvaluator(d, dec.error_model, depth, chunk=step, device=dev)
    closed = closed_kw(final_round)
    try:
        rows = n if return_volumes else step
        syn = torch.empty((rows, depth, d + 1, d + 1), dtype=torch.uint8, device=dev)
        hid = torch.empty((rows, d, d), dtype=torch.uint8, device=dev)
        uf_frame = torch.empty((rows, d, d), dtype=torch.uint8, device=dev)
        triv = torch.empty(rows, dtype=torch.uint8, device=dev)
        verd = torch.empty(rows, dtype=torch.uint8, device=dev)
        verd2 = torch.empty(step, dtype=torch.uint8, device=dev)
        corr, ncorr, frame, status = dec.outputs(rows)
        uf_status = torch.full((step,), STATUS_IDENTITY, dtype=torch.uint8, device=dev)
        flags = torch.empty(step, dtype=torch.uint8, device=dev) if refereed else None
        ref_kw = dict(referee=referee, inexact=flags) if refereed else {}     # (no referee: the call of before, argument for argument)
        iters = []

        def run(m, s, sl, a, b):
            ev.run_into(m, depth, depth, base + s, seed, a, b, hid[sl], triv[sl], uf_frame[sl], syndromes=syn[sl], **closed, **weights_kw(weights, dev, s, m))

        def decode(m, sl):
            iters.append(dec.decode_into(params, packed, syn[sl], m, corr[sl], ncorr[sl], frame[sl], status[sl]))

        def agent(m, sl):
            ev.verdict_into(hid[sl], frame[sl], m, verd[sl], **ref_kw)
            return verd[sl], triv[sl], status[sl], ncorr[sl], flags

        def union_find(m, sl):
            ev.verdict_into(hid[sl], uf_frame[sl], m, verd2[:m], **ref_kw)
            return verd2[:m], triv[sl], uf_status[:m], corrected_cells(uf_frame[sl]), flags

        def uncorrected(m, sl):
            uncorrected_into(ev, hid[sl], m, verd2[:m], flags, referee or "matching")
            return verd2[:m], triv[sl], None, None, flags

        with torch.cuda.device(dev):
            packed = dec.net.pack(params)
            results = score_chunks(ev, dev, n, ph, pm, blk, run, [agent, union_find] if baseline else [agent], uncorrected if no_decoder else None,
                                   keep=return_volumes, decode=decode, phases=("run", "decode"), timings=timings)
    finally:
        ev.close()
    if return_volumes:
        r = results[0][0]
        r.volumes, r.hidden, r.trivial, r.verdict = syn, hid, triv, verd
        r.decode = DecodeResult(corr, ncorr, frame, status, iterations=iters)
    if baseline:
        for k, r in enumerate(results[1]):                            # (a block of rates=[...] holds one rate pair, so one pair of weights)
            r.weights = weight_pairs(used if used is None or isinstance(used, tuple) else used[k * blk:(k + 1) * blk])
    out = tuple(keyed(x, keys) for x in results)
    return out if baseline else out[0]
