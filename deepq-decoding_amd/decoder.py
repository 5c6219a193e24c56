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

import numpy as np

STATUS_IDENTITY, STATUS_REPEAT, STATUS_STOPPED = 1, 2, 3          # include/deepq_hip.h DQ_DECODE_*
STATUS_NAMES = {STATUS_IDENTITY: "identity", STATUS_REPEAT: "repeat", STATUS_STOPPED: "stopped"}
PLANES = {"environment": 0, "readme": 1}
OBS_FORMS = {"uint8": 0, "patch": 1}
MODELS = {"X": 0, "DP": 1, "IIDXZ": 2}
DEFAULT_CHUNK = 65536


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
