"""The replay ring of the device loop (keras-rl's SequentialMemory(limit, window_length=1), TRAIN:109): time-major tensors

    store    int32 [T, N, patch_stride] patch words (compact) or uint8 [T, N, C, H, W] images
    action   int32 [T, N]     reward float [T, N]     terminal uint8 [T, N]

row (t, i) = what lattice i saw / did / received at vector step t; its successor observation is row (t+1, i).  `cur` is the slot
of the newest observation (no action recorded in it yet), `filled` the number of slots written.  ReplayRing is the ONE place that
knows the fields: slot arithmetic, the decoded view of a compact ring, the pickled form, ring-to-ring copies and the scratch ring of
an evaluation all live here, so a new field is added here and nowhere else.  Pure torch: a ring on the CPU works (tests)."""
import numpy as np
import torch


_PER_STEP = (("action", torch.int32), ("reward", torch.float32), ("terminal", torch.uint8))      # the [T, N] tensors of a ring, in pickled order


class ObsRingView:
    """`ReplayRing.obs` of a ring that holds PATCH WORDS: the padded uint8 observations [T, N, C, H, W] the reference's memory would
    hold (SequentialMemory stores the env's board_state, TRAIN:109), decoded on demand by `patch_to_obs` (the image is a fixed
    function of the words).  Indexing returns decoded tensors; copy_() encodes through `obs_to_patch`.  Tests, pickling and
    diagnostics only -- nothing in the loop touches it."""

    dtype = torch.uint8

    def __init__(self, ring, patch_to_obs, obs_to_patch):
        self._r, self._decode, self._encode = ring, patch_to_obs, obs_to_patch

    @property
    def shape(self):
        return torch.Size(tuple(self._r.store.shape[:2]) + tuple(self._r.obs_shape))

    @property
    def device(self):
        return self._r.store.device

    def __getitem__(self, idx):
        return self._decode(self._r.store[idx])

    def clone(self):
        return self._decode(self._r.store)

    def cpu(self):
        return self.clone().cpu()

    def copy_(self, src):
        if isinstance(src, ObsRingView):
            self._r.store.copy_(src._r.store)
        else:
            self._r.store.copy_(self._encode(torch.as_tensor(src).to(self.device)))
        return self

    def __eq__(self, other):
        return self.clone() == (other.clone() if isinstance(other, ObsRingView) else other)


class ReplayRing:
    def __init__(self, T, N, obs_shape, patch_to_obs, obs_to_patch, patch_stride=None, device="cpu"):
        """patch_stride: words per observation of a compact ring; None: the uint8 ring.  patch_to_obs / obs_to_patch: the
        environment's pair (env.py), needed by either form (a uint8 ring loads the pickle of a compact one)."""
        self.T, self.N, self.obs_shape, self.compact = int(T), int(N), tuple(obs_shape), patch_stride is not None
        self.patch_to_obs, self.obs_to_patch, self.patch_stride = patch_to_obs, obs_to_patch, patch_stride
        if self.compact:
            self.store = torch.zeros((self.T, self.N, patch_stride), dtype=torch.int32, device=device)
        else:
            self.store = torch.zeros((self.T, self.N) + self.obs_shape, dtype=torch.uint8, device=device)
        for name, dtype in _PER_STEP:
            setattr(self, name, torch.zeros((self.T, self.N), dtype=dtype, device=device))
        self.cur, self.filled = 0, 0
        self.presampled = None       # (update number, head slot, filled slots) a look-ahead minibatch draw was made for

    def scratch(self, T=3):
        """An empty ring of T slots for the same lattices (DQNCore.begin_eval: evaluation steps store nothing in the memory)."""
        return ReplayRing(T, self.N, self.obs_shape, self.patch_to_obs, self.obs_to_patch, self.patch_stride, self.store.device)

    # -- slot arithmetic ----------------------------------------------------------------------------------------------------
    def next_slot(self, n=1):
        """The slot n vector steps after `cur` (n = -1: the one before it)."""
        return (self.cur + n) % self.T

    def filled_after(self, n=1):
        return min(self.T, self.filled + n)

    def advance(self):
        """One vector step was recorded: its successor observation is the newest slot."""
        self.cur, self.filled = self.next_slot(), self.filled_after()

    @property
    def nb_entries(self):
        return min(self.filled, self.T) * self.N

    @property
    def obs(self):
        """uint8 [T, N, C, H, W]: the tensor itself, or -- compact -- a view that decodes the patch words on demand."""
        return ObsRingView(self, self.patch_to_obs, self.obs_to_patch) if self.compact else self.store

    @obs.setter
    def obs(self, value):
        if self.compact:
            raise AttributeError("compact ring: assign patch_ring")
        self.store = value

    @property
    def patch(self):
        """int32 [T, N, patch_stride]: the compact ring's words; None where the ring holds uint8 images."""
        return self.store if self.compact else None

    @patch.setter
    def patch(self, value):
        if not self.compact:
            raise AttributeError("uint8 ring: assign obs_ring")
        self.store = value

    # -- the pickled form (SequentialMemory), ring-to-ring copies -------------------------------------------------------------
    def state(self):
        s = dict(obs_shape=tuple(self.obs.shape), **{name: getattr(self, name).cpu().numpy() for name, _ in _PER_STEP}, cur=self.cur, filled=self.filled)
        if self.compact:             # patch words are pickled as they are, d * d words per observation
            s["patch"] = self.store.cpu().numpy()
        else:
            s["obs"] = np.packbits(self.store.cpu().numpy(), axis=None)
        return s

    def load_state(self, s):
        """Takes over a state() dict of a ring of the same [T, N, C, H, W]; returns False (ring untouched) for another shape."""
        if s is None or tuple(s["obs_shape"]) != tuple(self.obs.shape):
            return False
        if "patch" in s:
            patch = torch.from_numpy(s["patch"]).to(self.store.device)
            if self.compact and tuple(patch.shape) == tuple(self.store.shape):
                self.store.copy_(patch)
            else:
                self.obs.copy_(self.patch_to_obs(patch))
        else:
            n = int(np.prod(s["obs_shape"]))
            self.obs.copy_(torch.from_numpy(np.unpackbits(s["obs"], count=n).reshape(s["obs_shape"])))
        for name, _ in _PER_STEP:
            getattr(self, name).copy_(torch.from_numpy(s[name]))
        self.cur, self.filled, self.presampled = int(s["cur"]), int(s["filled"]), None
        return True

    def copy_from(self, other):
        """Takes over another ring's transitions (either form); returns False (ring untouched) where the shapes do not fit."""
        if tuple(other.obs.shape) != tuple(self.obs.shape):
            return False
        if self.compact and other.compact:
            self.store.copy_(other.store)
        else:
            self.obs.copy_(other.obs[:])
        for name, _ in _PER_STEP:
            getattr(self, name).copy_(getattr(other, name))
        self.cur, self.filled, self.presampled = other.cur, other.filled, None
        return True
