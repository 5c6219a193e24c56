"""Device-resident DQN loop over a batch of lattices: act -> environment step -> replay ring -> update.

This is the vectorised form of the loop keras-rl runs one lattice / one minibatch at a time
(`Agent.fit` + `DQNAgent.forward/backward`, call site
/root/reference/cluster_scripts/d5_dp/0.001/Single_Point_Training_Script.py:138-152).  With one lattice it
performs exactly that sequence per step; with N lattices every launch handles all of them and nothing is
copied to the host inside a step.

The transitions live in `DQNCore.ring`, a replay.ReplayRing (time-major device tensors; its fields, slot arithmetic, pickled
form and the scratch ring of an evaluation are that class's business).  The environment kernel writes the new observation
straight into slot t+1, so there is no append copy; a lattice that terminated spends its next step being reset (keras-rl's
extra forward/backward on the terminal observation), which is what makes keras-rl's "skip entries whose predecessor was
terminal" sampling rule carry over unchanged.  An update is one procedure (`_learn`) whatever the number of GPUs: TD job,
form of the gradient exchange (`_exchange_form`), backward, exchange, optimizer step, repack.
"""
import contextlib
import ctypes
import os

import numpy as np
import torch

from . import _lib, dist as _dist, qnet as _q
from ._lib import check, ptr
from .replay import ObsRingView, ReplayRing      # (ObsRingView: re-exported)


MIN_FILLED = 4      # ring slots an update needs: keras-rl asserts nb_entries >= window_length + 2 (csrc/common.h dq_replay_row)


class _TargetAhead:
    """State of DQ_TARGET_AHEAD=1 (off by default): the extra updates' TARGET forwards on a second stream.  The target network does not change
    inside a vector step and the extra updates' rows are drawn by one launch in front of them, so Q_target(s1) of update i needs nothing
    update i - 1 produces: a second network handle evaluates it on `stream`, released by a mark inside update i - 1's backward
    (dq_qnet_mark_conv_backward) and handed to update i's TD launch by an event.  Bit-identical results (tests/test_agent_gpu.py) and SLOWER on
    one MI355X, 138.5 against 123.9 us per update: the two event hand-offs cost more than the 10 us they move (NOTEBOOK.md Round 5 section 3)."""

    def __init__(self, net, device):
        self.net, self.stream = net, torch.cuda.Stream(device=device)      # (a network handle of its own: its own per-job scratch)
        self.e_rows = torch.cuda.Event()             # behind the launch that drew the updates' rows
        self.ready, self.marks = [], []              # per update: "Q_target(s1) ready" event, mark inside the backward
        self.q1 = None                               # Q_target(s1) rows [k - 1][B][A]


class _SideStream:
    """A second stream and the events that order it against the step's own.  DQ_ENV_STREAM=1 (e_fwd, e_env): the environment launch of a fused
    step does not feed the same step's backward (keras-rl's sampling range), so it CAN run beside the backward chain -- 0.299 ms per step against
    0.279 on one stream, the two hand-offs cost more than the 15 us launch they hide: off by default.  DQ_DIST_MODE=overlap (e_dense, e_ar): the
    dense range's all-reduce (DQNCore._exchange)."""

    def __init__(self, device, *events):
        self.stream, self.inflight = torch.cuda.Stream(device=device), False
        for name in events:
            setattr(self, name, torch.cuda.Event())


def _ring_field(name):
    """DQNCore.<attribute> = self.ring.<name>, for callers outside this module (the loop itself reads self.ring)."""
    return property(lambda self: getattr(self.ring, name), lambda self, value: setattr(self.ring, name, value))


# The shared ends of DQNCore's acting steps.  Plain functions of the core (`self`), not methods: they need its attributes only, and the tests drive
# the acting steps on stand-in objects that carry those attributes without being a DQNCore.
def _step_taken(self, cur, record_stats):
    """The tail of every acting step.  The episode bookkeeping of the step that filled slot `cur` rides on the next update's TD launch
    (dq_td_update_stats) when an update follows, else it is launched on its own; the ring moves on."""
    self._stats_pending = (cur,) if record_stats else None
    if record_stats and not self.defer_stats:
        self._flush_stats()
    self.ring.advance()
    self.vector_steps += 1


def _guided_head(self):
    """The head of the two guided acting steps: the previous step's bookkeeping, the Q forward on the current observations, the flags buffer.
    Returns (current slot, next slot, q, flags)."""
    self._flush_stats()
    cur, nxt = self.ring.cur, self.ring.next_slot()
    q = self.net.forward_multi([self._obs_job(params=self.params, slot=cur, batch=self.N, out=self.q_act, packed=self.params_pk)])[0]
    if self._guide_flags is None:
        self._guide_flags = torch.zeros((2, self.N), dtype=torch.uint8, device=self.device)
    return cur, nxt, q, self._guide_flags


class DQNCore:
    def __init__(self, env, net, batch_size=32, memory_limit=50000, gamma=0.99, lr=1e-3, beta_1=0.9, beta_2=0.999, epsilon=1e-7,
                 target_model_update=10000, enable_double_dqn=True, seed=None, rank=0, world_size=1, process_group=None,
                 params=None, compact=None, delta_clip=np.inf):
        """delta_clip: keras-rl's DQNAgent(delta_clip) -- inf (the reference's setting) trains on the squared TD error, a finite value > 0 on the
        Huber loss at that delta (include/deepq_hip.h dq_td_job.delta_clip), on every update path."""
        self.env, self.net = env, net
        self.delta_clip = _q.check_delta_clip(delta_clip)
        self.N, self.A = env.n_envs, env.num_actions
        assert net.n_actions == self.A and tuple(net.input_shape) == tuple(env.obs_shape)
        self.device = env.device
        self.batch_size = int(batch_size)
        assert self.batch_size <= net.max_batch and self.N <= net.max_batch
        self.gamma, self.lr, self.beta_1, self.beta_2, self.epsilon = gamma, lr, beta_1, beta_2, epsilon
        self.target_model_update = target_model_update
        self.enable_double_dqn = enable_double_dqn
        self.seed = tuple(env.seed) if seed is None else tuple(seed)
        self.rank, self.world_size, self.pg = rank, world_size, process_group
        self.last_index = None       # rows of the most recent update (self.index, or a row of _index_multi)
        self._index_multi = None     # [k - 1][B] rows of the extra updates of a vector step (_extra_updates)
        self.target_ahead = os.environ.get("DQ_TARGET_AHEAD", "0") == "1"
        self._side = None            # DQ_TARGET_AHEAD's state (_TargetAhead), created at its first use
        self.pair_targets = os.environ.get("DQ_PAIR_TARGETS", "1") != "0"      # extra updates in pairs (_extra_updates); 0: three forwards per launch pair
        self._q1_pair = None
        self._rccl, self._rccl2, self._rccl_tried = None, None, False       # the learner's own RCCL communicator (dist.make_rccl), created at the first several-GPU update
        self.L = _lib.lib()
        dev = self.device
        # ring
        self._wide = bool(getattr(env, "wide", False))       # lattices beyond d = 7 (csrc/env_big.hip)
        C = env.obs_shape[0]
        # Compact observations (include/deepq_hip.h dq_env_patch_output, dq_qnet_set_patch_input): the ring holds d * d patch words per
        # transition (128 bytes at d = 5 instead of the 847-byte padded image; 2^20 transitions: 134 MB instead of 0.9 GB), the environment
        # writes them, the first convolution reads them.  Where the fused chains and the one-word-per-plane environment cover the
        # configuration; DQ_COMPACT_OBS=0 (or compact=False) keeps the uint8 ring.
        if compact is None:
            compact = os.environ.get("DQ_COMPACT_OBS", "1") != "0"
        compact = bool(compact and not self._wide and getattr(env, "patch_supported", False) and net.fused_backward_supported
                       and net.fused_enabled and C == env.volume_depth + env.n_action_layers and net.c_layers[0][1:] == [3, 2])
        if compact:
            try:
                net.set_patch_input(env.volume_depth, env.patch_stride)        # (before the first pack(): the packed buffer carries the compact kernel)
            except _lib.DeepQError:
                compact = False
        self.ring = ReplayRing(max(MIN_FILLED, int(memory_limit) // self.N + 1), self.N, env.obs_shape, env.patch_to_obs, env.obs_to_patch,
                               env.patch_stride if compact else None, dev)
        self._train_ring = None      # (the training ring, started) while an evaluation runs on a scratch ring (begin_eval)
        # parameters
        self.params = net.init_params(self.seed) if params is None else params
        _dist.broadcast_(self.params, src=0, group=self.pg)
        self.target = self.params.clone()
        # f16 pieces of the weights for the fused chains: packed once per parameter change (repack()), shared by every forward
        self.params_pk = net.pack(self.params)
        self.target_pk = None if self.params_pk is None else self.params_pk.clone()
        self.m = torch.zeros_like(self.params)
        self.v = torch.zeros_like(self.params)
        self.grads = torch.zeros_like(self.params)
        # scratch
        self.q_act = torch.zeros((self.N, self.A), dtype=torch.float32, device=dev)
        B = self.batch_size
        self.index = torch.zeros(B, dtype=torch.int32, device=dev)         # rows of the update in progress
        self._index_next = torch.zeros(B, dtype=torch.int32, device=dev)   # rows drawn ahead by an environment launch (ring.presampled)
        self.q1_online = torch.zeros((B, self.A), dtype=torch.float32, device=dev)
        self.q1_target = torch.zeros((B, self.A), dtype=torch.float32, device=dev)
        self.q0 = torch.zeros((B, self.A), dtype=torch.float32, device=dev)
        self.y = torch.zeros(B, dtype=torch.float32, device=dev)
        self.dq = torch.zeros((B, self.A), dtype=torch.float32, device=dev)
        self.metrics = torch.zeros(_q.TD_METRICS_FLOATS, dtype=torch.float32, device=dev)
        self.stats = torch.zeros(4, dtype=torch.int64, device=dev)
        self._stats_pending = None   # episode bookkeeping not yet launched (slot,)
        self.defer_stats = True      # act_and_step leaves the bookkeeping launch to the next update() (dq_post_step) / act / read_stats
        self._metrics_stale = False
        self.vector_steps = 0        # policy / environment counter
        self.updates = 0             # optimizer steps taken
        self.started = False
        self._env_side = _SideStream(dev, "e_fwd", "e_env") if os.environ.get("DQ_ENV_STREAM", "0") == "1" else None
        # step_and_update on one GPU: the environment launch rides on the dense backward's first kernel (DQ_RIDE_ENV=0: separate launches)
        self.ride_env = os.environ.get("DQ_RIDE_ENV", "1") != "0"
        # DQ_TD_AUTOSCALE=1 (or auto_scale = True): the fused backward's gradient scale MEASURED from every minibatch's TD errors (dq_td_job.auto_scale: one
        # small launch per update, +3 us; any finite TD error is carried -- keras-rl's delta_clip = inf).  Default: the host-known scale (TD errors up to
        # several thousand -- the reference's recorded losses stay below 160 --; a larger one makes the WHOLE update a no-op on every rank and
        # read_metrics() at the next synchronisation switches this on for good, with a warning (DQ_TD_AUTOSCALE=0: raises DQ_ERR_RANGE instead):
        # nothing is ever partially applied)
        self.auto_scale = os.environ.get("DQ_TD_AUTOSCALE", "0") == "1"
        self.discarded_updates = 0   # optimizer steps the range guard discarded whole in this run (read_metrics; the reference would have applied them)
        self._range_ok_at = 0        # self.updates at the last synchronisation that found the range flag clear
        self.local_stats = [0, 0, 0, 0]
        self.inexact_total = 0
        self._inexact_acc = torch.zeros((), dtype=torch.int64, device=dev) if self._wide else None
        # guided exploration (guided_act_and_step): per-lattice flags of the step (row 0: followed the teacher, row 1: its matching took the fallback)
        # and their running sums; the caller zeroes and reads the sums (DQNAgent.fit)
        self._guide_flags = None
        self.guide_counts = torch.zeros(2, dtype=torch.int64, device=dev)
        self.ar_events = None        # bench.py: a list here collects HIP-event pairs around the exposed part of the gradient all-reduce
        self.ar_pool = []            # ... taken from this pool of pre-created pairs (creating two timing events per step costs host time inside the timed region)
        self.ar_stride, self._ar_seen = 1, 0     # ... in every ar_stride-th step only (two marker packets in the stream cost the step ~4 us)
        self._overlap = None         # DQ_DIST_MODE=overlap: the dense range's all-reduce stream (_SideStream, created at its first use)

    # ------------------------------------------------------------------------------------------------------
    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def _fused_update(self):
        """The update's launches run on the fused chains: they cover the network's BACKWARD (a narrower set than the forward's,
        QNetwork.fused_backward_supported) and are switched on.  What the riding environment step, the paired / ahead-of-time target forwards and the
        compact ring are decided on: each of them is a property of the fused training forward or backward."""
        return self.net.fused_backward_supported and self.net.fused_enabled

    # the ring's fields under the names bench.py, agent.py, the tests and tools/ use (obs_ring: uint8 [T, N, C, H, W], the tensor or -- compact
    # ring -- an ObsRingView; patch_ring: the compact ring's words, else None)
    T, cur, filled, compact = _ring_field("T"), _ring_field("cur"), _ring_field("filled"), _ring_field("compact")
    action_ring, reward_ring, terminal_ring = _ring_field("action"), _ring_field("reward"), _ring_field("terminal")
    obs_ring, patch_ring = _ring_field("obs"), _ring_field("patch")

    def _obs_job(self, **kw):
        """A forward job on the ring (rows through kw['index']) or on one slot of it (kw['slot'])."""
        slot = kw.pop("slot", None)
        store = self.ring.store
        kw["obs"] = store if slot is None else store[slot]
        if self.ring.compact:
            kw["patch"] = True
        return kw

    def reset_env(self):
        """env.reset() for every lattice; the new observation lands in ring slot `cur` (which has no action recorded
        yet).  If the ring already holds transitions (a second fit(), or a memory restored from a pickle), the entry
        before it is marked terminal so that no TD target bootstraps across the discontinuity."""
        self._join_env()
        r = self.ring
        if r.filled >= 2:
            r.terminal[r.next_slot(-1)].fill_(1)
        if r.compact:
            self.env.reset(out_patch=r.store[r.cur], write_obs=False)
        else:
            self.env.reset(out_obs=r.store[r.cur])
        r.filled = max(r.filled, 1)
        self.started = True

    def act_and_step(self, eps, masked_greedy=False, use_q=True, record_stats=True, presample=False):
        """One vector step: Q forward on the current observations, epsilon-greedy over the legal set, environment
        step with auto-reset; the transition is recorded in the ring by construction.  presample=True when update() follows this
        step: its replay sampling then rides on the environment launch (the rule never reads the slot this step writes)."""
        self._flush_stats()          # bookkeeping of the previous step, if no update() took it along (env buffers are about to be reused)
        r = self.ring
        cur = r.cur
        q = None
        if use_q:
            q = self.net.forward_multi([self._obs_job(params=self.params, slot=cur, batch=self.N, out=self.q_act, packed=self.params_pk)])[0]
        # action selection + environment step in one launch (dq_env_act_step == dq_policy_select then dq_env_step)
        sj = None
        if presample and r.filled_after() >= MIN_FILLED:
            sj = self._sample_job(self.updates + 1, r.next_slot(), r.filled_after())
        self._launch_env(self._env_step(q, eps, masked_greedy, sj))
        _step_taken(self, cur, record_stats)

    def guided_act_and_step(self, evaluator, eps, guide_share, masked_greedy=False, record_stats=True, method="matching"):
        """act_and_step() with a teacher: Q forward on the current observations, VectorEnv.guided_select -- an exploring lattice
        follows the matching decoder with probability guide_share -- into the ring's action slot, then dq_env_step with auto-reset writing the ring's
        reward / done slots and the successor observation; the episode bookkeeping is act_and_step's.  The lattice-steps that followed the teacher and
        those whose matching took its fallback are added to self.guide_counts on the device.  evaluator: a decoder.Evaluator of the environment's
        lattice.  method: the teacher, "matching" or "union_find" (VectorEnv.guided_select's).  One GPU, the narrow environment."""
        if self._wide or self.world_size > 1:
            raise NotImplementedError("guided_act_and_step: one GPU and the narrow environment (d <= 7)")
        cur, nxt, q, flags = _guided_head(self)
        r, env = self.ring, self.env
        env.guided_select(evaluator, self.vector_steps, q=q, eps=eps, guide_share=guide_share, masked_greedy=masked_greedy, out=r.action[cur],
                          out_guided=flags[0], out_inexact=flags[1], method=method)
        self.guide_counts += flags.sum(dim=1)
        if r.compact:
            env.arm_patch_output(r.store[nxt])
        env._launch(self.L.dq_env_step, env._h, ptr(r.action[cur]), 1, None if r.compact else ptr(r.store[nxt]), ptr(r.reward[cur]), ptr(r.terminal[cur]),
                    ptr(env.legal), ptr(env.lifetime), ptr(env.was_reset), self._stream())
        _step_taken(self, cur, record_stats)

    def guided_act_and_step_wide(self, evaluator, eps, guide_share, masked_greedy=False, record_stats=True, weights=None, correlated=None):
        """guided_act_and_step() for the wide environment with the union-find teacher: Q forward on the current observations,
        VectorEnv.guided_select_wide into the ring's action slot, then dq_envb_step with auto-reset writing the ring's reward / done slots and the successor
        observation; the referee's inexact flags are accumulated as _launch_env does it, the lattice-steps that followed the teacher are added to
        self.guide_counts[0].  Nothing rides on a wide launch: the update draws its own minibatch.  evaluator: a decoder_wide.WideEvaluator of the
        environment's d and error model, window >= volume_depth.  weights: VectorEnv.guided_select_wide's -- the teacher decodes
        on the weighted graph; None is the call of before, argument for argument.  correlated: VectorEnv.guided_select_wide's -- the
        teacher decodes in the three correlated passes.  One GPU, the wide environment."""
        if not self._wide or self.world_size > 1:
            raise NotImplementedError("guided_act_and_step_wide: one GPU and the wide environment (the narrow one: guided_act_and_step)")
        if weights is not None or correlated is not None:             # ValueError before the acting forward is launched
            weights = self.env._wide_uf_weights(weights, "guided_act_and_step_wide", correlated)
        kw = {} if weights is None else dict(weights=weights)
        if isinstance(weights, tuple) and len(weights) == 3:
            kw = dict(weights=weights[:2], correlated=weights[2])
        cur, nxt, q, flags = _guided_head(self)
        r, env = self.ring, self.env
        env.guided_select_wide(evaluator, self.vector_steps, q=q, eps=eps, guide_share=guide_share, masked_greedy=masked_greedy, out=r.action[cur],
                               out_guided=flags[0], **kw)
        self.guide_counts[0] += flags[0].sum()
        r.presampled = None
        check(self.L.dq_envb_step(env._h, ptr(r.action[cur]), 1, ptr(r.store[nxt]), ptr(r.reward[cur]), ptr(r.terminal[cur]), ptr(env.legal), ptr(env.lifetime),
                                  ptr(env.was_reset), ptr(env.inexact), self._stream()))
        self._inexact_acc += env.inexact.sum()                       # (read and reported at the next read_stats())
        _step_taken(self, cur, record_stats)

    def _sample_job(self, t, head, filled):
        """dq_sample_job for update number t, to be run on a ring with `head` / `filled`, into the look-ahead buffer (the update in
        progress may still be reading self.index)."""
        sj = _lib.SampleJob()
        sj.terminal_ring_dev, sj.n_slots, sj.head_slot, sj.filled_slots, sj.batch = ptr(self.ring.terminal), self.ring.T, head, filled, self.batch_size
        sj.seed[0], sj.seed[1] = int(self.seed[0]) & 0xFFFFFFFF, int(self.seed[1]) & 0xFFFFFFFF
        sj.t, sj.sample_base, sj.index_dev = t, _dist.shard(self.rank, self.N, self.batch_size)[1], ptr(self._index_next)
        self.ring.presampled = (t, head, filled)
        return sj

    def _env_step(self, q, eps, masked_greedy, sample=None, stats=None):
        """THE description of the environment launch of the vector step about to be taken (ring slot `cur` -> its successor): the record
        qnet._env_step_job reads for a launch that rides on the backward, and what _launch_env spells out as dq_env[b]_act_step[_sample]'s
        arguments.  patch: the ring slot to arm as patch output in front of the launch (compact ring; obs is then None)."""
        r, env = self.ring, self.env
        cur, nxt = r.cur, r.next_slot()
        return dict(q=q, eps=eps, masked_greedy=masked_greedy, seed=env.seed, t=self.vector_steps, action=r.action[cur], auto_reset=1,
                    obs=None if r.compact else r.store[nxt], patch=r.store[nxt] if r.compact else None, reward=r.reward[cur], done=r.terminal[cur],
                    legal=env.legal, lifetime=env.lifetime, was_reset=env.was_reset, sample=sample, stats=stats)

    def _launch_env(self, step):
        """The environment launch `step` (_env_step) on its own; an exception in front of it leaves no armed ring slot."""
        env, sj = self.env, step["sample"]
        try:
            if step["patch"] is not None:
                env.arm_patch_output(step["patch"])
            args = (env._h, ptr(step["q"]), float(step["eps"]), int(step["masked_greedy"]), (ctypes.c_uint32 * 2)(*step["seed"]), int(step["t"]),
                    ptr(step["action"]), step["auto_reset"], ptr(step["obs"]), ptr(step["reward"]), ptr(step["done"]), ptr(step["legal"]),
                    ptr(step["lifetime"]), ptr(step["was_reset"]))
            if self._wide:
                # selection + step in one launch; no replay sampling rides on it -- the update draws its own minibatch (_take_minibatch
                # notices that no look-ahead draw was made)
                self.ring.presampled = None
                check(self.L.dq_envb_act_step(*args, ptr(env.inexact), self._stream()))
                self._inexact_acc += env.inexact.sum()               # (read and reported at the next read_stats())
            elif sj is not None:
                check(self.L.dq_env_act_step_sample(*args, ctypes.byref(sj), self._stream()))
            else:
                check(self.L.dq_env_act_step(*args, self._stream()))
        except BaseException:
            env.disarm_patch_output()
            raise

    def _join_env(self):
        """Orders the current stream behind an environment launch still running on the side stream."""
        side = self._env_side
        if side is not None and side.inflight:
            torch.cuda.current_stream(self.device).wait_event(side.e_env)
            side.inflight = False

    def _episode_stats(self, slot):
        """The episode bookkeeping launch of the vector step recorded in ring slot `slot`, on the current stream."""
        env, r = self.env, self.ring
        check(self.L.dq_episode_stats(ptr(r.terminal[slot]), ptr(env.was_reset), ptr(env.lifetime), ptr(r.reward[slot]), self.N, ptr(self.stats),
                                      self._stream()))

    def _flush_stats(self):
        self._join_env()
        if self._stats_pending is not None:
            self._episode_stats(self._stats_pending[0])
            self._stats_pending = None

    def update(self, rows=None, target_ready=None, target_next=None):
        """One minibatch update (keras-rl DQNAgent.backward's training branch).  rows: its minibatch, already drawn (_extra_updates);
        target_ready: (Q_target(s1) of those rows, None or the event behind the forward that writes it): no target job in this update's launch pair;
        target_next: (rows of the NEXT update, buffer): its Q_target(s1) rides on this update's launch pair as a fourth job."""
        r = self.ring
        assert r.filled >= MIN_FILLED, "fewer than three complete transitions in the replay ring"
        self._join_env()
        B, N, T = self.batch_size, self.N, r.T
        self.updates += 1
        t = self.updates
        _, sample_base = _dist.shard(self.rank, N, B)
        if rows is None:
            self._take_minibatch(t, r.cur, r.filled, sample_base)
            self.last_index = self.index
            self.net.forward_multi(self._update_jobs(t, sample_base))
            self._learn(t)
            return
        self.last_index = rows                                      # (the rows of the last update: self.index keeps its own buffer for the look-ahead draws)
        own, self.index = self.index, rows                          # (every job record and the TD step read self.index)
        own_q1 = self.q1_target
        try:
            jobs = self._update_jobs(t, sample_base, with_target=target_ready is None)
            if target_next is not None:
                jobs.insert(0, self._obs_job(params=self.target, batch=B, index=target_next[0], index_off=N, index_mod=T * N, out=target_next[1],
                                             packed=self.target_pk))
            self.net.forward_multi(jobs)
            if target_ready is not None:
                self.q1_target = target_ready[0]
                if target_ready[1] is not None:
                    torch.cuda.current_stream(self.device).wait_event(target_ready[1])
            self._learn(t)
        finally:
            self.index, self.q1_target = own, own_q1

    def _extra_updates(self, k):
        """k further updates on the ring as it stands (DQNAgent.updates_per_vector_step - 1).  The first one's minibatch came with the environment
        launch; the others' are drawn by ONE launch here (dq_replay_sample_multi: the draws of consecutive updates on one ring state do not depend
        on each other) instead of a launch in front of every update -- round 5: one launch fewer per extra update."""
        if k <= 0:
            return
        self.update()
        if k == 1:
            return
        B = self.batch_size
        if self._index_multi is None or self._index_multi.shape[0] < k - 1:
            self._index_multi = torch.empty((k - 1, B), dtype=torch.int32, device=self.device)
        _, sample_base = _dist.shard(self.rank, self.N, B)
        r = self.ring
        _q.replay_sample_multi(r.terminal, self.N, r.T, r.cur, r.filled, B, self.seed, self.updates + 1, k - 1,
                               sample_base=sample_base, out=self._index_multi)
        if not (self.target_ahead and self._fused_update()):
            # The target network does not change inside a vector step and the rows of all these updates are known, so Q_target(s1) of update i + 1 needs
            # nothing update i produces: updates go in PAIRS -- the first one's launch pair carries four forwards (its own three and the second's target
            # forward), the second one's two.  At c3 the wave-private convolution kernel then runs 2 + 1 whole trips per pair of updates where three
            # forwards per launch are 1.5 trips timed as 2 each, and the dense kernel fills the chip (256 workgroups) instead of 192.
            if self.pair_targets and self._fused_update():
                if self._q1_pair is None:
                    self._q1_pair = torch.empty((B, self.A), dtype=torch.float32, device=self.device)
                i = 0
                while i + 1 < k - 1:
                    self.update(rows=self._index_multi[i], target_next=(self._index_multi[i + 1], self._q1_pair))
                    self.update(rows=self._index_multi[i + 1], target_ready=(self._q1_pair, None))
                    i += 2
                if i < k - 1:
                    self.update(rows=self._index_multi[i])
                return
            for i in range(k - 1):
                self.update(rows=self._index_multi[i])
            return
        # Q_target(s1) of update i + 1 on the side stream, released by a mark inside update i's backward (dq_qnet_mark_conv_backward: behind the
        # convolutional backward's launch -- the final reduction and the repacking that follow leave most of the device idle) and handed to update
        # i + 1's TD launch by an event of its own.  The first one goes out at once.
        side = self._side_setup(k - 1)
        self._side_forward(0, None)
        for i in range(k - 1):
            last = i + 1 == k - 1
            if not last:
                self.net.mark_conv_backward(side.marks[i])
            try:
                self.update(rows=self._index_multi[i], target_ready=(side.q1[i], side.ready[i]))
            finally:
                self.net.mark_conv_backward(None)
            if not last:
                self._side_forward(i + 1, side.marks[i])

    def _side_setup(self, n):
        B, net = self.batch_size, self.net
        if self._side is None:
            net2 = _q.QNetwork(net.input_shape, net.c_layers, net.ff_layers, net.n_actions, dueling=net.dueling, max_batch=net.max_batch, device=self.device)
            if self.ring.compact:
                net2.set_patch_input(self.env.volume_depth, self.env.patch_stride)
            self._side = _TargetAhead(net2, self.device)
        side = self._side
        if side.q1 is None or side.q1.shape[0] < n:
            side.q1 = torch.empty((n, B, self.A), dtype=torch.float32, device=self.device)
        while len(side.ready) < n:
            side.ready.append(torch.cuda.Event())
            side.marks.append(torch.cuda.Event())
        side.e_rows.record(torch.cuda.current_stream(self.device))  # behind the launch that drew the rows (and behind every reader of last step's Q_target rows)
        return side

    def _side_forward(self, i, after):
        """Q_target(s1) of extra update i (rows self._index_multi[i]) on the side stream, behind `after` (an event of the main stream) or, the first one,
        behind the rows' draw."""
        side = self._side
        with torch.cuda.stream(side.stream):
            side.stream.wait_event(side.e_rows if after is None else after)
            side.net.forward_multi([self._obs_job(params=self.target, batch=self.batch_size, index=self._index_multi[i], index_off=self.N,
                                                  index_mod=self.ring.T * self.N, out=side.q1[i], packed=self.target_pk)])
            side.ready[i].record(side.stream)

    def _take_minibatch(self, t, head, filled, sample_base):
        """self.index <- rows of update t on a ring with `head` / `filled`: the look-ahead draw if an environment launch made exactly
        that one, else a launch of its own."""
        r = self.ring
        if r.presampled == (t, head, filled):
            self.index, self._index_next = self._index_next, self.index
        else:
            _q.replay_sample(r.terminal, self.N, r.T, head, filled, self.batch_size, self.seed, t, sample_base=sample_base, out=self.index)
        r.presampled = None

    def _update_jobs(self, t, sample_base, with_target=True):
        # Q_online(s1) picks the action, Q_target(s1) values it (double DQN; without it Q_target does both); the training forward
        # on s0 is independent of both, so the three share one pair of launches
        B, N = self.batch_size, self.N
        rows = self.ring.T * N
        jobs = []
        if with_target:
            jobs.append(self._obs_job(params=self.target, batch=B, index=self.index, index_off=N, index_mod=rows, out=self.q1_target, packed=self.target_pk))
        if self.enable_double_dqn:
            jobs.append(self._obs_job(params=self.params, batch=B, index=self.index, index_off=N, index_mod=rows, out=self.q1_online,
                                      packed=self.params_pk))
        jobs.append(self._obs_job(params=self.params, batch=B, index=self.index, training=True, seed=self.seed, t=t, sample_base=sample_base,
                                  out=self.q0, packed=self.params_pk))
        return jobs

    def _td_job(self, step_stats=None):
        q_sel = self.q1_online if self.enable_double_dqn else self.q1_target
        r = self.ring
        return dict(q_online_s1=q_sel, q_target_s1=self.q1_target, q_s0=self.q0, reward=r.reward, terminal=r.terminal,
                    action=r.action, gamma=self.gamma, grad_scale=_dist.grad_scale(self.batch_size, self.world_size),
                    index=self.index, y=self.y, dq=self.dq, metrics=self.metrics, step_stats=step_stats, auto_scale=self.auto_scale,
                    delta_clip=self.delta_clip)

    def local_gradient(self, index=None):
        """This rank's contribution to the NEXT update's gradient, without the all-reduce and without the optimizer step: minibatch
        draw (or the given ring rows), the three forwards, TD step, backward; scaled by 1 / (batch_size * world_size), so that the SUM
        over the ranks is the gradient of the global-minibatch mean loss.  Leaves counters and parameters untouched (tests, diagnostics:
        tests/test_agent_gpu.py compares the sum of eight shard gradients with the gradient of one eight-times-larger lattice batch)."""
        r = self.ring
        assert r.filled >= MIN_FILLED
        self._join_env()
        t = self.updates + 1
        _, sample_base = _dist.shard(self.rank, self.N, self.batch_size)
        if index is None:
            _q.replay_sample(r.terminal, self.N, r.T, r.cur, r.filled, self.batch_size, self.seed, t, sample_base=sample_base, out=self.index)
        else:
            self.index.copy_(index)
        r.presampled = None
        self.net.forward_multi(self._update_jobs(t, sample_base))
        self.net.td_backward_phase0(self.params, self._td_job(), self.grads)
        self.net.backward_phase(self.params, self.dq, self.grads, 1)
        self._metrics_stale = True
        return self.grads

    def _exchange_form(self):
        """How this update's gradient is exchanged: None on one GPU, else "single" | "overlap" | "split" (DQ_DIST_MODE, default single).  Read at
        every call (bench.py times the forms against each other in one process).  overlap needs the learner's own RCCL communicator: a group
        without one (gloo, DQ_DIST_NATIVE=0) takes split instead."""
        if not _dist.dist_path(self.world_size):
            return None
        mode = os.environ.get("DQ_DIST_MODE", "single")
        if mode == "overlap":
            self.ensure_comm()
            return "overlap" if self._rccl is not None else "split"
        return "single" if mode == "single" else "split"

    def _backward(self, td, t, ride, whole, m=None, v=None):
        """The backward behind the forwards, TD step in its first launch.  whole: every layer in one sequence (td_backward_adam[_env]; with m, v
        Adam on its last launch, with None, None the gradient only); else phase 0 -- dueling + dense layers --, backward_phase(.., 1) follows.
        ride: the vector step's environment launch (_env_step) carried by the dense backward's first kernel."""
        net = self.net
        if ride is None:
            f_whole, f_phase0, tail = net.td_backward_adam, net.td_backward_phase0, ()
        else:
            f_whole, f_phase0, tail = net.td_backward_adam_env, net.td_backward_phase0_env, (self.env._h, ride)
        if whole:
            f_whole(self.params, td, self.grads, m, v, t, self.lr, self.beta_1, self.beta_2, self.epsilon, *tail)
        else:
            f_phase0(self.params, td, self.grads, *tail)

    @contextlib.contextmanager
    def _exposed(self):
        """Around the part of the gradient exchange the step WAITS for: bench.py's HIP-event pair (ar_events), in every ar_stride-th update."""
        probe = self.ar_events is not None and self._ar_seen % self.ar_stride == 0
        self._ar_seen += 1
        if probe:
            e0, e1 = self.ar_pool.pop() if self.ar_pool else (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            e0.record()
        yield
        if probe:
            e1.record()
            self.ar_events.append((e0, e1))

    def _exchange(self, form):
        """Sums self.grads over the ranks behind _backward (whole for "single", phase 0 for the other two, which run phase 1 beside the dense
        range's all-reduce)."""
        net, nconv = self.net, self.net.n_conv_params
        if form == "single":
            # ONE all-reduce of the whole flat gradient, on THIS stream through the learner's own RCCL communicator (dist.RcclComm; through
            # torch.distributed for gloo groups): the cheapest form up to 4 ranks (DESIGN.md section 7 compares the three)
            with self._exposed():
                self.ensure_comm()
                if self._rccl is not None:
                    self._rccl.allreduce_sum_(self.grads)
                else:
                    _dist.allreduce_sum_(self.grads, group=self.pg)
        elif form == "overlap":
            # the dense range (0.7 of the 0.77 MB at c3) on a SECOND stream through the learner's own RCCL communicator while the convolutional
            # backward (32 us) runs on the step's stream -- one event each way --; the convolutional range (66 KB) follows in-stream.  The same
            # collectives in the same order on every rank
            main = torch.cuda.current_stream(self.device)
            o = self._overlap = self._overlap or _SideStream(self.device, "e_dense", "e_ar")
            o.e_dense.record(main)
            with torch.cuda.stream(o.stream):
                o.stream.wait_event(o.e_dense)
                (self._rccl2 or self._rccl).allreduce_sum_(self.grads[nconv:])     # (the side stream's OWN communicator: two collectives of one communicator
                o.e_ar.record(o.stream)                                            #  in flight on two streams rest on RCCL's implicit serialisation)
            net.backward_phase(self.params, self.dq, self.grads, 1)
            with self._exposed():
                self._rccl.allreduce_sum_(self.grads[:nconv])
                main.wait_event(o.e_ar)
        else:
            # split: the same through torch.distributed, the dense range on the communicator's stream; the step waits for the convolutional
            # range's all-reduce (critical path) + whatever is left of the dense range's
            work = _dist.allreduce_sum_async(self.grads[nconv:], group=self.pg)
            net.backward_phase(self.params, self.dq, self.grads, 1)
            with self._exposed():
                _dist.allreduce_sum_(self.grads[:nconv], group=self.pg)
                if work is not None:
                    work.wait()

    def _learn(self, t, ride=None):
        """TD step, backward, gradient exchange, optimizer step, repack -- everything of an update behind its forwards.  ride: the vector
        step's environment launch (_env_step) to be carried by the dense backward's first kernel."""
        step_stats = None
        if self._stats_pending is not None:          # the pending episode bookkeeping rides on the TD launch
            assert ride is None
            (slot,), env, r = self._stats_pending, self.env, self.ring
            step_stats = (r.terminal[slot], env.was_reset, env.lifetime, r.reward[slot], self.N, self.stats)
            self._stats_pending = None
        td = self._td_job(step_stats)
        self._metrics_stale = True
        form = self._exchange_form()
        if form is None:                             # one GPU: Adam on the backward's last launch
            self._backward(td, t, ride, True, self.m, self.v)
        else:                                        # no optimizer step on the reduction: the guarded Adam behind the exchange
            self._backward(td, t, ride, form == "single")
            self._exchange(form)
            self.net.adam_step(self.params, self.grads, self.m, self.v, t, self.lr, self.beta_1, self.beta_2, self.epsilon)     # (skips AND flags non-finite elements: every rank alike)
        self.repack()

    def step_and_update(self, eps, masked_greedy=False, record_stats=True, presample_next=True, extra_updates=0):
        """act_and_step() followed by update(), with the acting forward and the update's forwards in ONE pair of launches -- same
        results as the two calls.  extra_updates: that many further update() calls on the same ring state (DQNAgent's
        updates_per_vector_step - 1: the reference trains one 32-sample minibatch per environment step, TRAIN:119-127, i.e. N minibatches
        per vector step of N lattices).  Possible because the update's minibatch never contains the newest transition (keras-rl's range:
        its successor observation is not in the memory yet), so it does not depend on this step's environment results -- the newest
        row it can hold is the previous step's, whose successor is the observation this step acts on: the parameters are the same
        for all four forwards.
        With presample_next the environment launch also draws the NEXT step's minibatch (if that step does not update, update()
        notices the stale draw and redraws)."""
        self._flush_stats()
        env, r, N = self.env, self.ring, self.N
        cur, nxt, filled = r.cur, r.next_slot(), r.filled_after()
        assert filled >= MIN_FILLED, "fewer than three complete transitions in the replay ring"
        t = self.updates + 1
        _, sample_base = _dist.shard(self.rank, N, self.batch_size)
        self._take_minibatch(t, nxt, filled, sample_base)        # (drawn from the ring as it WILL be after this step)
        self.last_index = self.index
        jobs = self._update_jobs(t, sample_base)
        jobs.append(self._obs_job(params=self.params, slot=cur, batch=N, out=self.q_act, packed=self.params_pk))
        self.net.forward_multi(jobs)      # (fused forward, per-layer backward: the inference jobs share one fused launch pair, the training job runs per layer)
        sj = None
        if extra_updates > 0:                    # the next update runs on THIS step's ring: the environment launch draws its minibatch
            sj = self._sample_job(t + 1, nxt, filled)
        elif presample_next:
            sj = self._sample_job(t + 1, r.next_slot(2), r.filled_after(2))
        side = self._env_side
        ride = self.ride_env and side is None and self._fused_update() and not self._wide and not getattr(env, "mlp_referee", False)
        # riding: one launch fewer per step -- the environment step (+ look-ahead sampling + this step's episode bookkeeping) rides on the
        # dense backward's first kernel (dq_qnet_td_backward_adam_env / _phase0_env): neither needs the other's results
        step = self._env_step(self.q_act, eps, masked_greedy, sj, self.stats if ride and record_stats else None)
        if ride:
            self._stats_pending = None
        elif side is not None:
            main = torch.cuda.current_stream(self.device)
            side.e_fwd.record(main)
            with torch.cuda.stream(side.stream):
                side.stream.wait_event(side.e_fwd)           # needs the acting forward's Q-values (and everything before it)
                self._launch_env(step)
                if record_stats:                             # the bookkeeping needs this step's results: it stays with the environment
                    self._episode_stats(cur)
                side.e_env.record(side.stream)
            side.inflight = True
            self._stats_pending = None
        else:
            self._launch_env(step)
            self._stats_pending = (cur,) if record_stats else None
        r.advance()
        self.vector_steps += 1
        self.updates = t
        if not ride:
            self._learn(t)
        else:
            try:
                if step["patch"] is not None:
                    env.arm_patch_output(step["patch"])      # (consumed by the riding step's launch)
                self._learn(t, ride=step)
            except BaseException:
                env.disarm_patch_output()                    # (an error in front of the riding launch: no armed ring slot outlives the call)
                raise
        self._extra_updates(extra_updates)

    def read_metrics(self):
        """(loss, mean_q) of the last update on this rank; reduces the per-block partials first (syncs)."""
        if self._metrics_stale:
            _q.td_metrics(self.metrics, self.batch_size)
            self._metrics_stale = False
        m = self.metrics[:2].cpu().numpy()
        try:
            self.net.check_range()   # (already synchronised) a gradient beyond the fused backward's range is never silent ...
        except _lib.DeepQError as e:
            # ... and with the default settings it is not fatal either: an update whose TD step met such a sample was discarded WHOLE on every rank (no
            # parameter moved; `updates` and Adam's t advanced past it -- the reference, fp32 with delta_clip = inf, would have applied it: the count is
            # kept in self.discarded_updates and logged), and from here on the gradient scale is MEASURED per minibatch (dq_td_job.auto_scale, +3 us per
            # update), which carries any finite TD error.  Sticky.  DQ_TD_AUTOSCALE=0 keeps the host-known scale and raises; DQ_TD_AUTOSCALE=1 measures
            # from the first update (nothing is ever discarded).
            n_lost = self.net.range_discarded()
            self.discarded_updates += n_lost
            # (the FORWARD's guard -- a parameter or activation outside the f16 pieces' range: a diverged run -- is always fatal: no gradient scale helps;
            # so is any trip with a finite delta_clip: its scale already carries every finite TD error, what is left is a NaN one or a diverged network)
            if e.status != -6 or "[forward]" in str(e) or self.auto_scale or os.environ.get("DQ_TD_AUTOSCALE") is not None \
                    or not np.isinf(self.delta_clip):
                raise
            self.auto_scale = True
            self.range_switches = getattr(self, "range_switches", 0) + 1
            import warnings
            warnings.warn(f"a TD error beyond the fused backward's host-known gradient scale: {n_lost} of the {self.updates - self._range_ok_at} updates since "
                          f"the last synchronisation were discarded (whole, on every rank; {self.discarded_updates} in this run: the reference would have applied "
                          "them); the loop now measures the gradient scale per minibatch (DQNCore.auto_scale = True) -- set DQ_TD_AUTOSCALE=1 to start that way")
        self._range_ok_at = self.updates
        return float(m[0]), float(m[1])

    def repack(self):
        """Must follow every change of self.params (Adam step, weight loading): refreshes the packed conv kernels."""
        if self.params_pk is not None:
            self.net.pack(self.params, out=self.params_pk)

    def update_target_hard(self):
        self.target.copy_(self.params)
        if self.target_pk is not None:
            self.target_pk.copy_(self.params_pk)

    def ensure_comm(self, with_overlap=False):
        """Creates the learner's own RCCL communicator if the several-GPU branch will use one (dist.make_rccl: a collective call -- every rank, at the
        same point; None for gloo groups / DQ_DIST_NATIVE=0).  Called by the first several-GPU update; bench.py calls it in front of its warm-up
        steps so that the rendezvous (~1 s) can never fall into a timed region.  with_overlap: also the side stream's communicator, whatever DQ_DIST_MODE
        says now (bench.py times both forms of the exchange and runs the faster: every rank calls this alike)."""
        if self._rccl is None and not self._rccl_tried and _dist.dist_path(self.world_size):
            self._rccl_tried = True
            self._rccl = _dist.make_rccl(self.rank, self.world_size, self.device, self.pg)
        # DQ_DIST_MODE=overlap: a second communicator for the dense range's all-reduce on the side stream (the same collective call on every rank)
        if self._rccl is not None and self._rccl2 is None and (with_overlap or os.environ.get("DQ_DIST_MODE") == "overlap"):
            self._rccl2 = _dist.make_rccl(self.rank, self.world_size, self.device, self.pg)

    def close_comm(self, abort=False):
        """Destroys the learner's own RCCL communicator (dist.RcclComm) -- every rank, behind a synchronisation, BEFORE the process group
        that did its rendezvous is destroyed; a later several-GPU update would create a new one.  abort: the caller is leaving through an exception
        (DQNAgent.fit's finally): ncclCommAbort instead of ncclCommDestroy, which could wait for peers inside a collective this rank never joins."""
        if self._rccl is not None:
            if abort:
                # the abort path exists for a collective this rank has queued and its peers will never join: a device synchronisation IN FRONT of
                # ncclCommAbort would wait for exactly that collective, for ever.  Abort first; then drain what is left, and never let a (sticky) HIP
                # error raised by that drain replace the exception that is unwinding through fit()
                try:
                    if self._rccl2 is not None:
                        self._rccl2.close(abort=True)
                    self._rccl.close(abort=True)
                finally:
                    self._rccl = self._rccl2 = None
                    try:
                        torch.cuda.synchronize(self.device)
                    except Exception:
                        pass
            else:
                try:
                    torch.cuda.synchronize(self.device)
                finally:
                    if self._rccl2 is not None:
                        self._rccl2.close(abort=False)
                    self._rccl.close(abort=False)
                    self._rccl = None
        self._rccl, self._rccl2, self._rccl_tried = None, None, False

    def close(self):
        """Releases what outlives the Python objects: the learner's RCCL communicator (before torch.distributed.destroy_process_group)."""
        self.close_comm()

    def __del__(self):
        try:
            self.close_comm()
        except Exception:
            pass

    def read_stats(self, reset=True, all_ranks=False):
        """(episodes ended, sum of their lifetimes, rewards earned, lattices stepped) since the last reset; syncs.  all_ranks: summed
        over the process group, so that every rank takes the same decisions from them (early stopping in DQNAgent.fit: a rank that left
        the loop alone would leave the others waiting in the gradient all-reduce)."""
        self._flush_stats()
        st = self.stats
        self.local_stats = None
        if all_ranks and self.world_size > 1:
            self.local_stats = [int(x) for x in st.cpu().tolist()]       # this rank's own share (DQNAgent.fit: the single-lattice episode end)
            st = st.clone()
            _dist.allreduce_sum_(st, group=self.pg)
        s = [int(x) for x in st.cpu().tolist()]
        if self.local_stats is None:
            self.local_stats = list(s)
        if reset:
            self.stats.zero_()
        if self._inexact_acc is not None:
            # wide environment: lattice-steps whose reward / done came from the matching referee's FALLBACK (more than 14 defects in a
            # component: the rest go to their nearer boundary, csrc/match_dev.h) -- heuristic referee decisions must not enter the
            # replay memory or the lifetime statistics silently
            n = int(self._inexact_acc.item())
            if n:
                self.inexact_total += n
                self._inexact_acc.zero_()
                import warnings
                warnings.warn(f"{n} lattice-steps since the last synchronisation were refereed by the matching decoder's inexact fallback "
                              f"(a cluster of more than 20 defects, or more than 32 defects in one component; {self.inexact_total} in total): their reward / done are heuristic")
        return s

    # -- evaluation on a scratch ring ---------------------------------------------------------------------------------------
    def begin_eval(self):
        """keras-rl stores nothing in test mode (memory.append(training=False) is a no-op): greedy evaluation steps run on a scratch
        three-slot ring, so that fit -> test -> fit (or pickling the memory after test()) never trains on evaluation transitions."""
        assert self._train_ring is None
        self._flush_stats()
        self._join_env()
        self.env.disarm_patch_output()                               # (nothing armed for the training ring survives the switch of rings)
        self._train_ring = (self.ring, self.started)
        self.ring = self.ring.scratch()

    def end_eval(self):
        self._flush_stats()
        self._join_env()
        self.env.disarm_patch_output()
        (self.ring, self.started), self._train_ring = self._train_ring, None
        # the lattices were reset and stepped by the evaluation: the ring's newest observation no longer describes them, so the next
        # fit() (which calls reset_env(): previous entry marked terminal, fresh observation into slot `cur`) must not skip its reset
        self.started = False
