"""The weighted union-find decoder as a policy of the wide environment (include/deepq_hip.h dq_envb_uf_select_weighted) in numpy, for
tests/test_weighted_env_uf_cpu.py and tests/test_weighted_env_uf_gpu.py: test_wide_env_uf_cpu.rule_action with weighted_uf_ref.decode -- which grows in unit
steps, where the device jumps from event to event -- in wide_uf_ref.decode's place, and the C oracle environment played by that rule with auto-reset.

replay(name, weights) is computed once per (configuration, pair) and never modified."""
import functools
import importlib

import numpy as np

import weighted_uf_ref as WU
from test_wide_env_uf_cpu import SEED, volume_grids

# name: (lattice with both rates, lattices, steps); env_id_base 0
CONFIGS = {
    "d5x": (dict(d=5, error_model="X", use_Y=False, volume_depth=5, p_phys=0.01, p_meas=0.06), 64, 40),
    "d5dp": (dict(d=5, error_model="DP", use_Y=False, volume_depth=5, p_phys=0.004, p_meas=0.04), 64, 40),
    "d9dp": (dict(d=9, error_model="DP", use_Y=False, volume_depth=5, p_phys=0.004, p_meas=0.04), 32, 24),
    "d13iid": (dict(d=13, error_model="IIDXZ", use_Y=False, volume_depth=4, p_phys=0.015, p_meas=0.06), 16, 12),
    "d15dpy": (dict(d=15, error_model="DP", use_Y=True, volume_depth=3, p_phys=0.01, p_meas=0.05), 16, 12),
    "d15deep": (dict(d=15, error_model="DP", use_Y=False, volume_depth=16, p_phys=0.005, p_meas=0.03), 4, 8),
}
CPU_CONFIGS = ("d5x", "d5dp", "d9dp")                             # the three whose event counts the CPU tests assert
OTHER_PAIRS = ((1, 1), (2, 1), (1, 2), (3, 2))                    # launched on every record of a run beside the configuration's own pair
LIMIT_PAIRS = ((15, 1), (1, 15))                                  # d = 5 only: the five-bit growth limit


def rate_pair(dq, name):
    cfg = CONFIGS[name][0]
    return dq.decoder_wide.uf_weights(cfg["p_phys"], cfg["p_meas"], cfg["error_model"])


def rule_action(dq, cfg, rec, weights):
    """The rule of dq_envb_uf_select_weighted for one lattice of COracleWideEnv.export(): weighted union-find on the whole volume as one last open window,
    then decoder.frame_to_actions against the completed set; the identity where done."""
    d, depth = cfg["d"], cfg["volume_depth"]
    layers = dq.decoder.action_layers(cfg["error_model"], cfg["use_Y"])
    if rec["done"]:
        return layers * d * d
    frame = WU.decode(d, volume_grids(d, rec["volume"])[None], depth, depth, False, weights)[0][0]
    completed = {a for a in range(layers * d * d + 1) if (rec["completed"] >> a) & 1}
    return dq.decoder.frame_to_actions(frame, completed, d, cfg["error_model"], cfg["use_Y"])[1]


def play(kw, n, steps, weights, others=()):
    """The oracle environment of lattice kw played by the rule under `weights` with auto-reset.  Returns dict(state: uint64 [steps + 1, n, state_words]
    exported in front of each step and after the last, action int32 [steps, n], reward, done, legal of after each step, legal0, identity, events,
    other: {pair: int32 [steps, n], the rule under that pair on the SAME records}); events counts, besides test_wide_env_uf_cpu.replay's, `ended` (the sum
    of done over the steps) and `differ` (live lattice-steps on which the unit rule, others' (1, 1), chooses another action)."""
    from oracle import c_oracle
    dq = importlib.import_module("deepq-decoding_amd")
    ref = c_oracle.COracleWideEnv(n_envs=n, seed=SEED, env_id_base=0, **kw)
    identity = ref.num_actions - 1
    ref.reset()
    ev = dict(live=0, done_visits=0, flips=0, second_flips=0, reward=0, ended=0, differ=0)
    out = dict(state=[], action=[], reward=[], done=[], legal=[], legal0=ref.legal.copy())
    other = {tuple(p): [] for p in others}
    for _ in range(steps):
        out["state"].append(ref.export_state())
        recs = ref.export()
        a = np.array([rule_action(dq, kw, r, weights) for r in recs], dtype=np.int32)
        for p in other:
            other[p].append(np.array([rule_action(dq, kw, r, p) for r in recs], dtype=np.int32))
        for i, (r, ai) in enumerate(zip(recs, a)):
            if r["done"]:
                ev["done_visits"] += 1
                assert ai == identity
                continue
            ev["live"] += 1
            if (1, 1) in other:
                ev["differ"] += int(other[(1, 1)][-1][i] != ai)
            if ai != identity:
                ev["flips"] += 1
                ev["second_flips"] += int(r["completed"] != 0)
        ref.step(a, auto_reset=True, want_obs=False)
        ev["reward"] += int((ref.reward == 1.0).sum())
        ev["ended"] += int((ref.done != 0).sum())
        out["action"].append(a)
        out["reward"].append(ref.reward.copy())
        out["done"].append(ref.done.copy())
        out["legal"].append(ref.legal.copy())
    out["state"].append(ref.export_state())
    out = {k: np.stack(v) if isinstance(v, list) else v for k, v in out.items()}
    out["other"] = {p: np.stack(v) for p, v in other.items()}
    for v in list(out.values()) + list(out["other"].values()):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    out["events"] = ev
    out["identity"] = identity
    return out


@functools.lru_cache(maxsize=None)
def replay(name, weights=None, others=True):
    """play() of a configuration under `weights` (default: uf_weights of its rates); others: also the rule under OTHER_PAIRS (and LIMIT_PAIRS at d = 5) on
    every record of the run."""
    dq = importlib.import_module("deepq-decoding_amd")
    kw, n, steps = CONFIGS[name]
    pair = rate_pair(dq, name) if weights is None else tuple(weights)
    extra = (OTHER_PAIRS + (LIMIT_PAIRS if kw["d"] == 5 else ())) if others else ()
    out = play(kw, n, steps, pair, extra)
    out["pair"] = pair
    return out


NO_DONE_VISIT = ("d15dpy", "d15deep")                             # short runs at d = 15: no episode ends in them; done lattices are d5x's to cover


def assert_minimums(name, ev):
    """test_wide_env_uf_cpu.assert_minimums' conditions on flips and done-lattice visits, so that a run that compares actions is not a run of identities.
    The weighted rule trusts a lone defect less than the unit rule does and waits more often, so the floors are a quarter where that function has a
    half: a flip on one lattice-step in four, a completed set that is not empty under one flip in four."""
    _, n, steps = CONFIGS[name]
    assert ev["live"] + ev["done_visits"] == n * steps
    assert ev["flips"] >= n * steps / 4, (name, ev)
    assert ev["second_flips"] >= ev["flips"] / 4, (name, ev)
    assert ev["done_visits"] >= (0 if name in NO_DONE_VISIT else 1), (name, ev)
