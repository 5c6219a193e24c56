"""The correlated union-find decoder as a policy of the wide environment (include/deepq_hip.h dq_envb_uf_select_correlated) in numpy,
for tests/test_correlated_env_uf_cpu.py and tests/test_correlated_env_uf_gpu.py: weighted_env_uf_ref.rule_action with correlated_uf_ref.decode -- the three
passes of section 25 on the lattice's volume as one last open window, grown in unit steps where the device jumps from event to event -- in
weighted_uf_ref.decode's place, and the C oracle environment played by that rule with auto-reset, the way weighted_env_uf_ref.play does it.

Under the X model component 1 is not decoded, so there is no mask: the rule is the weighted one whatever w_corr, which this file states as w_corr = w_space.

replay(name) is computed once per configuration and never modified."""
import functools
import importlib

import numpy as np

import correlated_uf_ref as CU
import weighted_env_uf_ref as WR
from test_wide_env_uf_cpu import SEED, volume_grids

D5DPY = dict(d=5, error_model="DP", use_Y=True, volume_depth=5, p_phys=0.01, p_meas=0.01)
# name: (lattice with both rates, lattices, steps, the run's triple -- None: uf_weights_correlated of the rates); env_id_base 0
CONFIGS = {
    "d5dp": WR.CONFIGS["d5dp"] + (None,),
    "d5dpy": (D5DPY, 64, 40, None),
    "d9dp": WR.CONFIGS["d9dp"] + (None,),
    "d13iid_321": WR.CONFIGS["d13iid"] + ((3, 2, 1),),             # (uf_weights_correlated makes IIDXZ a no-op: explicit triples)
    "d13iid_442": WR.CONFIGS["d13iid"] + ((4, 4, 2),),
    "d15dpy": WR.CONFIGS["d15dpy"] + (None,),
    "d15deep": WR.CONFIGS["d15deep"] + (None,),
    "d5x": WR.CONFIGS["d5x"] + (None,),
}
DP_CONFIGS = ("d5dp", "d5dpy", "d9dp")                            # the three whose share of differing actions the CPU tests assert
CPU_CONFIGS = DP_CONFIGS + ("d5x",)
DIFFERING = tuple(k for k, v in CONFIGS.items() if v[0]["error_model"] == "DP")          # every DP run: some action differs from the weighted launch's
OTHER_TRIPLES = ((4, 4, 1), (8, 7, 2))                            # launched on every record of a run beside the configuration's own triple
LIMIT_TRIPLES = ((15, 15, 1), (15, 1, 1))                         # d = 5 only: the five-bit growth limit
NO_DONE_VISIT = WR.NO_DONE_VISIT + ("d9dp",)                      # (under the correlated rule no episode of the d = 9 run ends either; the weighted run ends one)


def run_triple(dq, name):
    cfg, _, _, triple = CONFIGS[name]
    return dq.decoder_wide.uf_weights_correlated(cfg["p_phys"], cfg["p_meas"], cfg["error_model"]) if triple is None else tuple(triple)


def others(dq, name):
    """The triples beside the run's own: OTHER_TRIPLES, LIMIT_TRIPLES at d = 5, and the run's pair with w_corr = w_space -- the weighted rule."""
    w_space, w_time, _ = run_triple(dq, name)
    out = OTHER_TRIPLES + (LIMIT_TRIPLES if CONFIGS[name][0]["d"] == 5 else ()) + ((w_space, w_time, w_space),)
    return tuple(p for p in dict.fromkeys(out) if p != run_triple(dq, name))


def at_w_space(r):
    """Of a replay: the rule's actions under the run's pair with w_corr = w_space (the run's own actions where its triple is that one)."""
    w_space, w_time, _ = r["triple"]
    return r["other"].get((w_space, w_time, w_space), r["action"])


def rule_action(dq, cfg, rec, triple):
    """The rule of dq_envb_uf_select_correlated for one lattice of COracleWideEnv.export(): the three correlated passes on the whole volume as one last open
    window, then decoder.frame_to_actions against the completed set; the identity where done."""
    d, depth = cfg["d"], cfg["volume_depth"]
    layers = dq.decoder.action_layers(cfg["error_model"], cfg["use_Y"])
    if rec["done"]:
        return layers * d * d
    w_space, w_time, w_corr = (int(x) for x in triple)
    if cfg["error_model"] == "X":                                 # component 1 is not decoded: no mask
        w_corr = w_space
    frame = CU.decode(d, volume_grids(d, rec["volume"])[None], depth, depth, False, (w_space, w_time, w_corr))[0][0]
    completed = {a for a in range(layers * d * d + 1) if (rec["completed"] >> a) & 1}
    return dq.decoder.frame_to_actions(frame, completed, d, cfg["error_model"], cfg["use_Y"])[1]


def play(kw, n, steps, triple, others=(), weighted=True):
    """The oracle environment of lattice kw played by the rule under `triple` with auto-reset.  Returns weighted_env_uf_ref.play's dict -- state, action, reward,
    done, legal, legal0, identity, events, other: {triple: int32 [steps, n], the rule under that triple on the SAME records} -- and weighted: int32 [steps, n],
    weighted_env_uf_ref.rule_action under the triple's pair on the same records; events["differ"] counts the live lattice-steps on which that weighted rule
    chooses another action.  Under the X model also weighted_other: {triple: the weighted rule under that triple's pair}."""
    from oracle import c_oracle
    dq = importlib.import_module("deepq-decoding_amd")
    ref = c_oracle.COracleWideEnv(n_envs=n, seed=SEED, env_id_base=0, **kw)
    identity = ref.num_actions - 1
    ref.reset()
    ev = dict(live=0, done_visits=0, flips=0, second_flips=0, reward=0, ended=0, differ=0)
    out = dict(state=[], action=[], reward=[], done=[], legal=[], weighted=[], legal0=ref.legal.copy())
    other = {tuple(p): [] for p in others}
    weighted_other = {p: [] for p in other} if kw["error_model"] == "X" else {}
    for _ in range(steps):
        out["state"].append(ref.export_state())
        recs = ref.export()
        a = np.array([rule_action(dq, kw, r, triple) for r in recs], dtype=np.int32)
        for p in other:
            other[p].append(np.array([rule_action(dq, kw, r, p) for r in recs], dtype=np.int32))
        for p in weighted_other:
            weighted_other[p].append(np.array([WR.rule_action(dq, kw, r, p[:2]) for r in recs], dtype=np.int32))
        if weighted:
            w = np.array([WR.rule_action(dq, kw, r, tuple(triple[:2])) for r in recs], dtype=np.int32)
            out["weighted"].append(w)
        for i, (r, ai) in enumerate(zip(recs, a)):
            if r["done"]:
                ev["done_visits"] += 1
                assert ai == identity
                continue
            ev["live"] += 1
            if weighted:
                ev["differ"] += int(w[i] != ai)
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
    if not weighted:
        del out["weighted"]
    out = {k: np.stack(v) if isinstance(v, list) else v for k, v in out.items()}
    out["other"] = {p: np.stack(v) for p, v in other.items()}
    out["weighted_other"] = {p: np.stack(v) for p, v in weighted_other.items()}
    for v in list(out.values()) + list(out["other"].values()) + list(out["weighted_other"].values()):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    out["events"] = ev
    out["identity"] = identity
    return out


@functools.lru_cache(maxsize=None)
def replay(name):
    """play() of a configuration under its own triple, with the rule under others(name) on every record of the run."""
    dq = importlib.import_module("deepq-decoding_amd")
    kw, n, steps, _ = CONFIGS[name]
    triple = run_triple(dq, name)
    out = play(kw, n, steps, triple, others(dq, name))
    out["triple"] = triple
    return out


def assert_minimums(name, ev):
    """weighted_env_uf_ref.assert_minimums' floors on flips, second flips and done-lattice visits, for this file's configurations."""
    _, n, steps, _ = CONFIGS[name]
    assert ev["live"] + ev["done_visits"] == n * steps
    assert ev["flips"] >= n * steps / 4, (name, ev)
    assert ev["second_flips"] >= ev["flips"] / 4, (name, ev)
    assert ev["done_visits"] >= (0 if name in NO_DONE_VISIT else 1), (name, ev)
