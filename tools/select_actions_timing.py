"""Launch times of the plain selection launch on both backends: recorded, not gated.

    python tools/select_actions_timing.py [--lattices 4096] [--rounds 5] [--calls 200] [--play 8] [--out FILE]

Per configuration -- the narrow environment at d = 5 (tools/guided_step_timing.py's), the wide one at d = 9 / volume_depth 9 and d = 15 / volume_depth 5
(tools/wide_env_uf_timing.py's) -- on --lattices mid-episode lattices (--play steps from a reset: uniform actions on the narrow backend, the union-find
policy on the wide one, whose per-step matching referee is slow on lattices that random actions have filled with defects) and one random Q row per
lattice: select_actions (policy_kernel / policy_wide_kernel) without a Q, at eps = 1, at eps = 0 unmasked and masked, and at eps = 0.1 masked.  Device
events around --calls back-to-back launches after ten untimed ones, as guided_step_timing does it; the variants alternate within each of --rounds
rounds.  Median, min and max of the rounds, in microseconds per launch."""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
dq = importlib.import_module("deepq-decoding_amd")

SEED = (24301, 57005)
CONFIGS = {
    "narrow_d5": dict(d=5, error_model="DP", use_Y=False, volume_depth=5, p_phys=0.011, p_meas=0.011),
    "wide_d9_depth9": dict(d=9, error_model="DP", use_Y=False, volume_depth=9, p_phys=0.006, p_meas=0.006, backend="wide"),
    "wide_d15_depth5": dict(d=15, error_model="DP", use_Y=False, volume_depth=5, p_phys=0.006, p_meas=0.006, backend="wide"),
}


def events_us(fn, calls):
    for _ in range(10):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return 1e3 * e0.elapsed_time(e1) / calls


class Config:
    def __init__(self, cfg, n, play):
        self.env = env = dq.VectorEnv(n_envs=n, seed=SEED, **cfg)
        dev = env.device
        self.q = torch.randn((n, env.num_actions), device=dev, generator=torch.Generator(device=dev).manual_seed(5))
        self.action = torch.empty(n, dtype=torch.int32, device=dev)
        env.reset()
        if env.wide:
            ev = dq.WideEvaluator(env.d, env.error_model, window=env.volume_depth, chunk=n, device=dev)
            for _ in range(play):
                env.uf_select_wide(ev, out=self.action)
                env.step(self.action, auto_reset=True, write_obs=False)
            ev.close()
        else:
            for t in range(play):
                env.act_step(t, auto_reset=True, out_action=self.action)
        self.t = play

    def launches(self):
        e, q, t, out = self.env, self.q, self.t, self.action
        return {"select_actions no q": lambda: e.select_actions(t, out=out),
                "select_actions eps=1": lambda: e.select_actions(t, q=q, eps=1.0, out=out),
                "select_actions eps=0": lambda: e.select_actions(t, q=q, eps=0.0, out=out),
                "select_actions eps=0 masked": lambda: e.select_actions(t, q=q, eps=0.0, masked_greedy=True, out=out),
                "select_actions eps=0.1 masked": lambda: e.select_actions(t, q=q, eps=0.1, masked_greedy=True, out=out)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lattices", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--play", type=int, default=8)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    cfgs = {}
    for k, cfg in CONFIGS.items():
        cfgs[k] = Config(cfg, a.lattices, a.play)
        torch.cuda.synchronize()
        print(k, "ready", flush=True)
    us = {k: {name: [] for name in c.launches()} for k, c in cfgs.items()}
    for _ in range(a.rounds):
        for k, c in cfgs.items():
            for name, fn in c.launches().items():
                us[k][name].append(events_us(fn, a.calls))
    record = dict(device=torch.cuda.get_device_name(0), lattices=a.lattices, rounds=a.rounds, calls_per_round=a.calls, played_steps=a.play, model="DP", configurations={})
    for k, c in cfgs.items():
        rows = {name: dict(median_us=float(np.median(v)), min_us=float(np.min(v)), max_us=float(np.max(v)), rounds_us=v) for name, v in us[k].items()}
        record["configurations"][k] = dict(d=c.env.d, volume_depth=c.env.volume_depth, num_actions=c.env.num_actions, launches=rows)
        for name, r in rows.items():
            print(f"{k:16s} {name:30s} median {r['median_us']:8.2f} us  [{r['min_us']:8.2f}, {r['max_us']:8.2f}]")
        c.env.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")
        print("wrote", a.out)


if __name__ == "__main__":
    main()
