"""Launch times of the union-find kernels beside the matching ones, on the same inputs in one process, interleaved.

    python tools/union_find_launch_timing.py [--volumes 1048576] [--dense 4096] [--lattices 4096] [--launches 200] [--rounds 5] [--out FILE]

(a) uf_st_kernel against match_st_kernel (Evaluator.uf_into / match_into, one launch each) on --volumes d5_dp volumes at p = 0.007 and on --dense
    volumes at p = 0.06, device events around single launches, the two kernels alternating, median / min / max over --rounds.
(b) the union-find env_match kernel against the matching one on --lattices d5_dp lattices (bench.py's c3, p = 0.011) in mid-episode -- the state of every
    launch is a fresh one: between two timed pairs the lattices advance one agent step with the matching's action --, min / mean / max over --launches.
Writes profiles/union_find_launch_timing.json."""
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

D5DP = dict(d=5, error_model="DP", use_Y=False, volume_depth=5)


def timed_us(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return 1e3 * e0.elapsed_time(e1)


def stats(v):
    return dict(median_us=float(np.median(v)), mean_us=float(np.mean(v)), min_us=float(np.min(v)), max_us=float(np.max(v)), launches=len(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--volumes", type=int, default=1 << 20)
    ap.add_argument("--dense", type=int, default=4096)
    ap.add_argument("--lattices", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    D = dq.decoder
    record = dict(device=torch.cuda.get_device_name(0), volume_kernels={}, env_kernels={})
    # ---- (a) the volume kernels ---------------------------------------------------------------------------------------------------------------------
    for tag, n, p in (("sparse", a.volumes, 0.007), ("dense", a.dense, 0.06)):
        env = dq.VectorEnv(n_envs=1, p_phys=p, p_meas=p, seed=(24301, 57005), referee=None, **D5DP)
        vol, _, _ = D.sample_volumes(env, n, chunk=n)
        ev = D.Evaluator(5, "DP", False, 5, chunk=n, device=env.device)
        frame = torch.empty((n, 5, 5), dtype=torch.uint8, device=env.device)
        flag = torch.empty(n, dtype=torch.uint8, device=env.device)
        runs = {"match_st_kernel": lambda: ev.match_into(vol, n, frame, None, None, flag), "uf_st_kernel": lambda: ev.uf_into(vol, n, frame)}
        for fn in runs.values():                                                  # the tables, first launches
            fn()
        inexact = int(flag.sum())
        t = {k: [] for k in runs}
        for _ in range(a.rounds):
            for k, fn in runs.items():
                t[k].append(timed_us(fn))
        record["volume_kernels"][tag] = dict(volumes=n, p=p, matching_inexact_volumes=inexact, **{k: stats(v) for k, v in t.items()})
        print(tag, n, "volumes at p =", p, {k: round(float(np.median(v)), 1) for k, v in t.items()}, "us; matching inexact on", inexact)
        ev.close()
        env.close()
        del vol, frame, flag
    # ---- (b) the environment kernels, mid-episode -------------------------------------------------------------------------------------------------------
    n = a.lattices
    env = dq.VectorEnv(n_envs=n, p_phys=0.011, p_meas=0.011, seed=(24301, 57005), **D5DP)
    ev = D.Evaluator(5, "DP", False, 5, chunk=n, device=env.device)
    act, other = (torch.empty(n, dtype=torch.int32, device=env.device) for _ in range(2))
    flag = torch.zeros(n, dtype=torch.uint8, device=env.device)
    env.reset(write_obs=False)
    for _ in range(24):
        env.step(env.match_select(ev, out=act), auto_reset=True, write_obs=False)
    env.match_select(ev, out=other, method="union_find")
    t = {"env_match_kernel": [], "env_match_uf_kernel": []}
    inexact = 0
    for _ in range(a.launches):
        t["env_match_kernel"].append(timed_us(lambda: env.L.dq_env_match_select(env._h, ev._h, act.data_ptr(), flag.data_ptr(), env._stream())))
        t["env_match_uf_kernel"].append(timed_us(lambda: env.L.dq_env_uf_select(env._h, ev._h, other.data_ptr(), env._stream())))
        inexact += int(flag.sum())
        env.step(act, auto_reset=True, write_obs=False)
    record["env_kernels"] = dict(lattices=n, p=0.011, matching_inexact_lattice_steps=inexact, **{k: stats(v) for k, v in t.items()})
    for k, v in t.items():
        s = stats(v)
        print(f"{k:22s} min {s['min_us']:8.1f}  mean {s['mean_us']:8.1f}  max {s['max_us']:8.1f} us over {len(v)} launches")
    path = a.out or os.path.join(ROOT, "profiles", "union_find_launch_timing.json")
    with open(path, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
    print("wrote", path)
    ev.close()
    env.close()


if __name__ == "__main__":
    main()
