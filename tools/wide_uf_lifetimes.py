"""Episode lifetimes of the wide environment under the union-find policy against the identity: recorded, not gated.

    python tools/wide_uf_lifetimes.py [--d 9 11 13 15] [--rates 0.016 ... 0.002] [--lattices 64] [--episodes 64] [--max-steps 40000] [--out FILE]

DP, volume_depth 5, p_meas = p_phys.  Per d one environment of --lattices lattices (one seed, ids 0 ..), and per rate one
WideUnionFindAgent.test_error_rates(env, [rate]) for the union-find row and one for the identity row: the same seed and ids for both.  The rates are taken
from the highest down; a rate whose union-find episodes do not end within --max-steps vector steps is recorded as censored and the lower ones, which last
longer still, are not run.  Mean lifetime with a 95 % normal interval of the mean.  Writes profiles/wide_uf_lifetimes_dp.json."""
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


def summary(hist):
    life = np.asarray(hist.history["episode_lifetime"], dtype=np.float64)
    half = 1.96 * life.std(ddof=1) / np.sqrt(len(life)) if len(life) > 1 else float("nan")
    return dict(episodes=int(len(life)), mean_lifetime=float(life.mean()), interval95=[float(life.mean() - half), float(life.mean() + half)],
                max_lifetime=float(life.max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", type=int, nargs="+", default=[9, 11, 13, 15])
    ap.add_argument("--rates", type=float, nargs="+", default=[0.016, 0.014, 0.012, 0.010, 0.008, 0.006, 0.004, 0.002])
    ap.add_argument("--lattices", type=int, default=64)
    ap.add_argument("--episodes", type=int, default=64)
    ap.add_argument("--max-steps", type=int, default=40000)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    record = dict(device=torch.cuda.get_device_name(0), model="DP", volume_depth=5, lattices=a.lattices, episodes=a.episodes, max_vector_steps=a.max_steps,
                  seed=list(SEED), rows={})
    path = a.out or os.path.join(ROOT, "profiles", "wide_uf_lifetimes_dp.json")
    for d in a.d:
        env = dq.VectorEnv(n_envs=a.lattices, seed=SEED, d=d, error_model="DP", use_Y=False, volume_depth=5, p_phys=0.01, p_meas=0.01, backend="wide")
        ev = dq.WideEvaluator(d, "DP", window=5, chunk=a.lattices, device=env.device)
        uf, ident = dq.WideUnionFindAgent(evaluator=ev), dq.WideUnionFindAgent(policy="identity")
        rows = record["rows"][f"d{d}"] = {}
        for rate in sorted(a.rates, reverse=True):
            row = dict(identity=summary(ident.test_error_rates(env, [rate], nb_episodes=a.episodes, verbose=0, nb_max_episode_steps=a.max_steps)[rate]))
            try:
                row["union_find"] = dict(summary(uf.test_error_rates(env, [rate], nb_episodes=a.episodes, verbose=0, nb_max_episode_steps=a.max_steps)[rate]),
                                         vector_steps=uf.last_vector_steps)
            except RuntimeError as e:
                row["union_find"] = dict(censored=True, reason=str(e)[:160])
            rows[f"{rate:g}"] = row
            u = row["union_find"]
            print(f"d = {d:2d} p = {rate:.3f}: identity {row['identity']['mean_lifetime']:9.1f}   union-find "
                  + ("censored" if u.get("censored") else f"{u['mean_lifetime']:9.1f} [{u['interval95'][0]:.1f}, {u['interval95'][1]:.1f}] in {u['vector_steps']} steps"),
                  flush=True)
            with open(path, "w") as f:                                                   # after every row: a time limit loses the row in progress only
                json.dump(record, f, indent=1)
                f.write("\n")
            if u.get("censored"):
                break
        ev.close()
        env.close()
    print("wrote", path)


if __name__ == "__main__":
    main()
