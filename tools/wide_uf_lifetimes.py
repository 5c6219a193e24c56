"""Episode lifetimes of the wide environment under the union-find policy against the identity (DESIGN.md sections 19, 24 and 26): recorded, not gated.

    python tools/wide_uf_lifetimes.py [--d 9 11 13 15] [--rates 0.016 ... 0.002] [--lattices 64] [--episodes 64] [--max-steps 40000]
                                      [--meas-ratio R] [--weights rates|WS,WT] [--correlated rates|W] [--referee matching|uf] [--out FILE]

DP, volume_depth 5, p_meas = p_phys (--meas-ratio R: p_meas = R p).  Per d one environment of --lattices lattices (one seed, ids 0 ..), and per rate one
WideUnionFindAgent.test_error_rates(env, [rate]) for the union-find row and one for the identity row: the same seed and ids for both.  --weights adds a third
row on the same seed and ids, the policy on the weighted graph: "rates" takes decoder_wide.uf_weights of the row's own (p, p_meas),
WS,WT one pair for every row; the row records the pair it played with and the ratio of its mean lifetime to the unit row's, with both episode counts and
whether the two 95 % intervals overlap (where they do the ratio resolves nothing).  The rates are taken from the highest down; a rate whose union-find
episodes do not end within --max-steps vector steps is recorded as censored and the lower ones, which last longer still, are not run.  Mean lifetime with a
95 % normal interval of the mean.  --correlated (with --weights) adds a fourth row on the same seed and ids, the policy in the three
correlated passes: "rates" (beside --weights rates) takes decoder_wide.uf_weights_correlated of the row's own rates, W one w_corr beside the pair WS,WT; the
row records the triple it played with and the ratio of its mean lifetime to the WEIGHTED row's, with both episode counts and whether the two 95 % intervals
overlap -- where they are apart the row says which policy lives longer.  Writes profiles/wide_uf_lifetimes_dp.json (with --weights:
profiles/wide_uf_lifetimes_weighted.json, with --correlated: profiles/wide_uf_lifetimes_correlated.json).
--referee plays under the named referee of the wide environment, VectorEnv(referee=...): "matching" is what the tool played under before
the option existed, "uf" the union-find referee, which has no cluster limit and so reaches d = 13 and 15.  The record then goes to
profiles/wide_uf_lifetimes_referee.json, which holds one record per referee: a run replaces its own referee's rows of the distances it played and keeps
everything else that the file held."""
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


def played(agent, env, rate, pm, a):
    """One row: the agent's episodes at (rate, pm) from a reset, or the censoring."""
    try:
        h = agent.test_error_rates(env, [rate], nb_episodes=a.episodes, p_meas=pm, verbose=0, nb_max_episode_steps=a.max_steps)[rate]
        return dict(summary(h), vector_steps=agent.last_vector_steps)
    except RuntimeError as e:
        return dict(censored=True, reason=str(e)[:160])


def shown(u):
    return "censored" if u.get("censored") else f"{u['mean_lifetime']:9.1f} [{u['interval95'][0]:.1f}, {u['interval95'][1]:.1f}] in {u['vector_steps']} steps"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", type=int, nargs="+", default=[9, 11, 13, 15])
    ap.add_argument("--rates", type=float, nargs="+", default=[0.016, 0.014, 0.012, 0.010, 0.008, 0.006, 0.004, 0.002])
    ap.add_argument("--lattices", type=int, default=64)
    ap.add_argument("--episodes", type=int, default=64)
    ap.add_argument("--max-steps", type=int, default=40000)
    ap.add_argument("--meas-ratio", type=float, default=1.0)
    ap.add_argument("--weights", default=None)
    ap.add_argument("--correlated", default=None)
    ap.add_argument("--referee", default=None, choices=["matching", "uf"])
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    weights = None if a.weights is None else a.weights if a.weights == "rates" else tuple(int(x) for x in a.weights.split(","))
    correlated = None if a.correlated is None else a.correlated if a.correlated == "rates" else int(a.correlated)
    if correlated is not None and weights is None:
        ap.error("--correlated compares against the weighted row: give --weights")
    record = dict(device=torch.cuda.get_device_name(0), model="DP", volume_depth=5, lattices=a.lattices, episodes=a.episodes, max_vector_steps=a.max_steps,
                  seed=list(SEED), p_meas="= p" if a.meas_ratio == 1.0 else f"= {a.meas_ratio:g} p", weights=a.weights, correlated=a.correlated, rows={})
    path = a.out or os.path.join(ROOT, "profiles", "wide_uf_lifetimes_referee.json" if a.referee else "wide_uf_lifetimes_correlated.json" if correlated is not None
                                 else "wide_uf_lifetimes_weighted.json" if weights else "wide_uf_lifetimes_dp.json")
    whole = record
    if a.referee:                                                                        # one record per referee in one file
        record["referee"] = a.referee
        whole = json.load(open(path)) if os.path.exists(path) else {}
        record["rows"] = dict(whole.get(a.referee, {}).get("rows", {}))
        whole[a.referee] = record
    for d in a.d:
        env = dq.VectorEnv(n_envs=a.lattices, seed=SEED, d=d, error_model="DP", use_Y=False, volume_depth=5, p_phys=0.01, p_meas=0.01, backend="wide",
                           **({"referee": a.referee} if a.referee else {}))
        ev = dq.WideEvaluator(d, "DP", window=5, chunk=a.lattices, device=env.device)
        uf, ident = dq.WideUnionFindAgent(evaluator=ev), dq.WideUnionFindAgent(policy="identity")
        weighted = dq.WideUnionFindAgent(evaluator=ev, weights=weights) if weights else None
        corr = dq.WideUnionFindAgent(evaluator=ev, weights=weights, correlated=correlated) if correlated is not None else None
        rows = record["rows"][f"d{d}"] = {}
        for rate in sorted(a.rates, reverse=True):
            pm = min(1.0, a.meas_ratio * rate)
            row = dict(p_meas=pm, identity=summary(ident.test_error_rates(env, [rate], nb_episodes=a.episodes, p_meas=pm, verbose=0,
                                                                          nb_max_episode_steps=a.max_steps)[rate]))
            u = row["union_find"] = played(uf, env, rate, pm, a)
            print(f"d = {d:2d} p = {rate:.3f}: identity {row['identity']['mean_lifetime']:9.1f}   union-find " + shown(u), flush=True)
            if weighted is not None:
                w = row["union_find_weighted"] = played(weighted, env, rate, pm, a)
                w["weights"] = weighted.last_weights
                if not u.get("censored") and not w.get("censored"):
                    apart = w["interval95"][0] > u["interval95"][1] or u["interval95"][0] > w["interval95"][1]
                    w.update(lifetime_over_unit=w["mean_lifetime"] / u["mean_lifetime"], episodes_unit=u["episodes"], intervals_overlap=not apart)
                print(f"                    weighted {w['weights']} " + shown(w)
                      + ("" if "lifetime_over_unit" not in w else f"   x {w['lifetime_over_unit']:.2f} of unit"
                         + (" (intervals overlap)" if w["intervals_overlap"] else "")), flush=True)
            if corr is not None:
                c = row["union_find_correlated"] = played(corr, env, rate, pm, a)
                c["weights"] = corr.last_weights
                if not w.get("censored") and not c.get("censored"):
                    longer = "correlated" if c["interval95"][0] > w["interval95"][1] else "weighted" if w["interval95"][0] > c["interval95"][1] else None
                    c.update(lifetime_over_weighted=c["mean_lifetime"] / w["mean_lifetime"], episodes_weighted=w["episodes"], intervals_overlap=longer is None,
                             resolved_longer=longer)
                print(f"                    correlated {c['weights']} " + shown(c)
                      + ("" if "lifetime_over_weighted" not in c else f"   x {c['lifetime_over_weighted']:.2f} of weighted"
                         + (" (intervals overlap)" if c["intervals_overlap"] else f" ({c['resolved_longer']} lives longer, resolved)")), flush=True)
            rows[f"{rate:g}"] = row
            with open(path, "w") as f:                                                   # after every row: a time limit loses the row in progress only
                json.dump(whole, f, indent=1)
                f.write("\n")
            if u.get("censored") or (weighted is not None and row["union_find_weighted"].get("censored")) or (
                    corr is not None and row["union_find_correlated"].get("censored")):
                break
        ev.close()
        env.close()
    print("wrote", path)


if __name__ == "__main__":
    main()
