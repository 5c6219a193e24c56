"""Episode lifetimes of four policies in the same environment (DESIGN.md sections 14 and 16): the shipped agent (DQNAgent.test_error_rates), the
space-time matching decoder (decoder.MatchingAgent), the union-find decoder (MatchingAgent(method="union_find")) and a policy that only ever sends the identity (no decoder), each on a fresh VectorEnv with the
same seed, global ids and rates, so that every policy meets the same noise streams.

    python tools/matching_lifetimes.py --family d5_dp|d5_x [--rates 0.001,...] [--episodes 101] [--lattices M] [--trained-at 0.007] [--out FILE]

One block of M lattices (default: --episodes, one episode per lattice) per rate, every rate run (no early stop).  Writes
profiles/matching_lifetimes_<family>.json: per policy the average lifetimes, episode counts, inexact steps and wall seconds, beside 1 / p."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
dq = importlib.import_module("deepq-decoding_amd")

C_LAYERS, FF_LAYERS = [[64, 3, 2], [32, 2, 1], [32, 2, 1]], [[512, 0.2]]
FAMILIES = {
    "d5_x": dict(d=5, error_model="X", use_Y=False, volume_depth=5),
    "d5_dp": dict(d=5, error_model="DP", use_Y=False, volume_depth=5),
}


def shipped_agent(env, family, trained_at):
    fx = np.load(os.path.join(ROOT, "tests", "golden", f"keras_weights_{family}_{trained_at}.npz"))
    model = dq.build_convolutional_nn(C_LAYERS, FF_LAYERS, env.obs_shape, env.num_actions)
    a = dq.DQNAgent(model=model, nb_actions=env.num_actions, memory=dq.SequentialMemory(limit=env.n_envs * 4, window_length=1),
                    nb_steps_warmup=1, target_model_update=1, policy=dq.GreedyQPolicy(masked_greedy=True),
                    test_policy=dq.GreedyQPolicy(masked_greedy=True), gamma=0.99, enable_dueling_network=True, batch_size=32)
    a.compile(dq.Adam(lr=1e-4))
    a._bind(env)
    a.model.set_weights([fx[f"w{i}"] for i in range(12)])
    return a


def run(policy, family, trained_at, rates, episodes, m, seed):
    env = dq.VectorEnv(n_envs=len(rates) * m, p_phys=rates[0], p_meas=rates[0], seed=seed, **FAMILIES[family])
    if policy == "agent":
        who = shipped_agent(env, family, trained_at)
    elif policy == "union_find":
        who = dq.decoder.MatchingAgent(method="union_find")
    else:
        who = dq.decoder.MatchingAgent(policy=policy)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    hist = who.test_error_rates(env, rates, nb_episodes=episodes, verbose=0)
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    out = dict(wall_seconds=seconds, avg_lifetime=[hist[p].history["episode_lifetimes_rolling_avg"][-1] for p in rates],
               episodes=[len(hist[p].history["episode_lifetime"]) for p in rates],
               agent_steps=[int(np.sum(hist[p].history["nb_steps"])) for p in rates])
    if policy in ("matching", "union_find"):
        out["inexact_steps"] = [who.last_inexact_by_rate[p] for p in rates]
        out["inexact_share"] = [who.last_inexact_by_rate[p] / max(1, who.last_vector_steps * m) for p in rates]
        out["vector_steps"] = who.last_vector_steps
    env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--family", required=True, choices=sorted(FAMILIES))
    ap.add_argument("--rates", default="")
    ap.add_argument("--episodes", type=int, default=101)
    ap.add_argument("--lattices", type=int, default=0)
    ap.add_argument("--trained-at", default="0.007")
    ap.add_argument("--seed", default="24301,57005")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    rates = [float(x) for x in a.rates.split(",")] if a.rates else [round(j * 0.001, 3) for j in range(1, 21)]
    m = a.lattices or a.episodes
    seed = tuple(int(x) for x in a.seed.split(","))
    res = {p: run(p, a.family, a.trained_at, rates, a.episodes, m, seed) for p in ("agent", "matching", "union_find", "identity")}
    print(f"{a.family}, agent trained at p = {a.trained_at}: average lifetime over {a.episodes} episodes per rate ({m} lattices per rate)")
    print(f"{'p':>7} {'agent':>10} {'matching':>10} {'union-find':>10} {'identity':>10} {'1/p':>8} {'inexact share':>14}")
    for k, p in enumerate(rates):
        print(f"{p:7.3f} {res['agent']['avg_lifetime'][k]:10.1f} {res['matching']['avg_lifetime'][k]:10.1f} {res['union_find']['avg_lifetime'][k]:10.1f} "
              f"{res['identity']['avg_lifetime'][k]:10.1f} "
              f"{1.0 / p:8.0f} {res['matching']['inexact_share'][k]:14.2e}")
    print("wall seconds: " + ", ".join(f"{p} {res[p]['wall_seconds']:.2f}" for p in res))
    record = dict(family=a.family, trained_at=a.trained_at, rates=rates, inverse_rate=[1.0 / p for p in rates], episodes_per_rate=a.episodes,
                  lattices_per_rate=m, seed=list(seed), policies=res,
                  note="inexact_share = inexact lattice-steps of the rate's block / (vector steps x lattices per rate): lattices that have delivered "
                       "their quota keep playing until the slowest rate is through")
    path = a.out or os.path.join(ROOT, "profiles", f"matching_lifetimes_{a.family}.json")
    with open(path, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
