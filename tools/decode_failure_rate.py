"""Logical failure rate of decoding one volume with a shipped agent, scored on the device (DQNAgent.decode_benchmark, csrc/decode_eval.hip;
DESIGN.md section 12).

    python tools/decode_failure_rate.py [--family d5_dp] [--weights 0.007] [--rates 0.003,0.007,0.011] [--n 1048576] [--chunk 262144] [--out profiles/NAME.json]

Per rate: the failure rate (1 - success / volumes: the residual error is not a stabilizer) with its Wilson 95 % interval for the agent under
the masked and the plain greedy policy, for space-time minimum-weight matching (the `matching` row, on the same volumes; its phases are sample /
match / verdict, and `match_over_agent_decode` is its match time over the masked agent's decode time), for the union-find decoder (the `union_find` row, the
same volumes and phases) and for no decoder at all (frame = 0), the death rate (the referee loses the residual's class), the
share of all-zero volumes, corrections per volume, the status histogram, and the wall time of the phases (sample / decode / verdict, each
closed by a synchronisation; the verdict phase of the masked run also carries the frame = 0 verdict).  Weights: tests/golden/keras_weights_<family>_<weights>.npz.
One process, no retries: the first failing GPU call ends it.  On a shared box run it under a time limit, e.g. `timeout -k 10 600 python tools/...`."""
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
FAMILIES = {"d5_x": dict(d=5, error_model="X", use_Y=False, volume_depth=5), "d5_dp": dict(d=5, error_model="DP", use_Y=False, volume_depth=5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--family", default="d5_dp", choices=sorted(FAMILIES))
    ap.add_argument("--weights", default="0.007")
    ap.add_argument("--rates", default="0.007")
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--chunk", type=int, default=1 << 18)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    cfg = FAMILIES[a.family]
    rates = [float(r) for r in a.rates.split(",")]
    fx = np.load(os.path.join(ROOT, "tests", "golden", f"keras_weights_{a.family}_{a.weights}.npz"))
    env = dq.VectorEnv(n_envs=1, p_phys=rates[0], p_meas=rates[0], **cfg)
    model = dq.build_convolutional_nn(C_LAYERS, FF_LAYERS, env.observation_space.shape, env.num_actions)
    agent = dq.DQNAgent(model=model, nb_actions=env.num_actions, memory=dq.SequentialMemory(limit=1000, window_length=1), nb_steps_warmup=100,
                        target_model_update=100, policy=dq.GreedyQPolicy(masked_greedy=True), test_policy=dq.GreedyQPolicy(masked_greedy=True),
                        gamma=0.99, enable_dueling_network=True)
    agent.compile(dq.Adam(lr=1e-4))
    agent._bind(env)
    agent.model.set_weights([fx[f"w{i}"] for i in range(12)])
    agent.decode_benchmark(env, min(a.n, a.chunk), rates=[rates[0]], chunk=a.chunk)            # warm-up: allocations, first launches
    out = {"family": a.family, "weights": a.weights, "volumes_per_rate": a.n, "chunk": a.chunk, "device": torch.cuda.get_device_name(0), "rates": {}}
    mev = None
    for r in rates:
        row = {}
        for name, masked in (("masked", True), ("unmasked", False)):
            agent.decode_benchmark(env, min(a.n, a.chunk), rates=[r], masked_greedy=masked, chunk=a.chunk)     # (a decoder of these settings exists)
            timings = {}
            t0 = time.perf_counter()
            res = agent.decode_benchmark(env, a.n, rates=[r], masked_greedy=masked, chunk=a.chunk, no_decoder=masked, timings=timings)[r]
            wall = time.perf_counter() - t0
            s = res.summary()
            nd = s.pop("no_decoder", None)
            s["ms"] = {k: round(1e3 * timings.get(k, 0.0), 3) for k in ("sample", "decode", "verdict")}
            s["ms"]["wall"] = round(1e3 * wall, 3)
            row[name] = s
            if nd is not None:
                row["no_decoder"] = {k: nd[k] for k in ("volumes", "in_codespace", "success", "alive", "failure_rate", "failure_interval", "death_rate",
                                                        "death_interval")}
            print(f"p = {r} {name:8s}: failure {res.failure_rate:.6f} [{res.failure_interval[0]:.6f}, {res.failure_interval[1]:.6f}]  death {res.death_rate:.6f}  "
                  f"trivial {res.trivial_share:.4f}  corrections / volume {res.mean_corrections:.4f}  {res.status_histogram}  ms {s['ms']}", flush=True)
        # the space-time matching baseline on the same volumes (decoder.score_matching)
        D = dq.decoder
        if mev is None:                                                                                 # one scoring handle for every call: its matching tables are built once
            mev = D.Evaluator(cfg["d"], cfg["error_model"], cfg["use_Y"], cfg["volume_depth"], chunk=a.chunk, device=env.device)
        for method in D.METHODS:                                                                        # the same volumes for either baseline
            D.score_matching(env, min(a.n, a.chunk), rates=[r], evaluator=mev, method=method)           # warm-up: the tables, first launch, allocations
            timings = {}
            t0 = time.perf_counter()
            mres = D.score_matching(env, a.n, rates=[r], timings=timings, evaluator=mev, method=method)[r]
            wall = time.perf_counter() - t0
            s = mres.summary()
            s["inexact"] = mres.inexact
            s["ms"] = {k: round(1e3 * timings.get(k, 0.0), 3) for k in ("sample", "match", "verdict")}
            s["ms"]["wall"] = round(1e3 * wall, 3)
            s["match_over_agent_decode"] = round(s["ms"]["match"] / row["masked"]["ms"]["decode"], 4)
            row[method] = s
            print(f"p = {r} {method}: failure {mres.failure_rate:.6f} [{mres.failure_interval[0]:.6f}, {mres.failure_interval[1]:.6f}]  death {mres.death_rate:.6f}  "
                  f"corrections / volume {mres.mean_corrections:.4f}  inexact {mres.inexact}  ms {s['ms']}  match / agent decode {s['match_over_agent_decode']}", flush=True)
        nd = row["no_decoder"]
        print(f"p = {r} frame = 0: failure {nd['failure_rate']:.6f} [{nd['failure_interval'][0]:.6f}, {nd['failure_interval'][1]:.6f}]  death {nd['death_rate']:.6f}",
              flush=True)
        out["rates"][str(r)] = row
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    if mev is not None:
        mev.close()
    agent._decoder = None
    env.close()


if __name__ == "__main__":
    main()
