"""Does exploration guided by the matching decoder help training?  Trains the same configuration twice from the same seed --
once with plain epsilon-greedy exploration, once with EpsGreedyQPolicy(guide=MatchingAgent(), guide_share=...) -- and scores both trained agents with
DQNAgent.test_error_rates on the same lattice ids.

    python tools/guided_training.py --family d5_dp|d5_x --steps N [--guide-share 0.5] [--method matching|union_find] [--lattices 64] [--updates-per-step 0] [--out FILE]

--method union_find: the teacher is the union-find decoder; the record then goes to profiles/union_find_training_<family>.json.

The configuration: the hyper-parameters of tests/golden/fixed_config_d5_dp.p (network, batch 32, buffer 50 000, no masked greedy; d5_x: the same with
bit-flip noise) at p = 0.007, the variable ones of tests/golden/variable_config_d5_dp_0.011_92.p (Adam 5e-6, gamma 0.99, target copy every 2500 steps,
learning starts at 1000, epsilon 1 -> 0.02) with the annealing stretched over the first fifth of the step budget as in the reference's recipe (200 000 of
1 000 000).  --steps counts environment steps (lattice-steps); --lattices lattices advance per vector step, --updates-per-step minibatch updates follow
each vector step (0: one per lattice, the reference's replay ratio).  Writes profiles/guided_training_<family>.json: both training histories, both
lifetime rows, the guided / inexact lattice-steps and the wall time per vector step of each run."""
import argparse
import importlib
import json
import os
import pickle
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
dq = importlib.import_module("deepq-decoding_amd")

P_TRAIN = 0.007
TEST_RATES = [0.003, 0.005, 0.007, 0.009, 0.011]


def configuration(family):
    with open(os.path.join(ROOT, "tests", "golden", "fixed_config_d5_dp.p"), "rb") as f:
        cfg = pickle.load(f)
    with open(os.path.join(ROOT, "tests", "golden", "variable_config_d5_dp_0.011_92.p"), "rb") as f:
        cfg.update(pickle.load(f))
    cfg.update(p_phys=P_TRAIN, p_meas=P_TRAIN)
    if family == "d5_x":
        cfg.update(error_model="X")
    return cfg


def lattice(cfg):
    return dict(d=cfg["d"], error_model=cfg["error_model"], use_Y=cfg["use_Y"], volume_depth=cfg["volume_depth"])


def train_and_score(cfg, steps, lattices, updates, guide_share, seed, episodes, eval_lattices, method="matching"):
    env = dq.VectorEnv(n_envs=lattices, p_phys=cfg["p_phys"], p_meas=cfg["p_meas"], seed=seed, **lattice(cfg))
    guide = None if guide_share is None else dq.decoder.MatchingAgent(method=method)
    inner = dq.EpsGreedyQPolicy(masked_greedy=cfg["masked_greedy"], guide=guide, guide_share=1.0 if guide_share is None else guide_share)
    policy = dq.LinearAnnealedPolicy(inner, attr="eps", value_max=cfg["max_eps"], value_min=cfg["final_eps"], value_test=0.0, nb_steps=max(1, steps // 5))
    model = dq.build_convolutional_nn(cfg["c_layers"], cfg["ff_layers"], env.obs_shape, env.num_actions)
    agent = dq.DQNAgent(model=model, nb_actions=env.num_actions, memory=dq.SequentialMemory(limit=cfg["buffer_size"], window_length=1),
                        nb_steps_warmup=cfg["learning_starts"], target_model_update=cfg["target_network_update_freq"], policy=policy,
                        test_policy=dq.GreedyQPolicy(masked_greedy=True), gamma=cfg["gamma"], enable_dueling_network=cfg["dueling"],
                        batch_size=cfg["batch_size"], train_interval=cfg["train_freq"], seed=seed, updates_per_vector_step=updates)
    agent.compile(dq.Adam(lr=cfg["learning_rate"]))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    hist = agent.fit(env, nb_steps=steps, verbose=0, episode_averaging_length=cfg["rolling_average_length"], success_threshold=None,
                     stopping_patience=None, min_nb_steps=steps, single_cycle=False)
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    vector_steps = agent._core.vector_steps
    # the greedy agent on fresh lattices: the same seed and ids for either run, one block of eval_lattices per rate
    sweep = dq.VectorEnv(n_envs=len(TEST_RATES) * eval_lattices, p_phys=P_TRAIN, p_meas=P_TRAIN, seed=(seed[0] + 1, seed[1]), **lattice(cfg))
    rows = agent.test_error_rates(sweep, TEST_RATES, nb_episodes=episodes, verbose=0)
    out = dict(guide_share=guide_share, train_seconds=seconds, vector_steps=vector_steps, ms_per_vector_step=1e3 * seconds / max(1, vector_steps),
               updates=agent._core.updates, guided_steps=agent.last_guided_steps, inexact_steps=agent.last_inexact_steps, env_steps=agent.step,
               history={k: [None if isinstance(x, float) and x != x else x for x in v] for k, v in hist.history.items()},
               lifetimes={str(p): rows[p].history["episode_lifetimes_rolling_avg"][-1] for p in TEST_RATES},
               episodes={str(p): len(rows[p].history["episode_lifetime"]) for p in TEST_RATES})
    sweep.close()
    env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--family", required=True, choices=["d5_dp", "d5_x"])
    ap.add_argument("--steps", type=int, required=True, help="environment steps (lattice-steps) of each training run")
    ap.add_argument("--guide-share", type=float, default=0.5)
    ap.add_argument("--method", default="matching", choices=["matching", "union_find"], help="the teacher of the guided run")
    ap.add_argument("--lattices", type=int, default=64)
    ap.add_argument("--updates-per-step", type=int, default=0)
    ap.add_argument("--episodes", type=int, default=101)
    ap.add_argument("--eval-lattices", type=int, default=101)
    ap.add_argument("--seed", default="24301,57005")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not 0.0 <= a.guide_share <= 1.0:
        ap.error("--guide-share must lie in [0, 1]")
    seed = tuple(int(x) for x in a.seed.split(","))
    cfg = configuration(a.family)
    updates = a.updates_per_step or a.lattices
    runs = {}
    for tag, share in (("plain", None), ("guided", a.guide_share)):
        runs[tag] = train_and_score(cfg, a.steps, a.lattices, updates, share, seed, a.episodes, a.eval_lattices, a.method)
        r = runs[tag]
        print(f"{tag:>7}: {r['env_steps']} steps, {r['updates']} updates, {r['train_seconds']:.1f} s ({r['ms_per_vector_step']:.3f} ms per vector step), "
              f"guided {r['guided_steps']}, inexact {r['inexact_steps']}")
    print(f"{a.family}, trained at p = {P_TRAIN} for {a.steps} steps: average greedy lifetime over {a.episodes} episodes per rate")
    print(f"{'p':>7} {'plain':>10} {'guided':>10} {'1/p':>8}")
    for p in TEST_RATES:
        print(f"{p:7.3f} {runs['plain']['lifetimes'][str(p)]:10.1f} {runs['guided']['lifetimes'][str(p)]:10.1f} {1.0 / p:8.0f}")
    record = dict(family=a.family, p_train=P_TRAIN, steps=a.steps, lattices=a.lattices, updates_per_vector_step=updates, guide_share=a.guide_share, method=a.method,
                  seed=list(seed), test_rates=TEST_RATES, episodes_per_rate=a.episodes, eval_lattices_per_rate=a.eval_lattices,
                  configuration={k: v for k, v in cfg.items() if isinstance(v, (int, float, str, bool, list))}, runs=runs)
    path = a.out or os.path.join(ROOT, "profiles", f"{'guided' if a.method == 'matching' else a.method}_training_{a.family}.json")
    with open(path, "w") as f:
        json.dump(record, f, indent=1, default=lambda o: o.item() if isinstance(o, np.generic) else str(o))
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
