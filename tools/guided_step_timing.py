"""What guided exploration costs per vector step, at bench.py's c3 (d = 5 depolarising, p = 0.011, 4096 lattices, minibatch = the lattice
count): the selection launches alone (device events over repeated calls on one fixed set of lattice states) and whole vector steps with an update
(host clock around a synchronised loop), every variant in this one process, the variants interleaved over several rounds.

    python tools/guided_step_timing.py [--lattices 4096] [--minibatch 0] [--steps 300] [--rounds 3] [--method matching|union_find] [--out FILE]

--method union_find: every variant with a teacher is timed for BOTH teachers, interleaved (the union-find ones carry the suffix " [union_find]"; DESIGN.md
section 16), and the record goes to profiles/union_find_step_timing.json.
"""
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
core_mod = importlib.import_module("deepq-decoding_amd.core")
qnet_mod = importlib.import_module("deepq-decoding_amd.qnet")

C3 = dict(d=5, error_model="DP", use_Y=False, volume_depth=5, p_phys=0.011, p_meas=0.011)
C_LAYERS, FF_LAYERS = [[64, 3, 2], [32, 2, 1], [32, 2, 1]], [[512, 0.2]]
FRACTIONS = [0.0, 0.1, 0.5, 1.0]


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lattices", type=int, default=4096)
    ap.add_argument("--minibatch", type=int, default=0, help="0: the lattice count (bench.py's default)")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--method", default="matching", choices=["matching", "union_find"])
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    methods = [("matching", "")] + ([("union_find", " [union_find]")] if a.method == "union_find" else [])
    N = a.lattices
    a.minibatch = a.minibatch or N
    env = dq.VectorEnv(n_envs=N, seed=(24301, 57005), **C3)
    ev = dq.decoder.Evaluator(5, "DP", False, 5, chunk=N, device=env.device)
    net = qnet_mod.QNetwork(env.obs_shape, C_LAYERS, FF_LAYERS, env.num_actions, dueling=True, max_batch=max(N, a.minibatch), device=env.device)
    core = core_mod.DQNCore(env, net, batch_size=a.minibatch, memory_limit=N * 64, lr=1e-5)
    core.reset_env()
    for _ in range(24):                                                       # lattices in mid-episode, a ring an update can sample
        core.guided_act_and_step(ev, 1.0, 0.5)
    torch.cuda.synchronize()
    # ---- the selection launches alone, on the lattices as they stand -----------------------------------------------------------------------------
    q = core.q_act
    act = torch.empty(N, dtype=torch.int32, device=env.device)
    flags = torch.zeros((2, N), dtype=torch.uint8, device=env.device)
    select = {"select_actions eps=1": lambda: env.select_actions(7, q=q, eps=1.0, out=act),
              "select_actions eps=0": lambda: env.select_actions(7, q=q, eps=0.0, out=act),
              }
    for m, tag in methods:
        select["match_select" + tag] = lambda m=m: env.match_select(ev, out=act, out_inexact=flags[1], method=m)
        for x in FRACTIONS:
            select[f"guided_select eps=1 share={x}" + tag] = lambda x=x, m=m: env.guided_select(ev, 7, q=q, eps=1.0, guide_share=x, out=act, out_guided=flags[0],
                                                                                                  out_inexact=flags[1], method=m)
        select["guided_select eps=0 (greedy)" + tag] = lambda m=m: env.guided_select(ev, 7, q=q, eps=0.0, guide_share=1.0, out=act, out_guided=flags[0],
                                                                                    out_inexact=flags[1], method=m)
    sel_us = {k: [] for k in select}
    for _ in range(a.rounds):
        for k, fn in select.items():
            sel_us[k].append(events_us(fn, 200))
    # ---- whole vector steps with one update each ------------------------------------------------------------------------------------------------------
    def loop(step):
        for _ in range(20):
            step()
            core.update()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            step()
            core.update()
        torch.cuda.synchronize()
        return 1e6 * (time.perf_counter() - t0) / a.steps

    def match_then_step(m):                                                   # section 14's form inside the loop: the matching for EVERY lattice, then a selection
        env.match_select(ev, out=act, out_inexact=flags[1], method=m)
        core.guided_act_and_step(ev, 1.0, 0.0, method=m)

    steps = {"act_and_step + update (eps=1)": lambda: core.act_and_step(1.0),
             "act_and_step + update (eps=0.1)": lambda: core.act_and_step(0.1)}
    for m, tag in methods:
        steps["full match_select + guided step(share=0) + update" + tag] = lambda m=m: match_then_step(m)
        for x in FRACTIONS:
            steps[f"guided_act_and_step(eps=1, share={x}) + update" + tag] = lambda x=x, m=m: core.guided_act_and_step(ev, 1.0, x, method=m)
    step_us = {k: [] for k in steps}
    for _ in range(a.rounds):
        for k, fn in steps.items():
            step_us[k].append(loop(fn))
    summary = lambda d: {k: dict(median_us=float(np.median(v)), runs_us=[float(x) for x in v]) for k, v in d.items()}
    record = dict(config=dict(C3, lattices=N, minibatch=a.minibatch), method=a.method, calls_per_selection_timing=200,
                  steps_per_loop=a.steps, rounds=a.rounds, selection_launch_us=summary(sel_us), vector_step_us=summary(step_us),
                  guided_counts=[int(x) for x in core.guide_counts.cpu().tolist()], device=torch.cuda.get_device_name(0))
    for name, d in (("selection launch, us", record["selection_launch_us"]), ("vector step with update, us", record["vector_step_us"])):
        print(name)
        for k, v in d.items():
            print(f"  {k:60s} {v['median_us']:9.2f}   {['%.2f' % x for x in v['runs_us']]}")
    path = a.out or os.path.join(ROOT, "profiles", "guided_step_timing.json" if a.method == "matching" else "union_find_step_timing.json")
    with open(path, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
    print("wrote", path)
    ev.close()


if __name__ == "__main__":
    main()
