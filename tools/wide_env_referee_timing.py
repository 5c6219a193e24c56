"""The wide environment's step and the refereed verdict under the two referees: recorded, not gated.

    python tools/wide_env_referee_timing.py [--lattices 4096] [--p 0.006] [--rounds 5] [--play 8] [--volumes 65536] [--skip-verdict] [--out FILE]

Step.  Per configuration (d = 9 / volume_depth 9 and d = 15 / volume_depth 5, DP, as tools/wide_env_uf_timing.py prepares them) two environments of --lattices
lattices on the same seed and ids, one per referee, each played --play agent steps of the union-find policy from a reset under its own referee: records
prepared the same way, in one process.  Then --rounds rounds of: one select launch (untimed), dq_envb_step (timed, device events), the referees and the
configurations alternating within a round.  Min, mean and max, and the ratio of the means matching / union-find.
Verdict.  Per d in (9, 15): --volumes depth-5 volumes sampled and decoded by memory_experiment_wide at --p; then the refereed verdict of the union-find row
(residual = hidden XOR frame) and of the no-decoder row (frame NULL) under each referee, --rounds times each.  The matching referee's no-decoder row goes in
decoder_wide.refereed_uncorrected_into's slices where it has to (d >= 13) and is timed as a whole; the union-find referee's is one launch.
Writes profiles/wide_env_referee_timing.json."""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
dq = importlib.import_module("deepq-decoding_amd")
from wide_env_uf_timing import SHAPES, Config, timed_us  # noqa: E402

REFEREES = ("uf", "matching")


def stats(v):
    return dict(min_us=float(np.min(v)), mean_us=float(np.mean(v)), max_us=float(np.max(v)), launches=len(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lattices", type=int, default=4096)
    ap.add_argument("--p", type=float, default=0.006)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--play", type=int, default=8)
    ap.add_argument("--volumes", type=int, default=1 << 16)
    ap.add_argument("--skip-verdict", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    record = dict(device=torch.cuda.get_device_name(0), lattices=a.lattices, p=a.p, model="DP", played_steps=a.play, timing_rounds=a.rounds, step={}, verdict={})
    path = a.out or os.path.join(ROOT, "profiles", "wide_env_referee_timing.json")
    cfgs = {(d, depth, r): Config(d, depth, a.lattices, a.p, referee=r) for d, depth in SHAPES for r in REFEREES}
    for c in cfgs.values():
        for _ in range(a.play + 1):                                                      # (the last one is the first launch of what is timed below)
            c.play()
    torch.cuda.synchronize()
    t = {k: [] for k in cfgs}
    for _ in range(a.rounds):
        for k, c in cfgs.items():
            c.env.uf_select_wide(c.ev, out=c.action)
            t[k].append(timed_us(lambda: c.env.step(c.action, auto_reset=True, write_obs=False)))
    for d, depth in SHAPES:
        rows = {r: stats(t[(d, depth, r)]) for r in REFEREES}
        ratio = rows["matching"]["mean_us"] / rows["uf"]["mean_us"]
        record["step"][f"d{d}_depth{depth}"] = dict(d=d, volume_depth=depth, **rows, matching_over_uf=ratio)
        for r in REFEREES:
            print(f"step    d = {d:2d} depth {depth} {r:9s} mean {rows[r]['mean_us']:12.1f} us  [{rows[r]['min_us']:.1f}, {rows[r]['max_us']:.1f}]")
        print(f"step    d = {d:2d} depth {depth} matching / uf = {ratio:.2f}", flush=True)
    for c in cfgs.values():
        c.ev.close()
        c.env.close()
    with open(path, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
    if not a.skip_verdict:
        DW = dq.decoder_wide
        for d in (9, 15):
            ev = dq.WideEvaluator(d, "DP", 5, chunk=a.volumes)
            _, s = dq.memory_experiment_wide((d, "DP"), a.volumes, 5, window=5, commit=5, p_phys=a.p, seed=(24301, 57005), evaluator=ev, return_streams=True)
            hid, frame, n = s["hidden"], s["frame"], a.volumes
            out = torch.empty(n, dtype=torch.uint8, device=ev.device)
            flags = torch.empty(n, dtype=torch.uint8, device=ev.device)
            launches = {}
            for r in REFEREES:
                launches[f"union_find_row_{r}"] = lambda r=r: ev.verdict_into(hid, frame, n, out, referee=r, inexact=flags)
                launches[f"no_decoder_row_{r}"] = lambda r=r: DW.refereed_uncorrected_into(ev, hid, n, out, flags, r)
            rows = {}
            for name, fn in launches.items():
                fn()                                                                     # the first launch
                torch.cuda.synchronize()
                rows[name] = stats([timed_us(fn) for _ in range(a.rounds)])
                print(f"verdict d = {d:2d} {name:26s} mean {rows[name]['mean_us']:12.1f} us  [{rows[name]['min_us']:.1f}, {rows[name]['max_us']:.1f}]", flush=True)
            for row in ("union_find_row", "no_decoder_row"):
                rows[f"{row}_matching_over_uf"] = rows[f"{row}_matching"]["mean_us"] / rows[f"{row}_uf"]["mean_us"]
            record["verdict"][f"d{d}_depth5"] = dict(d=d, volumes=n, **rows)
            ev.close()
            with open(path, "w") as f:                                                   # after every distance: a time limit loses the one in progress only
                json.dump(record, f, indent=1)
                f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
