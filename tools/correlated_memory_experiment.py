"""Memory experiments decoded with the weights of the sampled rates and with the correlated three passes on top, on the same streams (DESIGN.md section
25): recorded, not gated.

    python tools/correlated_memory_experiment.py [--streams 65536] [--rounds 30] [--distances 5,9,13] [--p-phys 0.004] [--p-meas 0.004,0.016,0.04] [--out FILE]

Every cell (d, p_meas) is memory_experiment_wide with final_round="perfect" on --streams DP streams of --rounds rounds under the default window and commit,
once with weights="rates" and once with weights="rates", correlated="rates" (decoder_wide.uf_weights_correlated of the cell's rates), the same seed and
lattice ids for both.  A cell records both failure rates with their Wilson 95 % intervals, the pair and the triple used, the seconds of each call, and
whether the two intervals are disjoint ("resolved").  Writes profiles/memory_experiment_correlated.json."""
import argparse
import importlib
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
dq = importlib.import_module("deepq-decoding_amd")

SEED = (24301, 57005)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--distances", default="5,9,13")
    ap.add_argument("--p-phys", type=float, default=0.004)
    ap.add_argument("--p-meas", default="0.004,0.016,0.04")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    DW = dq.decoder_wide
    record = dict(device=torch.cuda.get_device_name(0), model="DP", streams_per_cell=a.streams, rounds=a.rounds, p_phys=a.p_phys, seed=list(SEED),
                  final_round="perfect", cells={})
    for d in (int(x) for x in a.distances.split(",")):
        _, window, commit = DW.check_wide_schedule(d, a.rounds, None, None)
        ev = DW.WideEvaluator(d, "DP", window, chunk=min(a.streams, DW.DEFAULT_CHUNK))
        for pm in (float(x) for x in a.p_meas.split(",")):
            cell = dict(d=d, window=window, commit=commit, p_meas=pm)
            for name, kw in (("weighted", dict(weights="rates")), ("correlated", dict(weights="rates", correlated="rates"))):
                t0 = time.perf_counter()
                r = DW.memory_experiment_wide((d, "DP"), a.streams, a.rounds, p_phys=a.p_phys, p_meas=pm, seed=SEED, evaluator=ev, final_round="perfect", **kw)
                torch.cuda.synchronize()
                cell[name] = dict(weights=r.weights, failures=r.counters["volumes"] - r.counters["success"], failure_rate=r.failure_rate,
                                  failure_interval=list(r.failure_interval), mean_corrections=r.mean_corrections, seconds=time.perf_counter() - t0)
            u, w = cell["weighted"]["failure_interval"], cell["correlated"]["failure_interval"]
            cell["resolved"] = w[1] < u[0] or u[1] < w[0]
            cell["correlated_over_weighted"] = (cell["correlated"]["failure_rate"] / cell["weighted"]["failure_rate"]
                                                if cell["weighted"]["failure_rate"] > 0 else None)
            record["cells"][f"d{d}_pm{pm:g}"] = cell
            print(f"d = {d:2d}  p_meas = {pm:<6g} weighted {tuple(cell['weighted']['weights'])} {cell['weighted']['failure_rate']:.5f} {u}  correlated "
                  f"{tuple(cell['correlated']['weights'])} {cell['correlated']['failure_rate']:.5f} {w}  resolved: {cell['resolved']}", flush=True)
        ev.close()
    path = a.out or os.path.join(ROOT, "profiles", "memory_experiment_correlated.json")
    with open(path, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
