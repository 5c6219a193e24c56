"""Launch times of the weighted wide union-find stream kernel beside the unweighted one: recorded, not gated.

    python tools/wide_uf_weighted_timing.py [--streams 4096] [--rounds-per-stream 100] [--p 0.005] [--rounds 7] [--distances 7,9,15] [--out FILE]

Per distance, on the same streams (drawn once by dq_wide_uf_run, DP, p_meas = p) under window min(2 d, 32) and commit (window + 1) // 2, as
tools/wide_uf_timing.py times them: dq_wide_uf_decode (the unit-weight kernel, the yardstick) and dq_wide_uf_decode_weighted at (1, 1), (2, 1), (3, 2) and
(8, 5).  Device events around single launches; the launches of all configurations alternate within each of --rounds rounds of one process; median, min and
max per configuration and the ratio of each weighted median to the unweighted one of its distance.  The weighted launch at (1, 1) must return the
unweighted launch's frames, which is asserted.  Each weighted row also records the mean unit growth rounds per stream: the kernel jumps from one filling
edge to the next, so its passes do not grow with the weights as the unit rounds do.  Writes profiles/wide_uf_weighted_timing.json."""
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
PAIRS = ((1, 1), (2, 1), (3, 2), (8, 5))


def timed_us(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return 1e3 * e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--rounds-per-stream", type=int, default=100)
    ap.add_argument("--p", type=float, default=0.005)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--distances", default="7,9,15")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    DW = dq.decoder_wide
    n, T = a.streams, a.rounds_per_stream
    runs, keep, shapes = {}, [], {}
    for d in (int(x) for x in a.distances.split(",")):
        _, w, c = DW.check_wide_schedule(d, T, None, None)
        ev = DW.WideEvaluator(d, "DP", w, chunk=n)
        syn = torch.empty((n, T, d + 1, d + 1), dtype=torch.uint8, device="cuda")
        hid, frame = (torch.empty((n, d, d), dtype=torch.uint8, device="cuda") for _ in range(2))
        triv = torch.empty(n, dtype=torch.uint8, device="cuda")
        ev.run_into(n, T, c, 0, SEED, a.p, a.p, hid, triv, frame, syndromes=syn)
        out = torch.empty((n, d, d), dtype=torch.uint8, device="cuda")
        key = f"wide_d{d}_w{w}"
        runs[key] = (lambda ev=ev, syn=syn, out=out, c=c: ev.decode_into(syn, n, T, c, out))
        shapes[key] = dict(d=d, window=w, commit=c, kernel="stream_wide_uf_kernel", weights=None, yardstick=key)
        keep += [ev, syn, out]
        for pair in PAIRS:
            wout = torch.empty((n, d, d), dtype=torch.uint8, device="cuda")
            rounds = torch.empty((n, 2), dtype=torch.int32, device="cuda")
            k = f"{key}_weighted_{pair[0]}_{pair[1]}"
            runs[k] = (lambda ev=ev, syn=syn, wout=wout, rounds=rounds, c=c, pair=pair: ev.decode_into(syn, n, T, c, wout, rounds=rounds, weights=pair))
            shapes[k] = dict(d=d, window=w, commit=c, kernel="stream_wide_uf_kernel<weighted>", weights=list(pair), yardstick=key)
            keep += [wout, rounds]
            runs[k]()
            if pair == (1, 1):
                runs[key]()
                torch.cuda.synchronize()
                assert torch.equal(wout, out) and torch.equal(out, frame)         # unit weights: the unweighted kernel's frames, and the fused run's
            torch.cuda.synchronize()
            shapes[k]["mean_unit_rounds_per_stream"] = float(rounds.sum(dim=1).double().mean().item())
    for fn in runs.values():                                                      # first launches
        fn()
    torch.cuda.synchronize()
    t = {k: [] for k in runs}
    for _ in range(a.rounds):
        for k, fn in runs.items():
            t[k].append(timed_us(fn))
    record = dict(device=torch.cuda.get_device_name(0), streams=n, rounds_per_stream=T, p=a.p, model="DP", timing_rounds=a.rounds, kernels={})
    for k, v in t.items():
        record["kernels"][k] = dict(shapes[k], median_us=float(np.median(v)), min_us=float(np.min(v)), max_us=float(np.max(v)),
                                    ns_per_stream_round=float(1e3 * np.median(v) / (n * T)))
    for k, row in record["kernels"].items():
        row["over_unweighted"] = row["median_us"] / record["kernels"][row["yardstick"]]["median_us"]
        print(f"{k:34s} median {row['median_us']:10.1f} us  [{row['min_us']:10.1f}, {row['max_us']:10.1f}]  {row['ns_per_stream_round']:8.2f} ns per stream-round"
              f"  x {row['over_unweighted']:.3f}")
    path = a.out or os.path.join(ROOT, "profiles", "wide_uf_weighted_timing.json")
    with open(path, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
