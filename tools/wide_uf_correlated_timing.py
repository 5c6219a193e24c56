"""Launch times of the correlated wide union-find stream kernel beside the weighted one: recorded, not gated.

    python tools/wide_uf_correlated_timing.py [--streams 4096] [--rounds-per-stream 100] [--p 0.005] [--rounds 7] [--distances 7,9,15] [--out FILE]

Per distance, on the same streams (drawn once by dq_wide_uf_run, DP, p_meas = p) under window min(2 d, 32) and commit (window + 1) // 2, the shapes of
tools/wide_uf_weighted_timing.py: dq_wide_uf_decode_weighted at (4, 4) and (8, 7) (the yardsticks) and dq_wide_uf_decode_correlated at the same pairs with
w_corr = 1, and with w_corr = w_space, whose frames must be the weighted launch's, which is asserted.  Device events around single launches; the launches
of all configurations alternate within each of --rounds rounds of one process; median, min and max per configuration and the ratio of each correlated
median to the weighted one of its distance and pair.  Each row also records the mean unit growth rounds per stream (passes 1 and 2 for the correlated
rows) and the share of streams whose frame differs from the yardstick's.  Writes profiles/wide_uf_correlated_timing.json."""
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
PAIRS = ((4, 4), (8, 7))


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
        keep += [ev, syn]
        for pair in PAIRS:
            yard = f"wide_d{d}_w{w}_weighted_{pair[0]}_{pair[1]}"
            frames = {}
            for name, weights in ((yard, pair), (f"{yard}_correlated_1", pair + (1,)), (f"{yard}_correlated_{pair[0]}", pair + (pair[0],))):
                out = torch.empty((n, d, d), dtype=torch.uint8, device="cuda")
                rounds = torch.empty((n, 2), dtype=torch.int32, device="cuda")
                runs[name] = (lambda ev=ev, syn=syn, out=out, rounds=rounds, c=c, weights=weights: ev.decode_into(syn, n, T, c, out, rounds=rounds,
                                                                                                                  weights=weights))
                shapes[name] = dict(d=d, window=w, commit=c, kernel="stream_wide_uf_kernel<" + ("weighted>" if len(weights) == 2 else "correlated>"),
                                    weights=list(weights), yardstick=yard)
                keep += [out, rounds]
                runs[name]()
                torch.cuda.synchronize()
                frames[name] = out
                shapes[name]["mean_unit_rounds_per_stream"] = float(rounds.sum(dim=1).double().mean().item())
                shapes[name]["frames_differing_from_yardstick"] = float((out != frames[yard]).flatten(1).any(dim=1).double().mean().item())
            assert torch.equal(frames[f"{yard}_correlated_{pair[0]}"], frames[yard])       # w_corr = w_space: the weighted launch's frames
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
        row["over_weighted"] = row["median_us"] / record["kernels"][row["yardstick"]]["median_us"]
        print(f"{k:44s} median {row['median_us']:10.1f} us  [{row['min_us']:10.1f}, {row['max_us']:10.1f}]  {row['ns_per_stream_round']:8.2f} ns per stream-round"
              f"  x {row['over_weighted']:.3f}  differing {row['frames_differing_from_yardstick']:.3f}")
    path = a.out or os.path.join(ROOT, "profiles", "wide_uf_correlated_timing.json")
    with open(path, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
