"""Launch times of the wide union-find stream kernel: recorded, not gated.

    python tools/wide_uf_timing.py [--streams 4096] [--rounds-per-stream 100] [--p 0.005] [--rounds 5] [--out FILE]

(a) stream_wide_uf_kernel (one workgroup of four waves per stream) against stream_uf_kernel (one wavefront per stream) on the same d = 7 streams under
    window 14, commit 7: the price of the workgroup form.
(b) stream_wide_uf_kernel alone at d = 9, 11 and 15 under window min(2 d, 32).
Device events around single launches; the launches of all configurations alternate within each of --rounds rounds; median, min and max per
configuration.  The streams are drawn once by dq_wide_uf_run.  Writes profiles/wide_uf_timing.json."""
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
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    D, DW = dq.decoder, dq.decoder_wide
    n, T = a.streams, a.rounds_per_stream
    runs, keep, shapes = {}, [], {}
    for d in (7, 9, 11, 15):
        _, w, c = DW.check_wide_schedule(d, T, None, None)
        ev = DW.WideEvaluator(d, "DP", w, chunk=n)
        syn = torch.empty((n, T, d + 1, d + 1), dtype=torch.uint8, device="cuda")
        hid, frame = (torch.empty((n, d, d), dtype=torch.uint8, device="cuda") for _ in range(2))
        triv = torch.empty(n, dtype=torch.uint8, device="cuda")
        ev.run_into(n, T, c, 0, SEED, a.p, a.p, hid, triv, frame, syndromes=syn)
        out = torch.empty((n, d, d), dtype=torch.uint8, device="cuda")
        runs[f"wide_d{d}_w{w}"] = (lambda ev=ev, syn=syn, out=out, c=c: ev.decode_into(syn, n, T, c, out))
        shapes[f"wide_d{d}_w{w}"] = dict(d=d, window=w, commit=c, kernel="stream_wide_uf_kernel")
        keep += [ev, syn, out]
        if d == 7:
            env = dq.VectorEnv(n_envs=1, p_phys=a.p, p_meas=a.p, seed=SEED, d=d, error_model="DP", use_Y=False, volume_depth=5)
            nev = D.Evaluator(d, "DP", False, w, chunk=n, device=env.device)
            nout = torch.empty((n, d, d), dtype=torch.uint8, device="cuda")
            runs[f"narrow_d{d}_w{w}"] = (lambda nev=nev, syn=syn, nout=nout, c=c: nev.stream_uf_into(syn, n, T, c, nout))
            shapes[f"narrow_d{d}_w{w}"] = dict(d=d, window=w, commit=c, kernel="stream_uf_kernel")
            keep += [env, nev, nout]
            runs[f"narrow_d{d}_w{w}"]()
            runs[f"wide_d{d}_w{w}"]()
            torch.cuda.synchronize()
            assert torch.equal(out, nout) and torch.equal(out, frame)            # the two kernels and the fused run agree on every stream
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
        print(f"{k:18s} median {np.median(v):10.1f} us  [{np.min(v):10.1f}, {np.max(v):10.1f}]  {1e3 * np.median(v) / (n * T):8.2f} ns per stream-round")
    path = a.out or os.path.join(ROOT, "profiles", "wide_uf_timing.json")
    with open(path, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
