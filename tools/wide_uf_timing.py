"""Launch times of the wide union-find stream kernel: recorded, not gated.

    python tools/wide_uf_timing.py [--streams 4096] [--rounds-per-stream 100] [--p 0.005] [--rounds 5] [--closed-leg] [--out FILE]

(a) stream_wide_uf_kernel (one workgroup of four waves per stream) against stream_uf_kernel (one wavefront per stream) on the same d = 7 streams under
    window 14, commit 7: the price of the workgroup form.
(b) stream_wide_uf_kernel alone at d = 9, 11 and 15 under window min(2 d, 32).
Device events around single launches; the launches of all configurations alternate within each of --rounds rounds; median, min and max per
configuration.  The streams are drawn once by dq_wide_uf_run.  Writes profiles/wide_uf_timing.json.
--closed-leg adds, for every configuration, the closed kernel (final_round="perfect") on the same streams, its launches alternating
with the open ones in the same process: the yardstick of a closed launch is the open launch beside it.  The streams above end on a faulty round, whose lone
last-round defects a closed decode has to walk to the spatial boundary or to a partner; so both kernels are also timed on the same lattices' streams drawn
with a perfect last round (dq_wide_uf_run_closed; the keys ending in @perfect), the input a closed decode is meant for.  Writes
profiles/wide_uf_timing_closed.json."""
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
    ap.add_argument("--closed-leg", action="store_true")
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
        if a.closed_leg:
            cout = torch.empty((n, d, d), dtype=torch.uint8, device="cuda")
            runs[f"wide_d{d}_w{w}_closed"] = (lambda ev=ev, syn=syn, cout=cout, c=c: ev.decode_into(syn, n, T, c, cout, final_round="perfect"))
            shapes[f"wide_d{d}_w{w}_closed"] = dict(d=d, window=w, commit=c, kernel="stream_wide_uf_kernel<closed>")
            keep.append(cout)
            syn_p, out_p, cout_p = torch.empty_like(syn), torch.empty_like(out), torch.empty_like(out)
            ev.run_into(n, T, c, 0, SEED, a.p, a.p, torch.empty_like(hid), torch.empty_like(triv), torch.empty_like(frame), syndromes=syn_p, final_round="perfect")
            runs[f"wide_d{d}_w{w}@perfect"] = (lambda ev=ev, syn_p=syn_p, out_p=out_p, c=c: ev.decode_into(syn_p, n, T, c, out_p))
            runs[f"wide_d{d}_w{w}_closed@perfect"] = (lambda ev=ev, syn_p=syn_p, cout_p=cout_p, c=c: ev.decode_into(syn_p, n, T, c, cout_p, final_round="perfect"))
            shapes[f"wide_d{d}_w{w}@perfect"] = dict(d=d, window=w, commit=c, kernel="stream_wide_uf_kernel", streams="perfect last round")
            shapes[f"wide_d{d}_w{w}_closed@perfect"] = dict(d=d, window=w, commit=c, kernel="stream_wide_uf_kernel<closed>", streams="perfect last round")
            keep += [syn_p, out_p, cout_p]
        if d == 7:
            env = dq.VectorEnv(n_envs=1, p_phys=a.p, p_meas=a.p, seed=SEED, d=d, error_model="DP", use_Y=False, volume_depth=5)
            nev = D.Evaluator(d, "DP", False, w, chunk=n, device=env.device)
            nout = torch.empty((n, d, d), dtype=torch.uint8, device="cuda")
            runs[f"narrow_d{d}_w{w}"] = (lambda nev=nev, syn=syn, nout=nout, c=c: nev.stream_uf_into(syn, n, T, c, nout))
            shapes[f"narrow_d{d}_w{w}"] = dict(d=d, window=w, commit=c, kernel="stream_uf_kernel")
            keep += [env, nev, nout]
            if a.closed_leg:
                ncout = torch.empty((n, d, d), dtype=torch.uint8, device="cuda")
                runs[f"narrow_d{d}_w{w}_closed"] = (lambda nev=nev, syn=syn, ncout=ncout, c=c: nev.stream_uf_into(syn, n, T, c, ncout, final_round="perfect"))
                shapes[f"narrow_d{d}_w{w}_closed"] = dict(d=d, window=w, commit=c, kernel="stream_uf_kernel<closed>")
                keep.append(ncout)
                runs[f"narrow_d{d}_w{w}_closed"]()
                runs[f"wide_d{d}_w{w}_closed"]()
                torch.cuda.synchronize()
                assert torch.equal(cout, ncout)                                   # the two closed kernels agree on every stream
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
        print(f"{k:28s} median {np.median(v):10.1f} us  [{np.min(v):10.1f}, {np.max(v):10.1f}]  {1e3 * np.median(v) / (n * T):8.2f} ns per stream-round")
    if a.closed_leg:
        pairs = [(k, k.replace("@", "_closed@") if "@" in k else k + "_closed") for k in shapes if "_closed" not in k]
        record["closed_over_open"] = {k: record["kernels"][kc]["median_us"] / record["kernels"][k]["median_us"] for k, kc in pairs}
        for k, r in record["closed_over_open"].items():
            print(f"{k:28s} closed / open {r:.4f}")
    path = a.out or os.path.join(ROOT, "profiles", "wide_uf_timing_closed.json" if a.closed_leg else "wide_uf_timing.json")
    with open(path, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
