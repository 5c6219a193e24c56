"""Launch times of the refereed verdict at d = 9 and d = 15: recorded, not gated.

    python tools/wide_verdict_timing.py [--volumes 65536] [--depth 5] [--p 0.006] [--repeats 2] [--distances 9,15] [--none-volumes N] [--out FILE]

The command without options is the one that wrote the committed record.

One process, --volumes DP volumes of --depth rounds per distance (T = window = commit = depth: the union-find row of decode_benchmark_wide), drawn and decoded
by dq_wide_uf_run.  Device events around single launches, the better of --repeats after a first launch of each:
  run                the sample-and-decode launch of the chunk (stream_run_wide_uf_kernel): what a verdict launch stands beside
  unrefereed         verdict_wide_kernel on the union-find residuals: the yardstick
  refereed_faulty    verdict_wide_refereed_kernel on the union-find residuals of streams that end on a faulty round
  refereed_perfect   the same on residuals of streams closed by a perfect round: every wave takes the early exit -- the figure to hold against the yardstick
  refereed_none      the same with no correction (frame NULL): the no_decoder row, every error still on the lattice
with the volumes that reach the referee and the volumes flagged inexact.  Every leg records the volumes it ran on and its ratios PER VOLUME to the
unrefereed launch and to the run.  The last leg runs on the first NONE_VOLUMES_WIDE = 2048 volumes at d >= 13 unless --none-volumes N asks for another
count: with no correction nearly every volume reaches the referee, a few in a hundred hold a cluster of 15 .. 20 defects that walks 2^15 .. 2^20 subsets in
one of the referee's eight scratch-pool slots, and a first attempt at that leg on all 2^16 volumes of d = 15 did not end within 300 s (DESIGN.md section 22:
the time does not scale with the count, and why is not established).  A launch cannot be interrupted: raise the count with that in mind.  Every leg is
printed as it ends.  Writes profiles/wide_verdict_refereed.json."""
import argparse
import importlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
dq = importlib.import_module("deepq-decoding_amd")

SEED = (24301, 57005)
NONE_VOLUMES_WIDE = 2048                                          # the no-correction leg at d >= 13, unless --none-volumes says otherwise


def timed_us(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return 1e3 * e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--volumes", type=int, default=1 << 16)
    ap.add_argument("--depth", type=int, default=5)
    ap.add_argument("--p", type=float, default=0.006)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--distances", default="9,15")
    ap.add_argument("--none-volumes", type=int, default=0, help="volumes of the no-correction leg (default: all at d < 13, 2048 at d >= 13)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    DW = dq.decoder_wide
    n, T = a.volumes, a.depth
    record = dict(device=torch.cuda.get_device_name(0), volumes=n, depth=T, p=a.p, model="DP", repeats=a.repeats, figure="the better of the repeats, us",
                  distances={})
    for d in (int(x) for x in a.distances.split(",")):
        n0 = min(n, a.none_volumes if a.none_volumes > 0 else (NONE_VOLUMES_WIDE if d >= 13 else n))
        ev = DW.WideEvaluator(d, "DP", T, chunk=n)
        new = lambda *shape: torch.empty(shape, dtype=torch.uint8, device="cuda")
        hid, frame, triv = new(n, d, d), new(n, d, d), new(n)
        hid_p, frame_p = new(n, d, d), new(n, d, d)
        verd, flags = new(n), new(n)
        ev.run_into(n, T, T, 0, SEED, a.p, a.p, hid_p, triv, frame_p, final_round="perfect")
        runs = {
            "run": lambda: ev.run_into(n, T, T, 0, SEED, a.p, a.p, hid, triv, frame),
            "unrefereed": lambda: ev.verdict_into(hid, frame, n, verd),
            "refereed_faulty": lambda: ev.verdict_into(hid, frame, n, verd, referee="matching", inexact=flags),
            "refereed_perfect": lambda: ev.verdict_into(hid_p, frame_p, n, verd, referee="matching", inexact=flags),
            "refereed_none": lambda: ev.verdict_into(hid, None, n0, verd, referee="matching", inexact=flags),
        }
        row = {}
        for name, fn in runs.items():
            fn()                                                        # the first launch (and, for "run", the inputs of the others)
            torch.cuda.synchronize()
            m = n0 if name == "refereed_none" else n
            row[name] = v = dict(us=min(timed_us(fn) for _ in range(a.repeats)), volumes=m)
            if name.startswith("refereed"):
                v.update(to_referee=int((verd[:m] & 1 == 0).sum()), inexact=int(flags[:m].sum()), alive=int((verd[:m] & 16 != 0).sum()),
                         success=int((verd[:m] & 8 != 0).sum()))
            v["ns_per_volume"] = 1e3 * v["us"] / m
            if "unrefereed" in row:
                v["per_volume_over_unrefereed"] = v["ns_per_volume"] / row["unrefereed"]["ns_per_volume"]
            v["per_volume_over_run"] = v["ns_per_volume"] / row["run"]["ns_per_volume"]
            print(f"d = {d:2d}  {name:18s} {v['us']:12.1f} us on {m} volumes   per volume x {v.get('per_volume_over_unrefereed', float('nan')):9.2f} of the "
                  f"unrefereed launch   x {v['per_volume_over_run']:7.3f} of the run" + (f"   to the referee {v['to_referee']:6d}  inexact {v['inexact']}" if "to_referee" in v else ""), flush=True)
        assert row["refereed_perfect"]["to_referee"] == 0               # a closed stream's residual is in the code space
        record["distances"][str(d)] = row
        ev.close()
    path = a.out or os.path.join(ROOT, "profiles", "wide_verdict_refereed.json")
    with open(path, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
