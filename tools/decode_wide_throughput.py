"""Throughput of batched agent decoding at d = 9 .. 15 (DQNAgent.decode_benchmark_wide / decoder_wide.WideBatchDecoder, csrc/decode_wide.hip) on sampled
volumes, against the per-call loop.

    python tools/decode_wide_throughput.py [--d 9 11 13 15] [--n 65536] [--depth 5] [--p 0.006] [--loop 200] [--out profiles/decode_wide_throughput.json]
    python tools/decode_wide_throughput.py --d 15 --n 16384 --stats-csv <rocprofv3 ..._kernel_stats.csv> --merge-into <json>   # merge a traced run

No trained agent exists beyond d = 7, so the network is the test suite's stand-in (tests/decode_wide_ref.py sensitive_network: Glorot weights whose first
convolution weighs the action planes 30 times, the identity shifted so that a tenth of the volumes stop at once): the figures describe the machinery -- rows,
forwards, selection, compaction -- at a plausible sequence length, not a decoder's quality.  Per d one JSON record: volumes/s of the decode phase, iterations
per chunk, mean corrections, the wall-time phases of decode_benchmark_wide (run = sampling + union-find, decode, verdict), the chunk the footprint rule chose,
and the per-call compute_q_values loop on --loop of the same volumes.  --stats-csv: the kernel shares of pack / select / compact against the forwards and the
pack kernel's written bytes per second, from a `rocprofv3 --kernel-trace --stats` run of this tool (a run of its own: tracing slows the loop)."""
import argparse
import csv
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
dq = importlib.import_module("deepq-decoding_amd")
import decode_ref as R  # noqa: E402
import decode_wide_ref as WR  # noqa: E402

SEED = (0xD0, 0xDEC)
HBM_PEAK_GBPS = 8000.0                                               # MI355X: 8 TB/s


def make_agent(cfg, weights, p):
    env = dq.VectorEnv(n_envs=2, p_phys=p, p_meas=p, seed=SEED, **cfg)
    model = dq.build_convolutional_nn(WR.C_LAYERS, WR.FF_LAYERS, env.obs_shape, env.num_actions)
    agent = dq.DQNAgent(model=model, nb_actions=env.num_actions, memory=dq.SequentialMemory(limit=64, window_length=1), nb_steps_warmup=100,
                        target_model_update=100, policy=dq.GreedyQPolicy(masked_greedy=True), test_policy=dq.GreedyQPolicy(masked_greedy=True),
                        gamma=0.99, enable_dueling_network=True)
    agent.compile(dq.Adam(lr=1e-4))
    agent._bind(env)
    agent.model.set_weights(weights)
    return agent, env


def kernel_shares(path, packed_volumes, row_bytes):
    """Shares of the kernel time in a rocprofv3 --stats table (Name, Calls, TotalDurationNs, ...): the decode's pack / select / compact, the sampling and
    union-find kernel, the scoring kernels, and the rest (the network's forwards and weight packing); and the pack kernel's write rate over the
    `packed_volumes` rows of `row_bytes` the traced process packed."""
    groups = {"pack": ("decode_wide_pack_kernel",), "select": ("decode_wide_select_kernel",), "compact": ("decode_wide_compact_kernel",),
              "sampling_union_find": ("uf_",), "scoring": ("verdict", "count")}
    total, ns_of, calls = 0.0, {k: 0.0 for k in groups}, {k: 0 for k in groups}
    for r in csv.DictReader(open(path)):
        ns = float(r["TotalDurationNs"])
        total += ns
        for k, keys in groups.items():
            if any(key in r["Name"] for key in keys):
                ns_of[k] += ns
                calls[k] += int(r["Calls"])
                break
    out = {f"{k}_share": round(v / total, 5) for k, v in ns_of.items()}
    out["network_share"] = round(1.0 - sum(ns_of.values()) / total, 5)
    out["kernel_total_ms"] = round(total / 1e6, 3)
    out["calls"] = calls
    if ns_of["pack"] > 0:
        out["pack_ms_total"] = round(ns_of["pack"] / 1e6, 4)
        out["pack_row_bytes_written"] = int(packed_volumes) * int(row_bytes)
        out["pack_written_GBps"] = round(out["pack_row_bytes_written"] / ns_of["pack"], 2)          # bytes per ns
        out["pack_share_of_hbm_peak"] = round(out["pack_written_GBps"] / HBM_PEAK_GBPS, 4)
    return out


def merge_trace(args):
    """Attaches the kernel shares of a traced run (the same --d, --n, --repeats) to its record in the JSON file --merge-into."""
    out = json.load(open(args.merge_into))
    for rec in out["records"]:
        if rec["d"] == args.d[0]:
            rec["kernel_trace"] = dict(volumes=args.n, **kernel_shares(args.stats_csv, min(args.n, 1024) + args.repeats * args.n, rec["row_bytes"]))
    with open(args.merge_into, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")


def one(d, args):
    cfg = dict(d=d, error_model="DP", use_Y=False, volume_depth=args.depth)
    p = args.p
    _, streams = dq.memory_experiment_wide((d, "DP"), 150, rounds=args.depth, window=args.depth, commit=args.depth, p_phys=0.03, seed=SEED,
                                           return_streams=True)
    spec, flat = WR.sensitive_network(cfg, streams["syndromes"].cpu().numpy())
    agent, env = make_agent(cfg, WR.weights_of(spec, flat), p)
    lat = (d, "DP", False, args.depth)
    kw = dict(p_phys=p, seed=SEED, baseline="union_find")
    agent.decode_benchmark_wide(lat, min(args.n, 1024), **kw)                                   # warm-up: code objects, first launches
    best = None
    for _ in range(args.repeats):
        t = {}
        t0 = time.perf_counter()
        res, uf = agent.decode_benchmark_wide(lat, args.n, timings=t, return_volumes=True, **kw)
        torch.cuda.synchronize()
        t["wall"] = time.perf_counter() - t0
        if best is None or t["decode"] < best[0]["decode"]:
            best = (t, res, uf)
    t, res, uf = best
    dec = agent._wide_decoder
    iters = res.decode.iterations
    row_bytes = int(np.prod(env.obs_shape))
    rec = dict(d=d, error_model="DP", volume_depth=args.depth, p=p, volumes=args.n, num_actions=int(env.num_actions), chunk=dec.chunk,
               footprint_bytes_per_volume=dq.decoder_wide.decode_wide_footprint(env.obs_shape, WR.C_LAYERS, WR.FF_LAYERS, env.num_actions),
               row_bytes=row_bytes, masked_greedy=True, phases_s={k: round(v, 5) for k, v in t.items()},
               volumes_per_s=round(args.n / t["decode"], 1), iterations=iters, us_per_iteration=round(1e6 * t["decode"] / max(1, sum(iters)), 2),
               mean_corrections=round(res.mean_corrections, 4), status=res.status_histogram, agent_failure_rate=round(res.failure_rate, 5),
               union_find_failure_rate=round(uf.failure_rate, 5))
    if args.loop > 0:                                                # the per-call loop on the first volumes of the same batch
        sub = res.volumes[:args.loop].cpu().numpy()
        R.decode_volume(sub[0], agent.compute_q_values, d, "DP", False, True)
        t0 = time.perf_counter()
        loop = [R.decode_volume(g, agent.compute_q_values, d, "DP", False, True)[0] for g in sub]
        loop_s = time.perf_counter() - t0
        corr, ncorr = res.decode.corrections[:args.loop].cpu().numpy(), res.decode.n_corrections[:args.loop].cpu().numpy()
        rec.update(loop_volumes=len(sub), loop_s=round(loop_s, 4), loop_volumes_per_s=round(len(sub) / loop_s, 1),
                   loop_agree=sum(int(list(map(int, corr[i, :ncorr[i]])) == loop[i]) for i in range(len(sub))),
                   speedup_over_loop=round((args.n / t["decode"]) / (len(sub) / loop_s), 1))
    agent._wide_decoder.close()
    agent._wide_decoder = None
    env.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", type=int, nargs="+", default=[9, 11, 13, 15])
    ap.add_argument("--n", type=int, default=1 << 16)
    ap.add_argument("--depth", type=int, default=5)
    ap.add_argument("--p", type=float, default=0.006)
    ap.add_argument("--loop", type=int, default=200, help="volumes decoded by the per-call loop")
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--stats-csv", default=None)
    ap.add_argument("--merge-into", default=None, help="with --stats-csv: no measurement, only the merge into this JSON file")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.stats_csv:
        return merge_trace(args)
    out = dict(metric="decode_wide_throughput", network="tests/decode_wide_ref.py sensitive_network (no trained agent exists beyond d = 7)",
               hbm_peak_GBps=HBM_PEAK_GBPS, records=[one(d, args) for d in args.d])
    text = json.dumps(out, indent=1)
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
