"""The sliding-window union-find decoder measured: one process per table, the forms compared interleaved, medians with spread.

    python tools/memory_experiment.py fused    [--streams 16384] [--rounds 256] [--reps 5] [--final-round faulty|perfect]
    python tools/memory_experiment.py schedule [--streams 65536] [--reps 5]
    python tools/memory_experiment.py rates    [--streams 16384] [--distances 3,5,7] [--rates 0.003,0.007,0.011] [--lengths 10,100,1000]

fused     memory_experiment (dq_stream_run_uf: the rounds are drawn and decoded in one kernel) against sample into a [N, T, G] buffer followed by
          stream_decode's kernel on the same streams: d5_dp, p = 0.007, window 10 / commit 5.  The unfused sampler is the fused kernel's own syndromes
          output taken once (the existing sampler stops at 16 rounds); what is timed is fused run, and sample-to-buffer + decode-from-buffer.
schedule  stream_uf_kernel at T = 16, window 16 against uf_st_kernel on the same 2^16 volumes (one window: the schedule's own cost), then (8, 4) and
          (16, 1) on the same streams.
rates     failure rates with Wilson intervals: depolarising noise, every row the same seed and ids, windows (2d, d) and (d, d), the no-decoder row beside
          them, and for T <= 16 the whole-history decode (window = T) on the same streams.
--final-round perfect (fused, rates): the streams end on a round of perfect measurements.  `fused` then times the closed kernels
beside the open ones on the same streams, launches alternating; `rates` gives the closed failure rates.  The record gets the suffix _closed.
Writes profiles/memory_experiment_<table>.json (or --out)."""
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


def timed_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def stats(v):
    return dict(median_ms=float(np.median(v)), min_ms=float(np.min(v)), max_ms=float(np.max(v)), launches=len(v))


def env_of(d, depth=5, p=0.007, ref=None):
    return dq.VectorEnv(n_envs=1, p_phys=p, p_meas=p, seed=SEED, referee=ref, d=d, error_model="DP", use_Y=False, volume_depth=depth)


def fused(a):
    D = dq.decoder
    d, n, T, w, c, p = 5, a.streams, a.rounds, 10, 5, 0.007
    env = env_of(d, p=p)
    dev = env.device
    ev = D.Evaluator(d, "DP", False, w, chunk=n, device=dev)
    hid, frame, frame2 = (torch.empty((n, d, d), dtype=torch.uint8, device=dev) for _ in range(3))
    triv = torch.empty(n, dtype=torch.uint8, device=dev)
    syn = torch.empty((n, T, d + 1, d + 1), dtype=torch.uint8, device=dev)
    runs = {
        "fused_run": lambda: ev.stream_run_into(env, n, T, c, 0, SEED, p, p, hid, triv, frame),
        "run_writing_syndromes": lambda: ev.stream_run_into(env, n, T, c, 0, SEED, p, p, hid, triv, frame, syndromes=syn),
        "decode_from_buffer": lambda: ev.stream_uf_into(syn, n, T, c, frame2),
    }
    closed = a.final_round == "perfect"
    if closed:                                                                   # the closed kernels beside the open ones, on buffers of their own
        hid_c, frame_c, frame2_c = (torch.empty((n, d, d), dtype=torch.uint8, device=dev) for _ in range(3))
        runs["fused_run_closed"] = lambda: ev.stream_run_into(env, n, T, c, 0, SEED, p, p, hid_c, triv, frame_c, final_round="perfect")
        runs["decode_from_buffer_closed"] = lambda: ev.stream_uf_into(syn, n, T, c, frame2_c, final_round="perfect")
    for fn in runs.values():
        fn()
    torch.cuda.synchronize()
    assert torch.equal(frame, frame2)
    t = {k: [] for k in runs}
    for _ in range(a.reps):
        for k, fn in runs.items():
            t[k].append(timed_ms(fn))
    rec = dict(streams=n, rounds=T, window=w, commit=c, p=p, buffer_bytes=int(syn.numel()), **{k: stats(v) for k, v in t.items()})
    med = {k: float(np.median(v)) for k, v in t.items()}
    # the unfused form = a pass that writes the buffer + a pass that reads it; the writing pass here also decodes, so the sum is an upper bound, and
    # decode_from_buffer alone a lower bound, of "sample then decode"
    rec["unfused_over_fused_upper"] = (med["run_writing_syndromes"] + med["decode_from_buffer"]) / med["fused_run"]
    rec["decode_from_buffer_over_fused"] = med["decode_from_buffer"] / med["fused_run"]
    if closed:
        assert torch.equal(hid, hid_c)
        rec["closed_over_open"] = {k: med[k + "_closed"] / med[k] for k in ("fused_run", "decode_from_buffer")}
    print(json.dumps(rec))
    ev.close()
    return rec


def schedule(a):
    D = dq.decoder
    d, n, T, p = 5, a.streams, 16, 0.007
    env = env_of(d, depth=16, p=p)
    dev = env.device
    vol, _, _ = D.sample_volumes(env, n, chunk=n)
    frames = {k: torch.empty((n, d, d), dtype=torch.uint8, device=dev) for k in ("uf_st_kernel", "w16_c16", "w16_c8", "w8_c4", "w16_c1")}
    evs = {w: D.Evaluator(d, "DP", False, w, chunk=n, device=dev) for w in (16, 8)}
    runs = {
        "uf_st_kernel": lambda: evs[16].uf_into(vol, n, frames["uf_st_kernel"]),
        "w16_c16": lambda: evs[16].stream_uf_into(vol, n, T, 16, frames["w16_c16"]),
        "w16_c8": lambda: evs[16].stream_uf_into(vol, n, T, 8, frames["w16_c8"]),
        "w8_c4": lambda: evs[8].stream_uf_into(vol, n, T, 4, frames["w8_c4"]),
        "w16_c1": lambda: evs[16].stream_uf_into(vol, n, T, 1, frames["w16_c1"]),
    }
    for fn in runs.values():
        fn()
    torch.cuda.synchronize()
    assert torch.equal(frames["uf_st_kernel"], frames["w16_c16"]) and torch.equal(frames["uf_st_kernel"], frames["w16_c8"])      # one window either way
    t = {k: [] for k in runs}
    for _ in range(a.reps):
        for k, fn in runs.items():
            t[k].append(timed_ms(fn))
    rec = dict(volumes=n, rounds=T, p=p, **{k: stats(v) for k, v in t.items()})
    print(json.dumps(rec))
    for e in evs.values():
        e.close()
    return rec


def rates(a):
    D = dq.decoder
    rows = []
    for d in a.distances:
        env = env_of(d, ref="lut")
        for T in a.lengths:
            forms = [("2d_d", min(2 * d, 16), d), ("d_d", d, d)] + ([("whole", T, T)] if T <= 16 else [])
            for name, w, c in forms:
                out = D.memory_experiment(env, a.streams, T, window=w, commit=c, rates=a.rates, seed=SEED, no_decoder=name == "2d_d", chunk=a.streams,
                                          final_round=a.final_round)
                for p, r in out.items():
                    fail = r.failure_rate
                    row = dict(d=d, rounds=T, p=p, form=name, window=w, commit=c, streams=r.counters["volumes"], failure_rate=fail,
                               failure_interval=list(r.failure_interval), per_round=1.0 - (1.0 - fail) ** (1.0 / T), death_rate=r.death_rate)
                    if r.no_decoder is not None:
                        row["no_decoder_failure_rate"] = r.no_decoder.failure_rate
                        row["no_decoder_interval"] = list(r.no_decoder.failure_interval)
                    rows.append(row)
                    print(json.dumps(row), flush=True)
        env.close()
    return dict(seed=list(SEED), model="DP", final_round=a.final_round, rows=rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("table", choices=("fused", "schedule", "rates"))
    ap.add_argument("--streams", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--distances", default="3,5,7")
    ap.add_argument("--rates", default="0.003,0.007,0.011")
    ap.add_argument("--lengths", default="10,100,1000")
    ap.add_argument("--final-round", choices=("faulty", "perfect"), default="faulty")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert a.final_round == "faulty" or a.table != "schedule", "schedule compares with uf_st_kernel, which has no closed form"
    a.streams = a.streams or dict(fused=1 << 14, schedule=1 << 16, rates=1 << 14)[a.table]
    a.distances = [int(x) for x in a.distances.split(",")]
    a.rates = [float(x) for x in a.rates.split(",")]
    a.lengths = [int(x) for x in a.lengths.split(",")]
    rec = dict(device=torch.cuda.get_device_name(0), table=a.table, **dict(fused=fused, schedule=schedule, rates=rates)[a.table](a))
    path = a.out or os.path.join(ROOT, "profiles", f"memory_experiment_{a.table}{'_closed' if a.final_round == 'perfect' else ''}.json")
    with open(path, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
