"""Logical failure of a memory experiment against the physical error rate for a family of distances: the threshold table.

    python tools/threshold_sweep.py [--distances 3,5,...,15] [--rates 0.005,...] [--rounds 60,120] [--streams 4096] [--model DP] [--final-round faulty|perfect] [--referee matching]
                                      [--meas-ratio R] [--weights rates|WS,WT] [--correlated rates|W] [--out FILE]

Every cell (d, p) is memory_experiment_wide on --streams streams with p_meas = p, window min(2 d, 32), commit (window + 1) // 2, one seed and one range of
lattice ids for every cell, at each of the one or two stream lengths of --rounds.  For d <= 7 the same streams also go through decoder.memory_experiment
(the one-wavefront kernels) under the same window and commit, and the counters are asserted equal (with --referee matching `alive` too: the narrow
verdict asks the look-up referee, which the matching referee equals at these sizes).  A cell records per length the counters, the failure
rate f with its Wilson 95 % interval, 1 - (1 - f)^(1 / T) and the seconds it took.  A memory experiment that ends on a faulty round has a floor that does
not depend on T (a lone last-round defect beside the boundary is a data error or a misreading, at equal cost), and the floor grows with
d; with two lengths T1 < T2 the cell therefore also records the failure per round BETWEEN them, 1 - ((1 - f2) / (1 - f1))^(1 / (T2 - T1)), from which a
T-independent floor cancels, with the interval its two Wilson intervals span.  The threshold is read off that figure when it is there.  Writes
profiles/threshold_sweep_<model>.json and prints, per pair of neighbouring distances, the rates between which their curves cross (or that the grid does not
resolve it).  --final-round perfect closes every stream with a round of perfect measurements, which removes that floor: the raw
failure and its per-round figure can then be read directly; the record goes to profiles/threshold_sweep_<model>_closed.json.  --referee matching sends
every verdict through the matching referee: each cell then also records death_rate -- the share of streams on which the environment
would have ended the episode, the referee having completed the residual under perfect measurement -- with its Wilson interval and the volumes flagged
inexact, the crossings are also read on death_rate, and the record goes to profiles/threshold_sweep_<model>_refereed.json.  --meas-ratio R sweeps with
p_meas = R p instead of p_meas = p.  --weights decodes on the weighted graph: "rates" takes decoder_wide.uf_weights of every cell's
own (p, p_meas), WS,WT one pair for every cell; each cell records the pair it was decoded with, the one-wavefront kernels (unit weights only) are then not
compared, and the record's name ends in _weighted.  --correlated decodes the three passes of DESIGN.md section 25: "rates" (with --weights rates or none)
takes decoder_wide.uf_weights_correlated of every cell's rates, W an integer w_corr beside --weights WS,WT; each cell records its triple and the record's
name ends in _correlated."""
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


def per_round(f, rounds):
    return 1.0 - (1.0 - f) ** (1.0 / rounds) if f < 1.0 else 1.0


def between(f1, f2, T1, T2):
    """The failure per round between two stream lengths, from the survival ratio (clamped into [0, 1])."""
    if f1 >= 1.0:
        return 1.0
    return min(1.0, max(0.0, 1.0 - ((1.0 - f2) / (1.0 - f1)) ** (1.0 / (T2 - T1))))


def crossings(table, distances, rates, key, interval):
    """Per pair of neighbouring distances: the first pair of neighbouring rates between which the larger distance stops failing less often in table[d][p][key];
    the intervals tell whether the order on either side is resolved."""
    out = []
    for lo, hi in zip(distances, distances[1:]):
        better = [table[hi][p][key] < table[lo][p][key] for p in rates]
        resolved = [table[hi][p][interval][1] < table[lo][p][interval][0] or table[lo][p][interval][1] < table[hi][p][interval][0] for p in rates]
        cross = next(((rates[k], rates[k + 1]) for k in range(len(rates) - 1) if better[k] and not better[k + 1]), None)
        out.append(dict(distances=[lo, hi], figure=key, larger_distance_fails_less=better, intervals_disjoint=resolved, crossing_between=cross))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--distances", default="3,5,7,9,11,13,15")
    ap.add_argument("--rates", default="0.005,0.01,0.015,0.02,0.025,0.03,0.04")
    ap.add_argument("--rounds", default="60,120")
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--model", default="DP")
    ap.add_argument("--env-id-base", type=int, default=0)
    ap.add_argument("--final-round", choices=("faulty", "perfect"), default="faulty")
    ap.add_argument("--referee", choices=("matching",), default=None)
    ap.add_argument("--meas-ratio", type=float, default=1.0)
    ap.add_argument("--weights", default=None)
    ap.add_argument("--correlated", default=None)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    weights = None if a.weights is None else a.weights if a.weights == "rates" else tuple(int(x) for x in a.weights.split(","))
    correlated = None if a.correlated is None else a.correlated if a.correlated == "rates" else int(a.correlated)
    dq.decoder_wide.check_correlated(correlated, dq.decoder_wide.check_weights(weights, rates=True), rates=True)      # (a ValueError before any cell is run)
    distances = [int(x) for x in a.distances.split(",")]
    rates = [float(x) for x in a.rates.split(",")]
    lengths = sorted(int(x) for x in a.rounds.split(","))
    assert 1 <= len(lengths) <= 2 and len(set(lengths)) == len(lengths), "--rounds takes one or two distinct stream lengths"
    D, DW = dq.decoder, dq.decoder_wide
    record = dict(device=torch.cuda.get_device_name(0), model=a.model, rounds=lengths, streams_per_cell=a.streams, seed=list(SEED),
                  env_id_base=a.env_id_base, p_meas="= p" if a.meas_ratio == 1.0 else f"= {a.meas_ratio:g} p", weights=a.weights, correlated=a.correlated, final_round=a.final_round, referee=a.referee, cells={}, narrow_checked=[])
    table = {}
    for d in distances:
        _, window, commit = DW.check_wide_schedule(d, lengths[0], None, None)
        ev = DW.WideEvaluator(d, a.model, window, chunk=a.streams)
        env = dq.VectorEnv(n_envs=1, p_phys=rates[0], p_meas=rates[0], seed=SEED, d=d, error_model=a.model, use_Y=False, volume_depth=5) if d <= 7 and weights is None and correlated is None else None
        table[d] = {}
        for p in rates:
            pm = min(1.0, a.meas_ratio * p)
            cell = dict(window=window, commit=commit, p_meas=pm, per_length={})
            for T in lengths:
                t0 = time.perf_counter()
                r = DW.memory_experiment_wide((d, a.model), a.streams, T, p_phys=p, p_meas=pm, seed=SEED, env_id_base=a.env_id_base, evaluator=ev,
                                              final_round=a.final_round, referee=a.referee, weights=weights, correlated=correlated)
                cell["weights"] = r.weights
                torch.cuda.synchronize()
                one = r.summary()
                one.update(failure_per_round=per_round(r.failure_rate, T), failure_per_round_interval=[per_round(x, T) for x in r.failure_interval],
                           seconds=time.perf_counter() - t0)
                cell["per_length"][str(T)] = one
                if env is not None:                                               # the one-wavefront kernels on the same streams: the same counters
                    narrow = D.memory_experiment(env, a.streams, T, window=window, commit=commit, p_phys=p, p_meas=pm, seed=SEED, env_id_base=a.env_id_base,
                                                 final_round=a.final_round)
                    keys = ("volumes", "trivial", "in_codespace", "success", "identity", "repeat", "stopped", "corrections")
                    if a.referee:                                                 # the narrow verdict asks the look-up referee, which the matching referee equals at d <= 7
                        keys += ("alive",)
                    assert all(narrow.counters[k] == one[k] for k in keys), (d, p, T, narrow.counters, one)       # (unrefereed: alive is not comparable)
            last = cell["per_length"][str(lengths[-1])]
            cell.update(failure_rate=last["failure_rate"], failure_interval=last["failure_interval"])
            line = "  ".join(f"T = {T}: {cell['per_length'][str(T)]['failure_rate']:.5f}" for T in lengths)
            if a.referee:
                cell.update(death_rate=last["death_rate"], death_interval=last["death_interval"], inexact=last.get("inexact", 0))
                line += "  death " + "  ".join(f"T = {T}: {cell['per_length'][str(T)]['death_rate']:.5f}" for T in lengths)
            if len(lengths) == 2:
                (T1, T2), first = lengths, cell["per_length"][str(lengths[0])]
                cell["failure_per_round_between"] = between(first["failure_rate"], last["failure_rate"], T1, T2)
                ends = [between(first["failure_interval"][1], last["failure_interval"][0], T1, T2), between(first["failure_interval"][0], last["failure_interval"][1], T1, T2)]
                cell["failure_per_round_between_interval"] = [min(ends), max(ends)]
                line += f"  per round between {cell['failure_per_round_between']:.3e} [{min(ends):.3e}, {max(ends):.3e}]"
            table[d][p] = cell
            record["cells"][f"d{d}_p{p}"] = cell
            print(f"d = {d:2d}  p = {p:<6g} {line}  {sum(x['seconds'] for x in cell['per_length'].values()):.2f} s", flush=True)
        ev.close()
        if env is not None:
            env.close()
            record["narrow_checked"].append(d)
    figures = [("failure_rate", "failure_interval")] + ([("failure_per_round_between", "failure_per_round_between_interval")] if len(lengths) == 2 else [])
    if a.referee:
        figures.append(("death_rate", "death_interval"))
    record["crossings"] = [c for key, interval in figures for c in crossings(table, distances, rates, key, interval)]
    for c in record["crossings"]:
        lo, hi = c["distances"]
        where = (f"between p = {c['crossing_between'][0]} and {c['crossing_between'][1]}" if c["crossing_between"] else
                 "not inside the grid" + (" (the larger distance fails less at every rate)" if all(c["larger_distance_fails_less"]) else ""))
        print(f"{c['figure']}, d = {lo} / {hi}: the curves cross {where}; intervals disjoint at {sum(c['intervals_disjoint'])} of {len(rates)} rates")
    path = a.out or os.path.join(ROOT, "profiles", f"threshold_sweep_{a.model.lower()}{'_closed' if a.final_round == 'perfect' else ''}{'_refereed' if a.referee else ''}{'_weighted' if weights else ''}{'_correlated' if correlated else ''}.json")
    with open(path, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
