"""Launch times of the wide environment's union-find selection (DESIGN.md sections 19, 24 and 26): recorded, not gated.

    python tools/wide_env_uf_timing.py [--lattices 4096] [--p 0.006] [--rounds 5] [--play 8] [--meas-ratio R] [--weights rates|WS,WT] [--correlated] [--referee matching|uf]
                                        [--out FILE]

Per configuration (d = 9 / volume_depth 9 and d = 15 / volume_depth 5, DP) on --lattices mid-episode lattices (--play agent steps of the union-find policy
from a reset): the select launch (env_wide_uf_kernel), dq_envb_step, dq_wide_uf_decode on the same volumes exported as grids with window = commit =
volume_depth (stream_wide_uf_kernel), and the guided launch (env_wide_guided_uf_kernel) at guided fractions 0, 0.1 and 1 (eps = 1, guide_share = the
fraction).  --meas-ratio R plays at p_meas = R p.  --weights adds, on the same records in the same process, the weighted select launch
(env_wide_uf_kernel<true>) under (1, 1), under (2, 1) and under the given pair -- "rates": decoder_wide.uf_weights of (p, p_meas) --, and the weighted guided
launch under that pair at the three fractions; each is reported over the UNWEIGHTED select / guided launch, which is the yardstick; the lattices are still
played by the unweighted policy, and the record goes to profiles/wide_env_uf_weighted_timing.json.  Device events around single launches; the configurations alternate within each of --rounds rounds, and every round ends with one untimed agent
step and a fresh export, so that all launches of a round see the same volumes.  Median, min and max.  Writes profiles/wide_env_uf_timing.json.
--correlated (with --weights) adds the correlated select launch (env_wide_uf_kernel<true, true>) and the correlated guided launch at
the three fractions under the pair with w_corr = 1 and with w_corr = w_space -- with --weights rates the pair of decoder_wide.uf_weights_correlated, which the
weighted launches then take too --, each reported over the WEIGHTED launch at the same pair; the record goes to profiles/wide_env_uf_correlated_timing.json.
--referee plays and steps under the named referee of the wide environment, VectorEnv(referee=...); the record names it and, unless --out
says otherwise, goes to the default file's name with _<referee> in front of .json.  tools/wide_env_referee_timing.py holds the two referees' steps against each other."""
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
SHAPES = ((9, 9), (15, 5))


def timed_us(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return 1e3 * e0.elapsed_time(e1)


class Config:
    def __init__(self, d, depth, n, p, p_meas=None, weights=None, correlated=False, referee=None):
        from oracle import lattice
        self.d, self.depth, self.n = d, depth, n
        p_meas = p if p_meas is None else p_meas
        self.pair = None if weights is None else dq.uf_weights(p, p_meas, "DP") if weights == "rates" else weights
        self.correlated = correlated
        if correlated and weights == "rates":
            self.pair = dq.uf_weights_correlated(p, p_meas, "DP")[:2]
        self.env = dq.VectorEnv(n_envs=n, seed=SEED, d=d, error_model="DP", use_Y=False, volume_depth=depth, p_phys=p, p_meas=p_meas, backend="wide",
                                **({"referee": referee} if referee else {}))
        self.ev = dq.WideEvaluator(d, "DP", window=depth, chunk=n, device=self.env.device)
        dev = self.env.device
        self.action, self.other = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(2))
        self.flag = torch.empty(n, dtype=torch.uint8, device=dev)
        self.q = torch.randn((n, self.env.num_actions), device=dev, generator=torch.Generator(device=dev).manual_seed(5))
        self.frame = torch.empty((n, d, d), dtype=torch.uint8, device=dev)
        order = lattice.Masks(d).order
        self.cell = torch.tensor([a * (d + 1) + b for a, b in order], device=dev)
        self.word = torch.tensor([s >> 6 for s in range(len(order))], device=dev)
        self.bit = torch.tensor([s & 63 for s in range(len(order))], device=dev)
        self.grids = torch.zeros((n, depth, (d + 1) * (d + 1)), dtype=torch.uint8, device=dev)
        self.t = 0
        self.env.reset(write_obs=False)

    def export(self):
        """The lattices' current volumes as syndrome grids uint8 [n, depth, d+1, d+1] (dq_envb_export_state's layout)."""
        W, LW = (self.d * self.d + 63) // 64, self.env.legal_words
        o = 5 * W + 2 + 2 * LW
        vol = self.env.export_state()[:, o:o + self.depth * W].reshape(self.n, self.depth, W)
        self.grids[:, :, self.cell] = ((vol[:, :, self.word] >> self.bit) & 1).to(torch.uint8)

    def play(self):
        self.env.uf_select_wide(self.ev, out=self.action)
        self.env.step(self.action, auto_reset=True, write_obs=False)
        self.t += 1

    def launches(self):
        e, ev, n = self.env, self.ev, self.n
        out = {"select": lambda: e.uf_select_wide(ev, out=self.action),
               "decode": lambda: ev.decode_into(self.grids, n, self.depth, self.depth, self.frame)}
        for share in (0.0, 0.1, 1.0):
            out[f"guided_{share:g}"] = lambda share=share: e.guided_select_wide(ev, self.t, q=self.q, eps=1.0, guide_share=share, out=self.other, out_guided=self.flag)
        if self.pair is not None:                                                        # (into `other`: the step below plays the unweighted action)
            for name, w in (("select_w_1_1", (1, 1)), ("select_w_2_1", (2, 1)), ("select_w_pair", self.pair)):
                out[name] = lambda w=w: e.uf_select_wide(ev, out=self.other, weights=w)
            for share in (0.0, 0.1, 1.0):
                out[f"guided_w_pair_{share:g}"] = lambda share=share: e.guided_select_wide(ev, self.t, q=self.q, eps=1.0, guide_share=share, out=self.other,
                                                                                          out_guided=self.flag, weights=self.pair)
        if self.correlated:
            for wc in dict.fromkeys((1, self.pair[0])):
                out[f"select_c_{wc}"] = lambda wc=wc: e.uf_select_wide(ev, out=self.other, weights=self.pair, correlated=wc)
                for share in (0.0, 0.1, 1.0):
                    out[f"guided_c_{wc}_{share:g}"] = lambda wc=wc, share=share: e.guided_select_wide(
                        ev, self.t, q=self.q, eps=1.0, guide_share=share, out=self.other, out_guided=self.flag, weights=self.pair, correlated=wc)
        out["step"] = lambda: e.step(self.action, auto_reset=True, write_obs=False)      # last: it moves the lattices on
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lattices", type=int, default=4096)
    ap.add_argument("--p", type=float, default=0.006)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--play", type=int, default=8)
    ap.add_argument("--meas-ratio", type=float, default=1.0)
    ap.add_argument("--weights", default=None)
    ap.add_argument("--correlated", action="store_true")
    ap.add_argument("--referee", default=None, choices=["matching", "uf"])
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    weights = None if a.weights is None else a.weights if a.weights == "rates" else tuple(int(x) for x in a.weights.split(","))
    if a.correlated and weights is None:
        ap.error("--correlated times against the weighted launch: give --weights")
    p_meas = min(1.0, a.meas_ratio * a.p)
    cfgs = {f"d{d}_depth{depth}": Config(d, depth, a.lattices, a.p, p_meas, weights, a.correlated, a.referee) for d, depth in SHAPES}
    for c in cfgs.values():
        for _ in range(a.play):
            c.play()
        c.export()
        for name, fn in c.launches().items():                                           # first launches (the step included: one more agent step)
            fn()
        c.t += 1
        c.export()
    torch.cuda.synchronize()
    t = {k: {name: [] for name in c.launches()} for k, c in cfgs.items()}
    live = {k: [] for k in cfgs}
    for _ in range(a.rounds):
        for k, c in cfgs.items():
            for name, fn in c.launches().items():
                t[k][name].append(timed_us(fn))
            live[k].append(float((c.action != c.env.identity_index).float().mean()))
            c.t += 1
            c.export()
    record = dict(device=torch.cuda.get_device_name(0), lattices=a.lattices, p=a.p, p_meas=p_meas, weights=a.weights, correlated=a.correlated, model="DP",
                  referee=a.referee or "matching", played_steps=a.play,
                  timing_rounds=a.rounds, configurations={})
    for k, c in cfgs.items():
        rows = {name: dict(median_us=float(np.median(v)), min_us=float(np.min(v)), max_us=float(np.max(v))) for name, v in t[k].items()}
        ratio = rows["select"]["median_us"] / rows["decode"]["median_us"]
        record["configurations"][k] = dict(d=c.d, volume_depth=c.depth, flip_share=float(np.mean(live[k])), launches=rows, select_over_decode=ratio)
        for name, r in rows.items():
            print(f"{k:12s} {name:12s} median {r['median_us']:10.1f} us  [{r['min_us']:10.1f}, {r['max_us']:10.1f}]")
        print(f"{k:12s} select / decode = {ratio:.3f}")
        if c.pair is not None:                                                           # the weighted launches over the unweighted ones of the same records
            over = {name: r["median_us"] / rows["select" if name.startswith("select") else "guided_" + name.rsplit("_", 1)[1]]["median_us"]
                    for name, r in rows.items() if "_w_" in name}
            record["configurations"][k].update(pair=list(c.pair), weighted_over_unweighted=over)
            print(f"{k:12s} pair {c.pair}: " + "  ".join(f"{name} x {v:.3f}" for name, v in over.items()))
        if c.correlated:                                                                # the correlated launches over the weighted ones at the same pair
            over = {name: r["median_us"] / rows["select_w_pair" if name.startswith("select") else "guided_w_pair_" + name.rsplit("_", 1)[1]]["median_us"]
                    for name, r in rows.items() if "_c_" in name}
            record["configurations"][k].update(correlated_over_weighted=over)
            print(f"{k:12s} pair {c.pair}: " + "  ".join(f"{name} x {v:.3f}" for name, v in over.items()))
    path = a.out or os.path.join(ROOT, "profiles", "wide_env_uf_correlated_timing.json" if a.correlated else
                                 "wide_env_uf_weighted_timing.json" if weights else "wide_env_uf_timing.json")
    if a.referee and not a.out:
        path = path[:-len(".json")] + f"_{a.referee}.json"
    with open(path, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
