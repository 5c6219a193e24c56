"""Throughput of batched decoding (DQNAgent.decode / decoder.BatchDecoder, csrc/decode.hip) on real volumes, against the per-call loop.

    python tools/decode_throughput.py [--n 1048576] [--family d5_dp] [--p 0.007] [--chunk 262144] [--loop 200] [--masked] [--obs-form patch]

Volumes: each lattice's first volume of the environment at the agent's own p (VectorEnv.reset, seeded); weights: the shipped agent
tests/golden/keras_weights_<family>_<p>.npz.  Prints one JSON line: volumes/s, iterations per chunk, mean corrections per volume, us per
iteration, the forward kernels' time (dq_prof on the conv and dense chains, one extra decode each) and its share of the decode's wall time
(the rest: pack / select / compact launches, the per-iteration count readback, launch gaps), and the same kind of volumes decoded by the
per-call loop (one dqn.forward-style batch-1 forward per action, README.md:797-818 with environment action planes) on a subset."""
import argparse
import ctypes
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
dq = importlib.import_module("deepq-decoding_amd")
from oracle import lattice  # noqa: E402

C_LAYERS, FF_LAYERS = [[64, 3, 2], [32, 2, 1], [32, 2, 1]], [[512, 0.2]]
FAMILIES = {"d5_x": dict(d=5, error_model="X", use_Y=False, volume_depth=5), "d5_dp": dict(d=5, error_model="DP", use_Y=False, volume_depth=5)}


def volumes(cfg, n, p, seed):
    env = dq.VectorEnv(n_envs=n, p_phys=p, p_meas=p, seed=seed, **cfg)
    env.reset()
    st = env.export_state()[:, 11:11 + cfg["volume_depth"]].cpu().numpy().view(np.uint64)
    env.close()
    d, m = cfg["d"], lattice.Masks(cfg["d"])
    out = np.zeros(st.shape + (d + 1, d + 1), dtype=np.uint8)
    for s, (a, b) in enumerate(m.order):
        out[..., a, b] = ((st >> np.uint64(s)) & np.uint64(1)).astype(np.uint8)
    return out


def forward_loop(net, params, grids, cfg, masked=False):
    """The per-call path: one batch-1 forward and a host copy per action (DQNAgent.forward), environment action planes."""
    d, depth = cfg["d"], cfg["volume_depth"]
    A, layers = lattice.num_actions(d, cfg["error_model"], cfg["use_Y"])
    static = lattice.static_plane(d)
    out = []
    for g in grids:
        obs = np.zeros((depth + layers, 2 * d + 1, 2 * d + 1), np.uint8)
        for j in range(depth):
            obs[j] = static
            obs[j, 0::2, 0::2] = g[j]
        corr = []
        while len(corr) < A - 1:
            x = torch.from_numpy(obs[None]).cuda()
            q = net.forward(params, x, batch=1)[0].cpu().numpy()
            a = int(np.argmax(q))
            if a == A - 1 or a in corr:
                break
            corr.append(a)
            layer, qb = divmod(a, d * d)
            obs[depth + layer, 2 * (qb // d) + 1, 2 * (qb % d) + 1] = 1
        out.append(corr)
    return out


def prof_ms(L, name, fn):
    k = [L.dq_prof_kernel_name(i).decode() for i in range(L.dq_prof_kernel_count())].index(name)
    dq._lib.check(L.dq_prof_arm(k, 1 << 20))
    fn()
    n, ms = ctypes.c_int(0), ctypes.c_double(0)
    dq._lib.check(L.dq_prof_collect(ctypes.byref(n), ctypes.byref(ms)))
    dq._lib.check(L.dq_prof_arm(-1, 0))
    return ms.value, n.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--family", default="d5_dp", choices=sorted(FAMILIES))
    ap.add_argument("--p", default="0.007")
    ap.add_argument("--chunk", type=int, default=1 << 18)
    ap.add_argument("--loop", type=int, default=200, help="volumes decoded by the per-call loop")
    ap.add_argument("--masked", action="store_true")
    ap.add_argument("--obs-form", default=None, choices=["patch", "uint8"])
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    cfg = FAMILIES[args.family]
    d = cfg["d"]
    A, layers = lattice.num_actions(d, cfg["error_model"], cfg["use_Y"])
    shape = (cfg["volume_depth"] + layers, 2 * d + 1, 2 * d + 1)
    fx = np.load(os.path.join(ROOT, "tests", "golden", f"keras_weights_{args.family}_{args.p}.npz"))
    params = torch.from_numpy(np.concatenate([fx[f"w{i}"].reshape(-1) for i in range(12)]).astype(np.float32)).cuda()
    grids = volumes(cfg, args.n, float(args.p), (0xD0, 0xDEC))
    syn = torch.from_numpy(grids).cuda()
    dec = dq.decoder.BatchDecoder(shape, C_LAYERS, FF_LAYERS, A, d, cfg["error_model"], cfg["use_Y"], cfg["volume_depth"],
                                  masked_greedy=args.masked, obs_form=args.obs_form, chunk=args.chunk)
    dec.decode(params, syn[:min(args.n, 4096)], to_host=False)          # warm-up: code objects, first launches
    torch.cuda.synchronize()
    walls = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        res = dec.decode(params, syn, to_host=False)
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - t0)
    wall = min(walls)
    L = dq.lib()
    conv_ms, conv_n = prof_ms(L, "conv_chain_kernel", lambda: (dec.decode(params, syn, to_host=False), torch.cuda.synchronize()))
    dense_ms, dense_n = prof_ms(L, "dense_chain_kernel", lambda: (dec.decode(params, syn, to_host=False), torch.cuda.synchronize()))
    n_corr = res.n_corrections.cpu().numpy()
    iters = res.iterations
    # the per-call loop on a subset
    net1 = dq.QNetwork(shape, C_LAYERS, FF_LAYERS, A, max_batch=1)
    sub = grids[:args.loop]
    forward_loop(net1, params, sub[:2], cfg)
    t0 = time.perf_counter()
    loop = forward_loop(net1, params, sub, cfg) if not args.masked else None
    loop_s = time.perf_counter() - t0
    agree = None
    if loop is not None:
        corr = res.corrections[:args.loop].cpu().numpy()
        agree = sum(int(list(corr[i, :n_corr[i]]) == loop[i]) for i in range(len(loop)))
    fwd_s = (conv_ms + dense_ms) / 1e3
    out = dict(metric="decode_throughput", family=args.family, p=float(args.p), volumes=args.n, chunk=args.chunk, obs_form=dec.obs_form,
               masked_greedy=args.masked, wall_s=round(wall, 5), walls_s=[round(w, 5) for w in walls], volumes_per_s=round(args.n / wall, 1),
               iterations=iters, mean_corrections=round(float(n_corr.mean()), 4),
               us_per_iteration=round(1e6 * wall / max(1, sum(iters)), 2),
               forward_kernels_s=round(fwd_s, 5), forward_launches=[conv_n, dense_n], forward_share=round(fwd_s / wall, 4),
               other_share=round(1 - fwd_s / wall, 4),
               loop_volumes=len(sub), loop_s=round(loop_s, 4), loop_volumes_per_s=round(len(sub) / loop_s, 1) if loop is not None else None,
               loop_agree=agree)
    print(json.dumps(out))
    dec.close()


if __name__ == "__main__":
    main()
