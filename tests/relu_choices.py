"""Which side of a near-zero ReLU did the implementation under test take?  (Test infrastructure; plain module.)

A sample with a ReLU pre-activation within fp32 round-off of 0 (oracle/dqn_oracle.py fragile_samples / fragile_units) may land on either side of that
ReLU in an fp32 implementation, and its gradient then differs from the float64 oracle's by a finite amount.  The implementation's freedom is ONE BIT per
such unit, and the bit can be read back through the backward alone: both backward paths are deterministic and take their masks from the saved training
forward, so a backward whose dq is non-zero on that sample only returns that sample's gradient, which fits the oracle's single-sample gradient under
exactly one of the 2^k on / off assignments of its k near-zero units (several fit only where the unit cannot matter: dropped by dropout, or nothing
downstream of it is on -- they then give the same gradient).  With the bits identified, O.backward(..., relu_on=choices) is the reference for the FULL
minibatch: no sample has to be given dq = 0.

A fit is accepted at the tolerances the gradient tests state, nothing looser: 1e-5 of the largest reference element overall, and per layer tensor
1e-4 of that tensor's largest reference element plus an absolute floor of 1e-7 (taken relative to the largest element where that is below 1, as the
TD tests do, so that the floor never widens with the probe's magnitude)."""
import itertools

import numpy as np

from oracle import dqn_oracle as O

MAX_UNITS = 3            # near-zero units per sample: 2^k oracle gradients each (measured: at most 2 on every input of the suite)


class ReluChoices(dict):
    """{(sample, layer, unit): bool} for O.backward(relu_on=...), with what the identification measured."""
    worst_accepted = 0.0                 # largest error of an accepted fit, relative to the sample's largest gradient element
    smallest_rejected = float("inf")     # smallest error of a rejected assignment (the runner-up gap), same units
    n_samples = 0
    n_indifferent = 0                    # samples where more than one assignment fits (they agree: the unit does not matter)
    n_flipped = 0                        # samples identified on another side of a ReLU than the float64 oracle's own (indifferent samples not counted)


def fit(g, ref, spec):
    """(accepted, overall error / largest |ref| element) of gradient g against the reference gradient ref."""
    g, ref = np.asarray(g, np.float64), np.asarray(ref, np.float64)
    scale = float(np.abs(ref).max())
    err = float(np.abs(g - ref).max())
    if scale == 0.0:
        return err == 0.0, err
    ok = err < 1e-5 * scale
    floor = 1e-7 * min(1.0, scale)
    for (gk, gb), (rk, rb) in zip(spec.split(g), spec.split(ref)):
        for a, b in ((gk, rk), (gb, rb)):
            ok = ok and bool(np.abs(a - b).max() <= 1e-4 * np.abs(b).max() + floor)
    return ok, err / scale


def probe_dq(sample, batch, n_actions):
    """The one-sample dq of the identification: N(0, 1) in every action of `sample` (dense, so that a unit is indifferent only structurally)."""
    dq = np.zeros((batch, n_actions), np.float32)
    dq[sample] = np.random.RandomState(1000003 + sample).randn(n_actions).astype(np.float32)
    return dq


def identify_relu_choices(backward_one, spec, flat, cache, units, label=""):
    """backward_one(dq float32 (B, A)) -> the implementation's flat gradient for the training forward it has saved.  units: O.fragile_units(cache, ...).
    Returns ReluChoices; raises AssertionError where a sample's gradient fits no assignment, or fits two that disagree."""
    assert getattr(spec, "dueling_mean", "row") == "row"
    B, A = cache["head_in"].shape[0], spec.n_actions
    by_sample = {}
    for s, l, u in units:
        by_sample.setdefault(s, []).append((l, u))
    out = ReluChoices()
    for s, lu in sorted(by_sample.items()):
        assert len(lu) <= MAX_UNITS, f"{label}: sample {s} has {len(lu)} near-zero ReLU units (cap {MAX_UNITS})"
        dq = probe_dq(s, B, A)
        g = np.asarray(backward_one(dq), np.float64)
        one = O.sample_cache(cache, [s])
        cands = []
        for bits in itertools.product((False, True), repeat=len(lu)):
            ref = O.backward(spec, flat, one, dq[s:s + 1].astype(np.float64), relu_on={(0, l, u): b for (l, u), b in zip(lu, bits)})
            ok, err = fit(g, ref, spec)
            cands.append((err, ok, bits, ref))
        passing = [c for c in cands if c[1]]
        assert passing, (f"{label}: the gradient of sample {s} fits the oracle under no on/off assignment of its near-zero units {lu}: "
                         f"errors {[f'{c[0]:.2e}' for c in cands]} of the largest element")
        for a, b in itertools.combinations(passing, 2):
            assert fit(a[3], b[3], spec)[0] and fit(b[3], a[3], spec)[0], \
                f"{label}: sample {s}: assignments {a[2]} and {b[2]} of units {lu} both fit and differ from each other"
        best = min(passing, key=lambda c: c[0])
        for (l, u), b in zip(lu, best[2]):
            out[(s, l, u)] = b
        out.n_samples += 1
        out.n_indifferent += len(passing) > 1
        own = tuple(bool(cache["layers"][l]["y"].reshape(B, -1)[s, u] > 0.0) for l, u in lu)
        out.n_flipped += len(passing) == 1 and best[2] != own
        out.worst_accepted = max(out.worst_accepted, best[0])
        out.smallest_rejected = min([out.smallest_rejected] + [c[0] for c in cands if not c[1]])
    print(f"{label}: ReLU choices of {out.n_samples} fragile samples ({len(units)} units, {out.n_indifferent} samples indifferent, {out.n_flipped} on another side than float64) identified: "
          f"worst accepted fit {out.worst_accepted:.2e}, smallest rejected runner-up {out.smallest_rejected:.2e} (of the sample's largest gradient element)")
    return out


def device_relu_choices(net, params, spec, flat, obs, keep, fwd, thr=None, rel=None, cache=None, label=""):
    """The choices of the HIP path that is active on `net` (fused or per-layer: identify once per path).  fwd(): the test's own training forward on
    (params, obs) with the dropout draw `keep`; it is called here, and the backward calls that follow read what it saved.  The probes' scale is not
    declared: the backward measures it from dq.  thr / rel: fragile_units' threshold (give one).  cache: the oracle's training-forward cache where the
    test has it already."""
    import torch
    assert (thr is None) != (rel is None)
    if cache is None:
        _, cache = O.forward(spec, flat, obs, training=True, keep_masks=[keep])
    units = O.fragile_units(cache, rel=rel) if rel is not None else O.fragile_units(cache, thr=thr)
    assert sorted(set(u[0] for u in units)) == np.nonzero(O.fragile_samples(cache, **(dict(rel=rel) if rel is not None else dict(thr=thr))))[0].tolist()
    fwd()
    net.set_grad_scale(0.0)
    out = identify_relu_choices(lambda dq: net.backward(params, torch.from_numpy(dq).to(params.device)).cpu().numpy(), spec, flat, cache, units,
                                label=label or ("fused" if net.fused_enabled else "per-layer"))
    net.check_range()
    return out
