"""The episode loop of an evaluation, shared by every policy that plays the environment (DQNAgent.test / test_error_rates, decoder.MatchingAgent):
quotas, the block layout of an error-rate sweep, the device-resident records (include/deepq_hip.h dq_test_bookkeeping) and the hard cap on vector
steps.  The policy is a callback that makes one vector step and says where that step's done / was_reset / reward / lifetime are."""
import numpy as np

STEPS_PER_EPISODE_CAP = 1 << 20      # default cap: this many vector steps per episode of the largest quota (days of wall time: a device-side mistake
                                     # that keeps episodes from ending raises instead of spinning; no evaluation comes near it)


def share_quota(n_lattices, nb_episodes):
    """test()'s ceil-share rule: lattice i contributes its first nb_episodes // N (+ 1 for i < nb_episodes % N) episodes."""
    quota = np.full(n_lattices, nb_episodes // n_lattices, dtype=np.int64)
    quota[:nb_episodes % n_lattices] += 1
    return quota


def rate_blocks(n_lattices, error_rates, nb_episodes, p_meas=None):
    """The layout of test_error_rates, validated before anything touches the library: K = len(error_rates) contiguous blocks of m = N // K lattices,
    block k at error_rates[k] (p_meas: None = the same rates, a scalar, or one per entry), each sharing nb_episodes by share_quota; lattices beyond
    K m run at the last rate and record nothing.  Returns (rates, m, p_phys [N], p_meas [N], quota [N])."""
    rates = [float(r) for r in error_rates]
    K, N = len(rates), int(n_lattices)
    if K < 1:
        raise ValueError("test_error_rates: no error rates")
    if K > N:
        raise ValueError(f"test_error_rates: {K} error rates need at least {K} lattices, the environment has {N}")
    if len(set(rates)) != K:
        raise ValueError("test_error_rates: the error rates must be distinct (they key the result)")
    if p_meas is None:
        meas = rates
    elif np.ndim(p_meas) == 0:
        meas = [float(p_meas)] * K
    else:
        meas = [float(r) for r in p_meas]
        if len(meas) != K:
            raise ValueError(f"test_error_rates: {len(meas)} measurement rates for {K} error rates")
    for r in rates + meas:
        if not (0.0 <= r <= 1.0):
            raise ValueError(f"test_error_rates: rate {r!r} is not in [0, 1]")
    m = N // K
    ph, pm = np.empty(N), np.empty(N)
    ph[:K * m] = np.repeat(rates, m); pm[:K * m] = np.repeat(meas, m)
    ph[K * m:], pm[K * m:] = rates[-1], meas[-1]                 # (idle lattices: any valid rate)
    quota = np.zeros(N, dtype=np.int64)
    quota[:K * m] = np.tile(share_quota(m, nb_episodes), K)
    return rates, m, ph, pm, quota


def block_records(rec, k, m):
    """The records of block k of rate_blocks' layout."""
    return rec[(rec[:, 1] >= k * m) & (rec[:, 1] < (k + 1) * m)]


def check_step_cap(nb_max_episode_steps, quota):
    """The cap on the vector steps of one evaluation: nb_max_episode_steps, default STEPS_PER_EPISODE_CAP per episode of the largest quota."""
    if nb_max_episode_steps is None:
        return STEPS_PER_EPISODE_CAP * max(1, int(np.max(quota, initial=0)))
    if isinstance(nb_max_episode_steps, (bool, np.bool_)) or not isinstance(nb_max_episode_steps, (int, np.integer)) or nb_max_episode_steps < 1:
        raise ValueError(f"nb_max_episode_steps must be a positive integer or None, not {nb_max_episode_steps!r}")
    return int(nb_max_episode_steps)


def episode_records(L, dev, stream, n_lattices, quota, step, sync_interval=None, nb_max_episode_steps=None):
    """Runs vector steps until every lattice has delivered its quota of episodes; returns the records int32 [sum(quota), 5] = (vector step, lattice,
    reward bits, length, lifetime), sorted by vector step, then lattice: the serial loop's order.  step(k) makes vector step k on the current
    stream and returns the device tensors (done uint8, was_reset uint8, reward float32, lifetime int32) of that step; the records are appended on
    the device (dq_test_bookkeeping, one small launch per vector step) and the host looks at the record counter every `sync_interval` steps
    only.  After nb_max_episode_steps vector steps (check_step_cap) without the quota RuntimeError is raised."""
    import torch
    from ._lib import check, ptr
    N = int(n_lattices)
    total = int(quota.sum())
    cap = check_step_cap(nb_max_episode_steps, quota)
    quota_d = torch.from_numpy(quota.astype(np.int32)).to(dev)
    ep_reward = torch.zeros(N, dtype=torch.float32, device=dev)
    ep_len = torch.zeros(N, dtype=torch.int32, device=dev)
    records = torch.zeros((max(total, 1), 5), dtype=torch.int32, device=dev)
    counter = torch.zeros(1, dtype=torch.int32, device=dev)
    if sync_interval is None:
        sync_interval = 1 if N == 1 else 64
    k = 0
    while total > 0:
        done, was_reset, reward, lifetime = step(k)
        check(L.dq_test_bookkeeping(ptr(done), ptr(was_reset), ptr(reward), ptr(lifetime), N, k, ptr(quota_d), ptr(ep_reward), ptr(ep_len), ptr(records),
                                    total, ptr(counter), stream()))
        k += 1
        if (k % sync_interval == 0 or k >= cap) and int(counter.item()) >= total:
            break
        if k >= cap:
            raise RuntimeError(f"the evaluation reached its cap of {cap} vector steps with {int(counter.item())} of {total} episodes finished "
                               "(nb_max_episode_steps)")
    rec = records.cpu().numpy()[:total]
    return rec[np.lexsort((rec[:, 1], rec[:, 0]))]                    # by vector step, then lattice
