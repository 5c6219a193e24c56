// Action selection on the device: epsilon-greedy with legal-move exploration and optional
// legal-only greedy choice.
//
// Replaces the keras-rl fork's EpsGreedyQPolicy(masked_greedy=...) / GreedyQPolicy(masked_greedy=True)
// (un-vendored; call sites /root/reference/cluster_scripts/d5_dp/0.001/Single_Point_Training_Script.py:110-115,
// 166-167).  Semantics follow README.md:168 ("we restrict the agents random choice to actions which
// are either adjacent to violated stabilizer, or adjacent to previously acted on qubits") and
// README.md:262 (masked_greedy: argmax restricted to the legal actions).
//
// The rule itself is common.h's ("the action-selection rule").  Here 16 lanes cooperate on one lattice (4 lattices per
// wavefront): coalesced reads of the Q row, then the row's first maximum like np.argmax.
#include "common.h"

__global__ __launch_bounds__(256) void policy_kernel(const float* __restrict__ q, const u64* __restrict__ legal, int n,
                                                     int n_actions, u64 T_eps, int masked_greedy, u32 seed0, u32 seed1,
                                                     u32 env_id_base, u64 t, int32_t* __restrict__ action) {
    const int gid = blockIdx.x * blockDim.x + threadIdx.x;
    const int i = gid >> 4, sub = gid & 15;
    if (i >= n) return;          // whole 16-lane groups leave together
    const u64 lo = legal[2 * (size_t)i], hi = legal[2 * (size_t)i + 1];
    u32 w[4];
    dq_policy_words(t, env_id_base + (u32)i, seed0, seed1, w);
    const int a = dq_explores(q, w[1], T_eps) ? dq_explore_action128(lo, hi, w[0])
                                              : dq_row_first_max(q + (size_t)i * n_actions, n_actions, sub, dq_admit128(masked_greedy, lo, hi));
    if (sub == 0) action[i] = a;
}

extern "C" dq_status dq_policy_select(const float* q_dev, const uint64_t* legal_dev, int n, int n_actions, double eps,
                                      int masked_greedy, const uint32_t seed[2], uint32_t env_id_base, uint64_t t,
                                      int32_t* action_dev, void* stream) {
    DQ_REQUIRE(legal_dev && action_dev && seed, DQ_ERR_INVALID, "dq_policy_select: null argument");
    DQ_REQUIRE(n >= 1 && n_actions >= 1 && n_actions <= 128, DQ_ERR_INVALID, "dq_policy_select: bad sizes");
    DQ_REQUIRE(eps >= 0.0 && eps <= 1.0, DQ_ERR_INVALID, "dq_policy_select: eps must be in [0,1]");
    const int threads = n * 16;
    policy_kernel<<<(threads + 255) / 256, 256, 0, (hipStream_t)stream>>>(q_dev, legal_dev, n, n_actions, dq_rate_threshold(eps),
                                                                         masked_greedy, seed[0], seed[1], env_id_base, t, action_dev);
    DQ_LAUNCH_CHECK();
    return DQ_OK;
}
