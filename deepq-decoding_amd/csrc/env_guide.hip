// Exploration guided by the matching decoder (include/deepq_hip.h dq_env_guided_select): epsilon-greedy action selection in which an
// exploring lattice follows the space-time matching decoder -- the teacher -- with probability guide_share instead of drawing uniformly over its legal set.
// One wavefront per lattice.  All 64 lanes draw the lattice's four policy words, common.h's dq_policy_words (counter t, lattice
// env_id_base + i, stream DQ_STREAM_POLICY, key = seed), so every branch below is wave-uniform:
//   explore = q == NULL || w[1] < T(eps)
//   guided  = explore && w[2] < T(guide_share)             (w[2]: the word the plain rule leaves unused; T = dq_rate_threshold)
//   guided:   the action of dq_env_match_select for the lattice as it stands -- env_match_dev.h env_match_wave, the code env_match_kernel runs: the lowest
//             action of the matching's frame that is not in completed_actions, else the identity; the identity for a lattice whose done flag is set
//   explore:  the k-th legal action, k = umulhi(w[0], n_legal)                                                   (common.h's rule)
//   else:     the first maximum of the Q row, over the legal set when masked_greedy                              (common.h's rule)
// The legal set is the record's (words 6 and 7: what the last reset / step also wrote to its legal_dev).  Only a guided wave loads the matching's tables
// and touches LDS; the others leave after a popcount or one pass over the Q row, so the matching's cost follows eps * guide_share, not the batch.  Every wave
// reserves the matching's MST_LDS bytes all the same (a launch has one LDS size).  Like env_match_kernel: no scratch pool, no lock, no loop whose exit
// depends on another wave; nothing is written but the outputs, by lane 0.
#include "env_match_dev.h"

namespace {

// One lattice by one wave, for either teacher (Solver: env_match_dev.h); smem: the solver's LDS bytes, touched by a guided wave only.
template <class Solver>
static __device__ __forceinline__ void env_guided_select_wave(const typename Solver::Comp& c0, const typename Solver::Comp& c1, const u8* __restrict__ stab,
                                                              const u64* __restrict__ state, int sw, int n_envs, int d2, int depth, int model, int use_Y, int identity,
                                                              int n_actions, const float* __restrict__ q, u64 T_eps, u64 T_share, int masked_greedy, u32 seed0,
                                                              u32 seed1, u32 env_id_base, u64 t, int32_t* __restrict__ action, u8* __restrict__ guided,
                                                              u8* __restrict__ inexact, u8* smem) {
    const int i = blockIdx.x, lane = threadIdx.x;
    if (i >= n_envs) return;
    const u64 word = lane < sw ? state[(size_t)i * sw + lane] : 0;             // the whole record in one load (sw = 16 or 32 words)
    u32 w[4];
    dq_policy_words(t, env_id_base + (u32)i, seed0, seed1, w);
    const u32 w0 = (u32)__builtin_amdgcn_readfirstlane((int)w[0]), w1 = (u32)__builtin_amdgcn_readfirstlane((int)w[1]);
    const u32 w2 = (u32)__builtin_amdgcn_readfirstlane((int)w[2]);
    const bool explore = dq_explores(q, w1, T_eps);
    const bool follow = explore && (u64)w2 < T_share;
    int a, flag = 0;
    if (follow) {
        a = env_match_wave<Solver>(c0, c1, stab, word, d2, depth, model, use_Y, identity, smem, lane, flag);
    } else {
        const u64 lo = wave_bcast64(word, 6), hi = wave_bcast64(word, 7);       // legal_actions
        if (explore) {
            a = dq_explore_action128(lo, hi, w0);
        } else {
            // The first maximum of the row, over the legal set when masked_greedy: common.h's rule (dq_scan_row<64> under dq_admit128, then dq_wave_argmax),
            // with the scan written out here because this kernel is slower through dq_wave_first_max.  A lane takes a candidate that
            // is admitted and either larger than its best or its first; the result does not depend on how many lanes share a row.
            float best = -INFINITY;
            int best_a = 0x7fffffff;
            const float* row = q + (size_t)i * n_actions;
            for (int k = lane; k < n_actions; k += 64) {
                const bool ok = !masked_greedy || (((k < 64 ? lo : hi) >> (k & 63)) & 1);
                const float v = row[k];
                if (ok && (v > best || best_a == 0x7fffffff)) { best = v; best_a = k; }
            }
            dq_wave_argmax(best, best_a);
            a = __builtin_amdgcn_readfirstlane(best_a);
        }
    }
    if (lane == 0) {
        action[i] = a;
        if (guided) guided[i] = follow ? 1 : 0;
        if (inexact) inexact[i] = (u8)flag;
    }
}

__global__ __launch_bounds__(64) void env_guided_select_kernel(MatchStComp c0, MatchStComp c1, const u8* __restrict__ stab, const u64* __restrict__ state, int sw,
                                                               int n_envs, int d2, int depth, int model, int use_Y, int identity, int n_actions,
                                                               const float* __restrict__ q, u64 T_eps, u64 T_share, int masked_greedy, u32 seed0, u32 seed1,
                                                               u32 env_id_base, u64 t, int32_t* __restrict__ action, u8* __restrict__ guided,
                                                               u8* __restrict__ inexact) {
    extern __shared__ __attribute__((aligned(16))) u8 smem[];
    env_guided_select_wave<EnvSolveMatching>(c0, c1, stab, state, sw, n_envs, d2, depth, model, use_Y, identity, n_actions, q, T_eps, T_share, masked_greedy, seed0,
                                             seed1, env_id_base, t, action, guided, inexact, smem);
}

// The union-find teacher (dq_env_guided_select_uf): UF_LDS bytes per wave; the flag it writes is 0.
__global__ __launch_bounds__(64) void env_guided_select_uf_kernel(UfComp c0, UfComp c1, const u8* __restrict__ stab, const u64* __restrict__ state, int sw, int n_envs,
                                                                  int d2, int depth, int model, int use_Y, int identity, int n_actions,
                                                                  const float* __restrict__ q, u64 T_eps, u64 T_share, int masked_greedy, u32 seed0, u32 seed1,
                                                                  u32 env_id_base, u64 t, int32_t* __restrict__ action, u8* __restrict__ guided,
                                                                  u8* __restrict__ inexact) {
    __shared__ __attribute__((aligned(16))) u8 smem[UF_LDS];
    env_guided_select_wave<EnvSolveUnionFind>(c0, c1, stab, state, sw, n_envs, d2, depth, model, use_Y, identity, n_actions, q, T_eps, T_share, masked_greedy, seed0,
                                              seed1, env_id_base, t, action, guided, inexact, smem);
}

// The two entry points: one body.  comp: the solver's tables in MatchStTables; kernel: its kernel; lds: the dynamic LDS of a launch (the matching's MST_LDS;
// 0 for the union-find kernel, which owns a static array: no attribute to set); who names the caller in the messages.
template <class Comp, class Kernel>
dq_status env_guided_select(const char* who, Comp (MatchStTables::*comp)[2], Kernel kernel, size_t lds, dq_env* env, dq_decode_eval* V, const float* q_dev, double eps,
                            double guide_share, int masked_greedy, const uint32_t seed[2], uint64_t t, int32_t* action_dev, uint8_t* guided_dev, uint8_t* inexact_dev,
                            void* stream) {
    DQ_REQUIRE(env && V && seed && action_dev, DQ_ERR_INVALID, "%s: null argument", who);
    DQ_REQUIRE((reinterpret_cast<uintptr_t>(action_dev) & 3) == 0 && (reinterpret_cast<uintptr_t>(q_dev) & 3) == 0, DQ_ERR_INVALID,
               "%s: action_dev and q_dev must be 4-byte aligned", who);
    DQ_REQUIRE(eps >= 0.0 && eps <= 1.0, DQ_ERR_INVALID, "%s: eps must be in [0,1]", who);                                    // (NaN fails both compares)
    DQ_REQUIRE(guide_share >= 0.0 && guide_share <= 1.0, DQ_ERR_INVALID, "%s: guide_share must be in [0,1]", who);
    EnvStateView S;
    const dq_status rc = env_match_prepare(env, V, &S, who);
    if (rc != DQ_OK) return rc;
    DQ_REQUIRE(S.n_actions >= 1 && S.n_actions <= 128, DQ_ERR_UNSUPPORTED, "%s: %d actions do not fit the two-word legal set", who, S.n_actions);
    static unsigned long long attr_devs = 0;                          // one per kernel: a static of a template is per instantiation; a bit per device (dq_device_bit)
    const unsigned long long dev_bit = dq_device_bit();
    if (lds > 0 && !(attr_devs & dev_bit)) {
        DQ_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        attr_devs |= dev_bit;
    }
    const MatchStTables* T = V->match_st;
    kernel<<<S.n_envs, 64, lds, (hipStream_t)stream>>>((T->*comp)[0], (T->*comp)[1], T->stab, S.state, S.sw, S.n_envs, S.d * S.d, S.depth, S.model, S.use_Y, S.identity,
                                                       S.n_actions, q_dev, dq_rate_threshold(eps), dq_rate_threshold(guide_share), masked_greedy, seed[0], seed[1],
                                                       S.env_id_base, t, action_dev, guided_dev, inexact_dev);
    DQ_LAUNCH_CHECK();
    return DQ_OK;
}

}  // namespace

extern "C" {

dq_status dq_env_guided_select(dq_env* env, dq_decode_eval* V, const float* q_dev, double eps, double guide_share, int masked_greedy, const uint32_t seed[2],
                               uint64_t t, int32_t* action_dev, uint8_t* guided_dev, uint8_t* inexact_dev, void* stream) {
    return env_guided_select("dq_env_guided_select", &MatchStTables::comp, env_guided_select_kernel, MST_LDS, env, V, q_dev, eps, guide_share, masked_greedy, seed, t,
                             action_dev, guided_dev, inexact_dev, stream);
}

dq_status dq_env_guided_select_uf(dq_env* env, dq_decode_eval* V, const float* q_dev, double eps, double guide_share, int masked_greedy, const uint32_t seed[2],
                                  uint64_t t, int32_t* action_dev, uint8_t* guided_dev, uint8_t* inexact_dev, void* stream) {
    return env_guided_select("dq_env_guided_select_uf", &MatchStTables::uf, env_guided_select_uf_kernel, 0, env, V, q_dev, eps, guide_share, masked_greedy, seed, t,
                             action_dev, guided_dev, inexact_dev, stream);
}

}  // extern "C"
