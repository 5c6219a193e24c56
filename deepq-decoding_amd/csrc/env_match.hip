// The matching decoder as a policy of the environment (include/deepq_hip.h dq_env_match_select): the baseline a trained agent's
// episode lifetime is quoted against.  One wavefront per lattice reads the lattice's record where the environment keeps it (env_dev.h: STATE_FIXED
// words, then the current volume's faulty syndrome words, bit s = stabilizer s in measurement order), forms the defects D_t = S_t xor S_{t-1}
// (S_-1 = 0: what earlier volumes left behind shows up as round-0 defects) of both Pauli components with one ballot per round, runs match_st_dev.h's
// mst_component on either -- the graph, the open future boundary, the tie rules and the 14 / 32 fallback of dq_decode_match, so the frame F is the one
// dq_decode_match returns for this volume -- and answers with ONE action:
//   wanted  = the action indices whose moves XOR to F (X: component 0's qubits on the one layer; DP with use_Y: code 1 / 2 / 3 -> layer 0 / 1 / 2;
//             DP without: X part -> layer 0, Z part -> layer 1, so a Y cell is the X action and the Z action of its qubit)
//   action  = the lowest wanted index that is not in completed_actions, else the identity
// The environment keeps a volume until the identity and clears completed_actions with the new volume, so calling this in front of every step applies
// F one flip per step in ascending index order and then asks for the next volume; nothing is remembered between calls and nothing is written but the
// action (and the flag).  A lattice whose done flag is set gets the identity.  Like match_st_kernel: no scratch pool, no lock, no loop whose exit
// depends on another wave.  The wave's work is env_match_dev.h env_match_wave, shared with env_guide.hip.
#include "env_match_dev.h"

namespace {

__global__ __launch_bounds__(64) void env_match_kernel(MatchStComp c0, MatchStComp c1, const u8* __restrict__ stab, const u64* __restrict__ state, int sw, int n_envs,
                                                       int d2, int depth, int model, int use_Y, int identity, int32_t* __restrict__ action,
                                                       u8* __restrict__ inexact) {
    extern __shared__ __attribute__((aligned(16))) u8 smem[];
    const int i = blockIdx.x, lane = threadIdx.x;
    if (i >= n_envs) return;
    const u64 word = lane < sw ? state[(size_t)i * sw + lane] : 0;             // the whole record in one load (sw = 16 or 32 words)
    int flag;
    const int a = env_match_wave<EnvSolveMatching>(c0, c1, stab, word, d2, depth, model, use_Y, identity, smem, lane, flag);      // env_match_dev.h
    if (lane == 0) { action[i] = a; if (inexact) inexact[i] = (u8)flag; }
}

// The union-find instantiation (dq_env_uf_select): the same rule around uf_dev.h's uf_component, UF_LDS bytes per wave, no flag.
__global__ __launch_bounds__(64) void env_match_uf_kernel(UfComp c0, UfComp c1, const u8* __restrict__ stab, const u64* __restrict__ state, int sw, int n_envs, int d2,
                                                          int depth, int model, int use_Y, int identity, int32_t* __restrict__ action) {
    __shared__ __attribute__((aligned(16))) u8 smem[UF_LDS];
    const int i = blockIdx.x, lane = threadIdx.x;
    if (i >= n_envs) return;
    const u64 word = lane < sw ? state[(size_t)i * sw + lane] : 0;
    int flag;
    const int a = env_match_wave<EnvSolveUnionFind>(c0, c1, stab, word, d2, depth, model, use_Y, identity, smem, lane, flag);
    if (lane == 0) action[i] = a;
}

}  // namespace

dq_status env_match_prepare(const dq_env* env, dq_decode_eval* V, EnvStateView* S, const char* who) {
    dq_status rc = env_state_view(env, S);
    if (rc != DQ_OK) return rc;
    DQ_REQUIRE(S->d == V->d && S->model == V->model && (S->model == DQ_MODEL_X || (S->use_Y != 0) == (V->use_Y != 0)) && S->depth == V->depth, DQ_ERR_INVALID,
               "%s: the environment's lattice (d = %d, model %d, use_Y = %d, volume_depth = %d) is not the evaluator's (d = %d, model %d, "
               "use_Y = %d, volume_depth = %d)", who, S->d, S->model, S->use_Y, S->depth, V->d, V->model, V->use_Y, V->depth);
    DQ_REQUIRE(V->d <= 7 && V->depth >= 1 && V->depth <= MST_MAX_DEPTH && STATE_FIXED + V->depth <= S->sw && S->sw <= 64, DQ_ERR_UNSUPPORTED,
               "%s: d = %d, volume_depth = %d: matching covers d <= 7, depth <= %d", who, V->d, V->depth, MST_MAX_DEPTH);
    return match_st_tables(V);
}

extern "C" {

dq_status dq_env_match_select(dq_env* env, dq_decode_eval* V, int32_t* action_dev, uint8_t* inexact_dev, void* stream) {
    DQ_REQUIRE(env && V && action_dev, DQ_ERR_INVALID, "dq_env_match_select: null argument");
    DQ_REQUIRE((reinterpret_cast<uintptr_t>(action_dev) & 3) == 0, DQ_ERR_INVALID, "dq_env_match_select: action_dev must be 4-byte aligned");
    EnvStateView S;
    const dq_status rc = env_match_prepare(env, V, &S, "dq_env_match_select");
    if (rc != DQ_OK) return rc;
    static unsigned long long attr_devs = 0;                          // per device (common.h dq_device_bit)
    const unsigned long long dev_bit = dq_device_bit();
    if (!(attr_devs & dev_bit)) {
        DQ_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(env_match_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, MST_LDS));
        attr_devs |= dev_bit;
    }
    const MatchStTables* T = V->match_st;
    env_match_kernel<<<S.n_envs, 64, MST_LDS, (hipStream_t)stream>>>(T->comp[0], T->comp[1], T->stab, S.state, S.sw, S.n_envs, S.d * S.d, S.depth, S.model, S.use_Y,
                                                                    S.identity, action_dev, inexact_dev);
    DQ_LAUNCH_CHECK();
    return DQ_OK;
}

dq_status dq_env_uf_select(dq_env* env, dq_decode_eval* V, int32_t* action_dev, void* stream) {
    DQ_REQUIRE(env && V && action_dev, DQ_ERR_INVALID, "dq_env_uf_select: null argument");
    DQ_REQUIRE((reinterpret_cast<uintptr_t>(action_dev) & 3) == 0, DQ_ERR_INVALID, "dq_env_uf_select: action_dev must be 4-byte aligned");
    EnvStateView S;
    const dq_status rc = env_match_prepare(env, V, &S, "dq_env_uf_select");
    if (rc != DQ_OK) return rc;
    const MatchStTables* T = V->match_st;
    env_match_uf_kernel<<<S.n_envs, 64, 0, (hipStream_t)stream>>>(T->uf[0], T->uf[1], T->stab, S.state, S.sw, S.n_envs, S.d * S.d, S.depth, S.model, S.use_Y, S.identity,
                                                                 action_dev);
    DQ_LAUNCH_CHECK();
    return DQ_OK;
}

}  // extern "C"
