// The union-find decoder as a policy and as a teacher of the WIDE environment, any odd d in 3 .. 15 (include/deepq_hip.h dq_envb_uf_select,
// dq_envb_guided_select_uf): env_match.hip's and env_guide.hip's rules on env_big.hip's lattice record, with uf_wide_dev.h's component
// decode in the solver's place.  One workgroup of UFW_THREADS threads per lattice, dynamic LDS from ufw_layout(n, d^2, volume_depth).
//   env_wide_uf_kernel          every lattice: the lowest action of the union-find frame of the lattice's current volume that is not in completed_actions,
//                               else the identity; the identity for a lattice whose done bit is set
//   env_wide_guided_uf_kernel   epsilon-greedy selection whose exploring lattices follow that action with probability guide_share
// The record (x[W] z[W] acted[W] round meta completed[LW] legal[LW] volume[depth][W]) is read in place and never written.  Thread 128 c + j picks node j of
// component c out of round t's words, D_t = S_t xor S_(t-1) goes into the LDS ring as stream_wide_uf_kernel stores it, and the whole volume is decoded as one
// last window (final, commit = depth): union_find_ref on the volume.  Every exit in front of or between barriers is decided by a kernel argument, the record's
// meta word or the Philox words every thread draws alike.  No scratch pool, no lock, no loop that waits on another workgroup.
// The action body and the two kernels are templates on (Weighted, Corr), three variants of each kernel, and differ only in what uf_wide.h's ufw_setup and
// ufw_window do for the flags:
//   <false, false>  unit weights (dq_envb_uf_select, dq_envb_guided_select_uf)
//   <true, false>   DESIGN.md section 24 (dq_envb_*_weighted): the lattice's own (w_space, w_time) -- the launch's pair or the lattice's two bytes of a uint8
//                   [n_envs][2] array --, so the last round's time edges to B cost w_time
//   <true, true>    DESIGN.md section 26 (dq_envb_*_correlated): section 25's three passes on that window with the lattice's own (w_space, w_time, w_corr), the
//                   launch's triple or three bytes of a uint8 [n_envs][3] array; the dynamic LDS holds the two masks behind ufw_layout's bytes
// The flags are compile-time: the unit-weight kernels carry no code of the other two.  env_wide_uf_kernel_of is the one map from (guided, mode) to a kernel.
#include "uf_wide.h"
#include "env_big_view.h"

#define EWU_NONE 0x7fffffff
#define EWU_MAX_DEPTH 16                                         // dq_envb_create's limit on volume_depth

namespace {

struct EnvUfArgs {
    UfwComp c0, c1;
    const u8* node_stab;        // [2][128] node -> stabilizer in measurement order
    const u64* state;           // [n_envs][sw]
    int sw, W, LW, n_envs, n, d2, depth, model, use_Y, identity, n_actions;
    int32_t* action;            // [n_envs]
    // the guided form
    const float* q;             // [n_envs][n_actions] or NULL
    u64 T_eps, T_share, t;
    int masked_greedy;
    u32 seed0, seed1, env_id_base;
    u8* guided;                 // [n_envs] or NULL
};

// The arguments of a weighted or a correlated launch are the unweighted ones with the weights behind them; the unit-weight kernels take EnvUfArgs itself.
struct EnvUfArgsWeighted : EnvUfArgs {
    UfwWeights w;
};
template <bool Weighted>
using EnvUfArgsOf = std::conditional_t<Weighted, EnvUfArgsWeighted, EnvUfArgs>;

// The select body for lattice i, whose record is `rec`, by the whole workgroup; returns the action to every thread.  Weighted, Corr: the lattice's own pair or
// triple (uf_wide.h ufw_setup); the dynamic LDS of a correlated launch holds the two masks behind the layout's bytes.  The growth's event reduction takes the
// spare word s_acc[7], since s_acc[6] is this body's own (below).
template <bool Weighted, bool Corr>
static __device__ __forceinline__ int env_wide_uf_action(const EnvUfArgsOf<Weighted>& p, size_t i, const u64* __restrict__ rec, u8* smem, int tid) {
    int W = p.W, depth = p.depth, identity = p.identity;
    const int O_META = 3 * W + 1;
    int o_comp = 3 * W + 2;
    if ((rec[O_META] >> 32) & 1) return identity;                   // done: workgroup-uniform, no barrier passed yet
    const UfwSetup S = ufw_setup<Weighted, Corr>(p, i, p.n, p.d2, depth);
    const UfwHead H = ufw_head(smem, S.L);
    u32 *s_frame = H.s_frame, *s_carry = H.s_carry, *s_ring = H.s_ring;
    int* s_acc = H.s_acc;
    int row_stride = depth * UFW_ROW_WORDS;
    const int my_stab = (tid & (UFW_NODE_SLOTS - 1)) < p.n ? p.node_stab[tid] : 255;
    const bool mine = my_stab < 255;
    const u64* vp = rec + o_comp + 2 * p.LW + (mine ? my_stab >> 6 : 0);       // (a thread without a node reads word 0 of its own volume and masks it)
    const int my_bit = my_stab & 63;
    const u64* comp = rec + o_comp;
    int d2 = p.d2, model = p.model, use_Y = p.use_Y;
    UFW_IN_VGPR(W); UFW_IN_VGPR(depth); UFW_IN_VGPR(identity); UFW_IN_VGPR(row_stride); UFW_IN_VGPR(comp); UFW_IN_VGPR(d2); UFW_IN_VGPR(model);
    UFW_IN_VGPR(use_Y);
    if (tid < 2 * UFW_FRAME_WORDS) s_frame[tid] = 0;
    if (tid < 2 * UFW_ROW_WORDS) s_carry[tid] = 0;
    if (tid < 8) s_acc[tid] = tid == 6 ? EWU_NONE : 0;             // [6]: the lowest wanted action that is not completed; [7]: the weighted growth's s_event
    int prev = 0, nd = 0;
    for (int t = 0; t < depth; ++t) {
        const int cur = (int)((vp[(size_t)t * W] >> my_bit) & 1);
        wide_rows(mine ? cur : 0, prev, tid, s_ring + t * UFW_ROW_WORDS, s_ring + row_stride + t * UFW_ROW_WORDS, nd);
    }
    __syncthreads();
    UfwGraph G = ufw_graph_in_vgpr(p.n, p.d2);
    const UfwEnds E = ufw_ends_in_vgpr(p.c0, p.c1);
    G.depth = depth; G.B = depth * G.n; G.NN = G.B + 1; G.NE = depth * G.per_round;
    // the whole volume as one last open window; the X model has no action layer for component 1: its frame is not asked for
    ufw_window<false, Weighted, Corr>(G, E, smem, S, H, tid, row_stride, depth, true, model == DQ_MODEL_X ? 1 : 2, s_acc + 7);
    // decoder.frame_to_actions' rule; thread q < d^2 holds qubit q's cell of the two frames (the component's last barrier is behind every thread, or its
    // frame words still hold the zeros stored in front of the first one)
    int best = EWU_NONE;
    if (tid < d2) {
        const int x = (s_frame[tid >> 5] >> (tid & 31)) & 1;
        const int z = model == DQ_MODEL_X ? 0 : (s_frame[UFW_FRAME_WORDS + (tid >> 5)] >> (tid & 31)) & 1;
        int a0 = -1, a1 = -1;                                      // this qubit's wanted actions, ascending
        if (model == DQ_MODEL_X) { if (x) a0 = tid; }
        else if (use_Y) { if (x | z) a0 = (x ? (z ? 1 : 0) : 2) * d2 + tid; }
        else { if (x) a0 = tid; if (z) a1 = d2 + tid; }
        if (a0 >= 0 && !((comp[a0 >> 6] >> (a0 & 63)) & 1)) best = a0;
        else if (a1 >= 0 && !((comp[a1 >> 6] >> (a1 & 63)) & 1)) best = a1;
    }
    if (best != EWU_NONE) __hip_atomic_fetch_min(s_acc + 6, best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __syncthreads();
    const int a = s_acc[6];
    return a == EWU_NONE ? identity : a;
}

template <bool Weighted = false, bool Corr = false>
__global__ __launch_bounds__(UFW_THREADS) void env_wide_uf_kernel(EnvUfArgsOf<Weighted> p) {
    extern __shared__ __attribute__((aligned(16))) u8 smem[];
    const int tid = threadIdx.x;
    const size_t i = blockIdx.x;
    if ((int)blockIdx.x >= p.n_envs) return;                        // workgroup-uniform
    int32_t* out = p.action + i;
    UFW_IN_VGPR(out);
    const int a = env_wide_uf_action<Weighted, Corr>(p, i, p.state + i * p.sw, smem, tid);
    if (tid == 0) *out = a;
}

template <bool Weighted = false, bool Corr = false>
__global__ __launch_bounds__(UFW_THREADS) void env_wide_guided_uf_kernel(EnvUfArgsOf<Weighted> p) {
    extern __shared__ __attribute__((aligned(16))) u8 smem[];
    const int tid = threadIdx.x;
    const size_t i = blockIdx.x;
    if ((int)blockIdx.x >= p.n_envs) return;                        // workgroup-uniform
    const u64* rec = p.state + i * p.sw;
    u32 w[4];                                                       // the words dq_policy_select_wide draws for the lattice, drawn by every thread
    dq_policy_words(p.t, p.env_id_base + (u32)blockIdx.x, p.seed0, p.seed1, w);
    const u32 w0 = (u32)__builtin_amdgcn_readfirstlane((int)w[0]), w1 = (u32)__builtin_amdgcn_readfirstlane((int)w[1]);
    const u32 w2 = (u32)__builtin_amdgcn_readfirstlane((int)w[2]);
    const bool explore = dq_explores(p.q, w1, p.T_eps);
    const bool follow = explore && (u64)w2 < p.T_share;
    int32_t* out = p.action + i;
    u8* flag = p.guided ? p.guided + i : nullptr;
    int a;
    if (follow) {                                                   // workgroup-uniform: the only branch with barriers, the only one that touches LDS
        UFW_IN_VGPR(out); UFW_IN_VGPR(flag);
        a = env_wide_uf_action<Weighted, Corr>(p, i, rec, smem, tid);
    } else {
        if (tid >= 64) return;                                      // one wave suffices, and no barrier follows
        const u64* lg = rec + 3 * p.W + 2 + p.LW;                   // the record's legal set: what the last reset / step also wrote to its legal_dev
        const auto word = [=](int k) { return lg[k]; };
        a = explore ? dq_explore_action(p.LW, word, w0)             // common.h's rule, as policy_wide_kernel applies it
                    : __builtin_amdgcn_readfirstlane(dq_wave_first_max(p.q + i * p.n_actions, p.n_actions, tid, dq_admit_words(p.masked_greedy, word)));
    }
    if (tid == 0) {
        *out = a;
        if (flag) *flag = follow ? 1 : 0;
    }
}

// The one place that maps (guided, mode) to a kernel instantiation: f(kernel) gets the __global__ function, whose argument is EnvUfArgs for the unit weights
// and EnvUfArgsWeighted otherwise.  The launches (env_wide_uf_launch) and env_wide_uf_prepare's LDS limits both go through it.
template <class F>
void env_wide_uf_kernel_of(bool guided, UfwMode mode, F&& f) {
    ufw_with_mode(mode, [&](auto weighted, auto corr) {
        constexpr bool W = decltype(weighted)::value, K = decltype(corr)::value;
        guided ? f(env_wide_guided_uf_kernel<W, K>) : f(env_wide_uf_kernel<W, K>);
    });
}

// What both entry points check alike, before any device work: the handles, the decoder's lattice and window (DQ_ERR_INVALID); then the kernels' LDS limit, once per
// device (DQ_ERR_UNSUPPORTED).
dq_status env_wide_uf_prepare(const dq_envb* E, const dq_wide_uf* H, const int32_t* action_dev, const float* q_dev, const UfwWeights* w, EnvUfArgsWeighted* a,
                              const char* who) {
    DQ_REQUIRE(E && H && action_dev, DQ_ERR_INVALID, "%s: null argument", who);
    DQ_REQUIRE((reinterpret_cast<uintptr_t>(action_dev) & 3) == 0 && (reinterpret_cast<uintptr_t>(q_dev) & 3) == 0, DQ_ERR_INVALID,
               "%s: action_dev and q_dev must be 4-byte aligned", who);
    EnvbStateView S;
    const dq_status rc = envb_state_view(E, &S);
    if (rc != DQ_OK) return rc;
    DQ_REQUIRE(S.d == H->d && S.model == H->model, DQ_ERR_INVALID, "%s: the environment's lattice (d = %d, model %d) is not the decoder handle's (d = %d, model %d)", who,
               S.d, S.model, H->d, H->model);
    DQ_REQUIRE(S.depth >= 1 && S.depth <= EWU_MAX_DEPTH && H->window >= S.depth, DQ_ERR_INVALID,
               "%s: the decoder handle's window %d is below the environment's volume_depth %d", who, H->window, S.depth);
    DQ_REQUIRE(S.n_actions >= 1 && S.n_actions <= 64 * S.LW && S.sw == 3 * S.W + 2 + 2 * S.LW + S.depth * S.W, DQ_ERR_INVALID, "%s: inconsistent record", who);
    static unsigned long long attr_devs = 0;                          // per device (common.h dq_device_bit)
    const unsigned long long dev_bit = dq_device_bit();
    if (!(attr_devs & dev_bit)) {
        const int lds_max = ufw_layout((UFW_MAX_D * UFW_MAX_D - 1) / 2, UFW_MAX_D * UFW_MAX_D, EWU_MAX_DEPTH).bytes;
        const int lds_max_corr = ufw_lds_bytes(UFW_CORRELATED, lds_max, EWU_MAX_DEPTH);       // the correlated kernels carry their two masks behind that
        hipError_t ea = hipSuccess;
        for (int k = 0; k < 6; ++k) {                                // every (guided, mode)
            const UfwMode mode = (UfwMode)(k >> 1);
            env_wide_uf_kernel_of(k & 1, mode, [&](auto* kernel) {
                if (ea == hipSuccess)
                    ea = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                             ufw_lds_bytes(mode, lds_max, EWU_MAX_DEPTH));
            });
        }
        if (ea != hipSuccess) {
            (void)hipGetLastError();
            dq_set_error("%s: the device refuses %d bytes of LDS per workgroup: %s", who, lds_max_corr, hipGetErrorString(ea));
            return DQ_ERR_UNSUPPORTED;
        }
        attr_devs |= dev_bit;
    }
    memset(a, 0, sizeof(*a));
    a->c0 = UfwComp{H->ends, H->ends + 256};
    a->c1 = UfwComp{H->ends + 512, H->ends + 768};
    a->node_stab = H->node_stab; a->state = S.state; a->sw = S.sw; a->W = S.W; a->LW = S.LW; a->n_envs = S.n_envs; a->n = H->n; a->d2 = H->d2; a->depth = S.depth;
    a->model = S.model; a->use_Y = S.use_Y; a->identity = S.identity; a->n_actions = S.n_actions; a->env_id_base = S.env_id_base;
    a->action = const_cast<int32_t*>(action_dev);
    if (w) a->w = *w;
    return DQ_OK;
}

// (a unit-weight kernel takes the EnvUfArgs part of `a`)
void env_wide_uf_launch(bool guided, UfwMode mode, const EnvUfArgsWeighted& a, void* stream) {
    const int lds = ufw_lds_bytes(mode, ufw_layout(a.n, a.d2, a.depth).bytes, a.depth);
    env_wide_uf_kernel_of(guided, mode, [&](auto* kernel) { kernel<<<a.n_envs, UFW_THREADS, lds, (hipStream_t)stream>>>(a); });
}

// The select entry points: one body, `who` names the caller in the messages.  w: the weights of a weighted or a correlated launch (already checked), NULL for
// the unit-weight kernel.
dq_status env_wide_uf_select(const char* who, dq_envb* env, dq_wide_uf* H, int32_t* action_dev, void* stream, UfwMode mode = UFW_UNIT,
                             const UfwWeights* w = nullptr) {
    EnvUfArgsWeighted a;
    const dq_status rc = env_wide_uf_prepare(env, H, action_dev, nullptr, w, &a, who);
    if (rc != DQ_OK) return rc;
    env_wide_uf_launch(false, mode, a, stream);
    DQ_LAUNCH_CHECK();
    return DQ_OK;
}

dq_status env_wide_uf_guided_select(const char* who, dq_envb* env, dq_wide_uf* H, const float* q_dev, double eps, double guide_share, int masked_greedy,
                                    const uint32_t seed[2], uint64_t t, int32_t* action_dev, uint8_t* guided_dev, void* stream, UfwMode mode = UFW_UNIT,
                                    const UfwWeights* w = nullptr) {
    DQ_REQUIRE(seed, DQ_ERR_INVALID, "%s: null argument", who);
    DQ_REQUIRE(eps >= 0.0 && eps <= 1.0, DQ_ERR_INVALID, "%s: eps must be in [0,1]", who);                                    // (NaN fails both compares)
    DQ_REQUIRE(guide_share >= 0.0 && guide_share <= 1.0, DQ_ERR_INVALID, "%s: guide_share must be in [0,1]", who);
    EnvUfArgsWeighted a;
    const dq_status rc = env_wide_uf_prepare(env, H, action_dev, q_dev, w, &a, who);
    if (rc != DQ_OK) return rc;
    a.q = q_dev; a.T_eps = dq_rate_threshold(eps); a.T_share = dq_rate_threshold(guide_share); a.t = t; a.masked_greedy = masked_greedy;
    a.seed0 = seed[0]; a.seed1 = seed[1]; a.guided = guided_dev;
    env_wide_uf_launch(true, mode, a, stream);
    DQ_LAUNCH_CHECK();
    return DQ_OK;
}

}  // namespace

extern "C" {

dq_status dq_envb_uf_select(dq_envb* env, dq_wide_uf* H, int32_t* action_dev, void* stream) {
    return env_wide_uf_select("dq_envb_uf_select", env, H, action_dev, stream);
}

dq_status dq_envb_uf_select_weighted(dq_envb* env, dq_wide_uf* H, int w_space, int w_time, const uint8_t* weights_each_dev, int32_t* action_dev, void* stream) {
    const UfwWeights w = {weights_each_dev, w_space, w_time, 1};
    const dq_status rc = ufw_check_weights(UFW_WEIGHTED, 0, w, true, "dq_envb_uf_select_weighted");
    if (rc != DQ_OK) return rc;
    return env_wide_uf_select("dq_envb_uf_select_weighted", env, H, action_dev, stream, UFW_WEIGHTED, &w);
}

dq_status dq_envb_uf_select_correlated(dq_envb* env, dq_wide_uf* H, int w_space, int w_time, int w_corr, const uint8_t* weights_each_dev, int32_t* action_dev,
                                       void* stream) {
    const UfwWeights w = {weights_each_dev, w_space, w_time, w_corr};
    const dq_status rc = ufw_check_weights(UFW_CORRELATED, 0, w, true, "dq_envb_uf_select_correlated");
    if (rc != DQ_OK) return rc;
    return env_wide_uf_select("dq_envb_uf_select_correlated", env, H, action_dev, stream, UFW_CORRELATED, &w);
}

dq_status dq_envb_guided_select_uf(dq_envb* env, dq_wide_uf* H, const float* q_dev, double eps, double guide_share, int masked_greedy, const uint32_t seed[2],
                                   uint64_t t, int32_t* action_dev, uint8_t* guided_dev, void* stream) {
    return env_wide_uf_guided_select("dq_envb_guided_select_uf", env, H, q_dev, eps, guide_share, masked_greedy, seed, t, action_dev, guided_dev, stream);
}

dq_status dq_envb_guided_select_uf_weighted(dq_envb* env, dq_wide_uf* H, const float* q_dev, double eps, double guide_share, int masked_greedy,
                                            const uint32_t seed[2], uint64_t t, int w_space, int w_time, const uint8_t* weights_each_dev, int32_t* action_dev,
                                            uint8_t* guided_dev, void* stream) {
    const UfwWeights w = {weights_each_dev, w_space, w_time, 1};
    const dq_status rc = ufw_check_weights(UFW_WEIGHTED, 0, w, true, "dq_envb_guided_select_uf_weighted");
    if (rc != DQ_OK) return rc;
    return env_wide_uf_guided_select("dq_envb_guided_select_uf_weighted", env, H, q_dev, eps, guide_share, masked_greedy, seed, t, action_dev, guided_dev, stream,
                                     UFW_WEIGHTED, &w);
}

dq_status dq_envb_guided_select_uf_correlated(dq_envb* env, dq_wide_uf* H, const float* q_dev, double eps, double guide_share, int masked_greedy,
                                              const uint32_t seed[2], uint64_t t, int w_space, int w_time, int w_corr, const uint8_t* weights_each_dev,
                                              int32_t* action_dev, uint8_t* guided_dev, void* stream) {
    const UfwWeights w = {weights_each_dev, w_space, w_time, w_corr};
    const dq_status rc = ufw_check_weights(UFW_CORRELATED, 0, w, true, "dq_envb_guided_select_uf_correlated");
    if (rc != DQ_OK) return rc;
    return env_wide_uf_guided_select("dq_envb_guided_select_uf_correlated", env, H, q_dev, eps, guide_share, masked_greedy, seed, t, action_dev, guided_dev,
                                     stream, UFW_CORRELATED, &w);
}

}  // extern "C"
